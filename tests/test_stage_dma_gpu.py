"""LDS-DMA staging (global_load_lds) of the layer-1 images and the world blob in k_step_coop<policy> and k_dqn_grad_packed8<2>:
the same bytes land in LDS as with the register-staged form, so the C loop computes the same thing bit for bit either way.
UAVENV_STAGE_VGPR=1 selects the register-staged form; the knob is read once per process, so every form runs in a fresh child
process under its own time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# BASELINE configs[1] as bench.py runs it: 16 384 envs, batch 16 384, packed ring of 1 M transitions (64 frames), f32 DQN.
# 40 passes leave the ring partly filled, 100 wrap it.
CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
from dqn_based_uav_3d_path_planer_amd.loop import HotLoop
from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
out, passes = sys.argv[2], int(sys.argv[3])
N = 16384
torch.cuda.set_device(0)
env = make_city26_env(N, obs_dtype="packed")
ring = DeviceReplayRing(env, 1 << 20, discrete=True)
ring.reset(seed=1000)
torch.manual_seed(42)
L = FusedDQNLearner({"NetWork": "Qnet2", "w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001",
                     "gamma": "0.99", "Update_loop": "3"}, "dqn", device="cuda:0")
loop = HotLoop(ring, L, N, seed=7, eps=0.1)
loop.run(passes)
torch.cuda.synchronize()
np.savez(out, obs=ring.obs.cpu().numpy().view(np.uint8), action=ring.action.cpu().numpy(), reward=ring.reward.cpu().numpy(),
         done=ring.done.cpu().numpy(), flat=L.flat.cpu().numpy(), loss=L.loss.cpu().numpy(), head=np.int64(ring.head),
         filled=np.int64(ring.filled))
"""


def _run(tmp_path, tag, passes, stage_vgpr):
    env = dict(os.environ)
    env.pop("UAVENV_STAGE_VGPR", None)
    if stage_vgpr:
        env["UAVENV_STAGE_VGPR"] = "1"
    out = str(tmp_path / ("%s.npz" % tag))
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, ROOT, out, str(passes)], env=env, check=True,
                   timeout=330)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("passes", [40, 100])
def test_c_loop_identical_with_lds_dma_and_register_staging(tmp_path, passes):
    dma = _run(tmp_path, "dma_%d" % passes, passes, False)
    vgpr = _run(tmp_path, "vgpr_%d" % passes, passes, True)
    assert int(dma["filled"]) == int(vgpr["filled"])
    if passes == 40:
        assert int(dma["filled"]) < 63      # the ring is not yet full
    for k in dma:
        assert dma[k].tobytes() == vgpr[k].tobytes(), k
    assert np.isfinite(dma["loss"]).all() and float(dma["loss"]) > 0.0
