"""Fixtures shared by the DQN kernel tests (tests/test_dqn_grad_kernels_gpu.py, tests/test_dqn_act_kernels_gpu.py,
tests/test_dqn_act_ref.py): the pool of observation rows the environment really produces, and the nets the acting tests use --
a golden's trained weights as a flat block, carried to other head sizes, and blocks with two identical layer-2 rows."""
import numpy as np

from oracle.dqn_grad_ref import layout, unflatten

W, HID = 100, 64


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


class Pool:
    """Observation rows the environment really produces (packed-representable), and a real packed ring that has wrapped."""

    def __init__(self):
        from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
        from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
        n = 2048
        self.env = make_city26_env(n, obs_dtype="packed")
        self.ring = DeviceReplayRing(self.env, 4 * n, discrete=True)
        assert self.ring.frames == 5
        import torch
        self.ring.reset(seed=4)
        gen = torch.Generator(device="cuda").manual_seed(1)
        for _ in range(8):                                       # 8 steps on 5 frames: wrapped
            self.ring.current_action().copy_(torch.randint(0, 3, (n,), generator=gen, device="cuda", dtype=torch.int32))
            self.ring.step_env(auto_reset=True)
        torch.cuda.synchronize()
        assert self.ring.filled == 4 and self.ring.head == 3
        self.obs = unpack(self.ring.obs)                         # [frames, n, 100] f32, exact
        self.rows = self.obs.reshape(-1, 100)


def unpack(obs_packed):
    import torch
    L = _lib()
    f, n = obs_packed.shape[:2]
    out = torch.empty((f * n, 100), dtype=torch.float32, device=obs_packed.device)
    assert L.load().uavenv_obs_unpack(obs_packed.data_ptr(), f * n, out.data_ptr(), L.OBS_F32,
                                      torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return out.view(f, n, 100).cpu().numpy()


def widen_head(flat3, n_actions: int, dueling: bool):
    """A trained three-action block (a golden's weights after its updates) carried to another head size: layer 1 as it is, action
    k takes row k mod 3 of the three-action head scaled by 1 + (k div 3) / 8 (weights and bias; distinct rows, so no ties), the value
    row as it is.  The |Q| and term mass of the trained net at every head the kernels take."""
    A = int(n_actions)
    n3 = 3 + (1 if dueling else 0)
    W1, b1, W2, b2 = unflatten(flat3, W, HID, n3)
    rows = [W2[k % 3] * (1.0 + (k // 3) / 8.0) for k in range(A)] + ([W2[3]] if dueling else [])
    bias = [b2[k % 3] * (1.0 + (k // 3) / 8.0) for k in range(A)] + ([b2[3]] if dueling else [])
    return np.concatenate([W1.ravel(), b1, np.concatenate(rows), np.array(bias)]).astype(np.float32)


def golden_flat(g: dict, pref: str, dueling: bool):
    """The flat block of a learner golden's state dict with key prefix pref ("l0_", "l1_", ...)."""
    keys = ["fc1.weight", "fc1.bias"] + (["fc_A.weight", "fc_V.weight", "fc_A.bias", "fc_V.bias"] if dueling
                                         else ["fc2.weight", "fc2.bias"])
    return np.concatenate([np.asarray(g[pref + k], dtype=np.float32).ravel() for k in keys])


def tie_rows(flat_params, n_actions: int, dueling: bool, a: int, b: int, others_below: float = 30.0):
    """A copy of the flat block in which outputs a < b of layer 2 are IDENTICAL (weights and bias: Q_a == Q_b bit for bit in any
    arithmetic that treats the rows alike) and every other action's bias lies others_below under theirs."""
    A = int(n_actions)
    n2 = A + (1 if dueling else 0)
    fl = np.array(flat_params, dtype=np.float32).reshape(-1).copy()
    _, o_w2, o_b2, P = layout(W, HID, n2)
    assert fl.size == P and 0 <= a < b < A
    fl[o_w2 + b * HID:o_w2 + (b + 1) * HID] = fl[o_w2 + a * HID:o_w2 + (a + 1) * HID]
    fl[o_b2 + b] = fl[o_b2 + a]
    for k in range(A):
        if k not in (a, b):
            fl[o_b2 + k] = fl[o_b2 + a] - np.float32(others_below)
    return fl
