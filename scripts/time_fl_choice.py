"""Time one selective federated merge (Federated_Learning_choice, <FL_Aggregate>choice</FL_Aggregate>) of U DQN slot learners on
S = 10 replayed states each, U = 4 and U = 8:
  device  federated.choice_merge_blocks: ONE uavenv_fed_choice launch on the packed ring rows;
  torch   federated.choice_merge_modules on the SAME learners' q_local modules (views of the same flat blocks, on the GPU) and
          the same rows unpacked -- the restatement tests/golden/federated_choice.npz pins: U^2 small forwards, one read-back of
          the distances per UAV, a state-dict loop per UAV.
Both forms start every repeat from the same blocks (restored outside the timed span).  Device events round each form on the
current stream plus host wall time (the torch form waits for the device inside: its event time is a wall time too); a warm-up of
both, then the two forms alternating in one process, medians of the repeats.  Before any time is taken the two forms' chosen lists
must agree.
    python scripts/time_fl_choice.py [--reps 30] [--out profiles/fl_choice_times.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dqn_based_uav_3d_path_planer_amd import federated  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.data import make_city26_env  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing  # noqa: E402

PARAM = {"NetWork": "VAnet2", "w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99",
         "Update_loop": "3"}
S = federated.CHOICE_STATES


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6       # microseconds


def one(U, reps, warmup=3):
    n = 128 * U
    env = make_city26_env(n, obs_dtype="packed")          # agent e * U + j counts as slot j's row: all the draw needs
    ring = DeviceReplayRing(env, 4 * n, discrete=True)
    ring.reset(seed=4)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(3):
        ring.current_action().copy_(torch.randint(0, 3, (n,), generator=gen, device="cuda", dtype=torch.int32))
        ring.step_env(auto_reset=True)
    torch.manual_seed(7)
    Ls = [FusedDQNLearner(PARAM, kind="dueling", device="cuda:0") for _ in range(U)]
    pairs = federated.draw_slot_pairs(ring, U, S, seed=11, counter=0)
    pr = pairs.long()
    states = [env.unpack(ring.obs[pr[p, :, 0], pr[p, :, 1]]) for p in range(U)]
    start = [L.flat[0].clone() for L in Ls]

    def restore():
        for L, w in zip(Ls, start):
            L.flat[0].copy_(w)

    def device():
        return federated.choice_merge_blocks(Ls, ring.obs, pairs)

    def torch_form():
        return federated.choice_merge_modules([L.q_local for L in Ls], states)

    restore()
    _, chosen, status = device()
    got = [[c for c in row if c >= 0] for row in chosen.cpu().tolist()]
    dev_blocks = [L.flat[0].clone() for L in Ls]
    restore()
    want = torch_form()
    assert int(status.cpu()[0]) == 0 and got == want, (got, want)
    same = all(torch.equal(a, L.flat[0]) for a, L in zip(dev_blocks, Ls))
    t = {"device": [], "torch": []}
    for i in range(warmup + reps):
        for name, fn in (("device", device), ("torch", torch_form)):
            restore()
            ev, wall = timed(fn)
            if i >= warmup:
                t[name].append((ev, wall))
    env.close()
    med = {k: [float(np.median([x[i] for x in v])) for i in range(2)] for k, v in t.items()}
    return {"U": U, "S": S, "chosen": got, "blocks_bit_equal_between_forms": bool(same), "reps": reps,
            "device_us_events": round(med["device"][0], 1), "device_us_wall": round(med["device"][1], 1),
            "torch_us_events": round(med["torch"][0], 1), "torch_us_wall": round(med["torch"][1], 1),
            "speedup_wall": round(med["torch"][1] / med["device"][1], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "fl_choice_times.json"))
    a = ap.parse_args()
    res = {"what": "one selective federated merge, S = 10 states per UAV, VAnet2 100-64-3; medians, microseconds",
           "gpu": torch.cuda.get_device_name(0), "cases": [one(U, a.reps) for U in (4, 8)]}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
