"""Time the DQN loop with one learner per UAV slot (csrc/loop.hip: UavDqnSlotsLoop, loop.DQNSlotsHotLoop) against the composition
of the entry points that existed before it, which is what the same bytes cost without it.

Shapes: U = 4 x 16 384 envs and U = 2 x 32 768 envs (N = 65 536 agents), batch 16 384 per slot, a packed ring of >= 1 M
transitions, untrained Qnet2, eps 0.1, auto-reset.
  loop   DQNSlotsHotLoop.run(passes): per pass uavenv_dqn_act_slots, uavenv_step, uavenv_replay_draw_slots and per slot
         uavenv_dqn_grad + uavenv_dqn_reduce_adam, enqueued from C;
  comp   per pass and slot a strided gather of the slot's rows, uavenv_dqn_act under seed + j and a scatter of the actions;
         uavenv_step; uavenv_replay_draw over U x batch draws turned into (frame, agent) pairs; per slot learn_from_ring on its
         slice -- issued from Python.
First both forms run a short stretch from the same start and every ring plane and every learner's parameters must be equal, bit
for bit.  Then both are warmed up and timed with device events around windows of `--passes` passes, the two forms alternating in
one process; the median of `--windows` windows is reported with their spread (min .. max).
    python scripts/time_slots_loop.py [--passes 2000] [--windows 5] [--out profiles/dqn_slots_loop_times.json]
    python scripts/time_slots_loop.py --profile-run     (the C loop alone, for rocprofv3 --kernel-trace --stats in its own process)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dqn_based_uav_3d_path_planer_amd import _lib  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.data import make_city26_env  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing  # noqa: E402

PARAM = {"NetWork": "Qnet2", "w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99",
         "Update_loop": "3"}
SEED, EPS, M64 = 9, 0.1, (1 << 64) - 1


def build(n_envs, U, ring_transitions):
    env = make_city26_env(n_envs, obs_dtype="packed", uav_per_env=U)
    ring = DeviceReplayRing(env, ring_transitions, discrete=True)
    ring.reset(seed=12)
    Ls = []
    for j in range(U):
        torch.manual_seed(1 + j)
        Ls.append(FusedDQNLearner(PARAM, "dqn", device="cuda:0"))
    return env, ring, Ls


class Composition:
    def __init__(self, ring, Ls, batch):
        self.ring, self.Ls, self.batch, self.counter = ring, Ls, batch, 0
        self.lib = _lib.load()
        U = len(Ls)
        self.n_envs = ring.env.N // U
        d = ring.env.device
        self.draws = torch.zeros((U * batch, 2), dtype=torch.int32, device=d)
        self.slot = (torch.arange(U * batch, device=d) // batch).to(torch.int32)
        self.a = torch.empty(self.n_envs, dtype=torch.int32, device=d)

    def run(self, passes):
        ring, Ls, B, U = self.ring, self.Ls, self.batch, len(self.Ls)
        s = torch.cuda.current_stream(ring.env.device).cuda_stream
        for _ in range(passes):
            c = self.counter
            obs, act = ring.current_obs(), ring.current_action()
            for j, L in enumerate(Ls):
                L.act(obs[j::U].contiguous(), EPS, (SEED + j) & M64, c, index_out=self.a)
                act[j::U] = self.a
            ring.step_env(auto_reset=True, skip_done=True)
            if ring.filled * self.n_envs >= B:
                _lib.check(self.lib.uavenv_replay_draw(ring.frames, self.n_envs, ring.head, ring.filled, U * B, SEED + 7, c,
                                                       self.draws.data_ptr(), s), "uavenv_replay_draw")
                self.draws[:, 1] = self.draws[:, 1] * U + self.slot
                for j, L in enumerate(Ls):
                    L.learn_from_ring(ring, B, SEED, c, explicit_idx=self.draws[j * B:(j + 1) * B])
            self.counter += 1


def window(fn, passes):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn(passes)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / passes          # us per pass


def measure(n_envs, U, batch, ring_transitions, passes, windows, check_passes):
    env_a, ring_a, La = build(n_envs, U, ring_transitions)
    env_b, ring_b, Lb = build(n_envs, U, ring_transitions)
    comp = Composition(ring_a, La, batch)
    loop = DQNSlotsHotLoop(ring_b, Lb, batch, seed=SEED, eps=EPS, auto_reset=True, skip_done=True)
    comp.run(check_passes)
    loop.run(check_passes)
    torch.cuda.synchronize()
    equal = all(torch.equal(getattr(ring_a, k), getattr(ring_b, k)) for k in ("obs", "action", "reward", "done", "valid"))
    equal = equal and all(torch.equal(a.flat, b.flat) and a.epoch == b.epoch for a, b in zip(La, Lb))
    equal = equal and (ring_a.head, ring_a.filled) == (ring_b.head, ring_b.filled) and La[0].epoch > 0
    if not equal:
        raise SystemExit(f"U={U}: the C loop and the composition differ after {check_passes} passes")
    warm = max(50, passes // 10)
    comp.run(warm)
    loop.run(warm)
    t_loop, t_comp = [], []
    for _ in range(windows):                          # the two forms alternate
        t_loop.append(window(loop.run, passes))
        t_comp.append(window(comp.run, passes))
    N = env_a.N
    res = {"uav_per_env": U, "n_envs": n_envs, "agents": N, "batch_per_slot": batch, "ring_frames": ring_a.frames,
           "ring_transitions": (ring_a.frames - 1) * N, "passes_per_window": passes, "windows": windows,
           "equal_after_passes": check_passes, "launches_per_pass_loop": 3 + 2 * U}
    for name, t in (("loop", t_loop), ("composition", t_comp)):
        med = float(np.median(t))
        res[name] = {"us_per_pass_windows": [round(x, 3) for x in t], "us_per_pass_median": round(med, 3),
                     "us_per_pass_min": round(min(t), 3), "us_per_pass_max": round(max(t), 3),
                     "agent_steps_per_s": round(N / med * 1e6), "updates_per_s": round(U / med * 1e6)}
    res["speedup_median"] = round(res["composition"]["us_per_pass_median"] / res["loop"]["us_per_pass_median"], 3)
    # the condition: the C loop's pass is not slower than the composition's beyond the spread of the windows
    spread = max(max(t_loop) - min(t_loop), max(t_comp) - min(t_comp))
    res["loop_not_slower_beyond_spread"] = bool(res["loop"]["us_per_pass_median"] <= res["composition"]["us_per_pass_median"] + spread)
    loop.close()
    env_a.close()
    env_b.close()
    return res


def profile_run(passes):
    env, ring, Ls = build(16384, 4, 1 << 20)
    loop = DQNSlotsHotLoop(ring, Ls, 16384, seed=SEED, eps=EPS, auto_reset=True, skip_done=True)
    loop.run(passes)
    torch.cuda.synchronize()
    loop.close()
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--check-passes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "dqn_slots_loop_times.json"))
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    if a.profile_run:
        profile_run(min(a.passes, 500))
        return
    out = {"device": torch.cuda.get_device_name(0), "method": "device events around windows of passes, both forms warmed up, "
           "alternating in one process, median of the windows; spread = min .. max of the windows",
           "shapes": [measure(16384, 4, 16384, 1 << 20, a.passes, a.windows, a.check_passes),
                      measure(32768, 2, 16384, 1 << 20, a.passes, a.windows, a.check_passes)]}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
