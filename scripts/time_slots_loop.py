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
--multi-update times the C loop against itself: its learning phase slot by slot (U gradient and U Adam launches per pass) and as
one gradient and one Adam launch for all slots (DQNSlotsHotLoop(multi_update=True): uavenv_dqn_grad_slots,
uavenv_dqn_reduce_adam_slots), same shapes, same method, both forms first checked equal on a short run.  Each shape is measured
by a child process of its own under a time limit; the first failure ends the run.
    python scripts/time_slots_loop.py --multi-update [--out profiles/dqn_slots_update_times.json]
    python scripts/time_slots_loop.py --multi-update --profile-run     (the multi-update loop alone, for rocprofv3)
--per times prioritised replay (one replay.DevicePER per slot): the C loop with DQNSlotsHotLoop(pers=...) -- every phase one launch for
all slots, 10 launches per pass -- against the composition of the per-tree entry points issued from Python (per slot
uavenv_per_rebuild_frame, uavenv_per_sample, uavenv_per_weights, the weighted update, uavenv_per_set_f32_gated), both checked equal
on a short run first (ring planes, parameters, every tree's priorities, beta); the uniform multi-update loop of the same process is
recorded next to them for information.  Same shapes, same method, one child process per shape.
    python scripts/time_slots_loop.py --per [--out profiles/dqn_slots_per_times.json]
    python scripts/time_slots_loop.py --per --profile-run     (the prioritised C loop alone, 500 passes at U = 4, for rocprofv3)
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
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


class PerComposition:
    """The prioritised pass as the per-tree entry points give it, issued from Python slot by slot."""

    def __init__(self, ring, Ls, pers, batch):
        self.ring, self.Ls, self.pers, self.batch, self.counter = ring, Ls, pers, batch, 0
        self.lib = _lib.load()
        self.n_envs = ring.env.N // len(Ls)
        self.a = torch.empty(self.n_envs, dtype=torch.int32, device=ring.env.device)
        self.bufs = [p.make_bufs(batch) for p in pers]
        self.beta = pers[0].beta

    def run(self, passes):
        import ctypes as C
        import math
        ring, Ls, pers, B, U, lib, n_envs = self.ring, self.Ls, self.pers, self.batch, len(self.Ls), self.lib, self.n_envs
        s = torch.cuda.current_stream(ring.env.device).cuda_stream
        p0 = pers[0]
        per_new = math.pow(0.0 + p0.epsilon, p0.alpha)
        for _ in range(passes):
            c = self.counter
            obs, act = ring.current_obs(), ring.current_action()
            for j, L in enumerate(Ls):
                L.act(obs[j::U].contiguous(), EPS, (SEED + j) & M64, c, index_out=self.a)
                act[j::U] = self.a
            t = ring.head
            ring.step_env(auto_reset=True, skip_done=True)
            nxt, valid_t = ring.head, ring.valid[t]
            learn = ring.filled * n_envs >= B
            if learn:
                self.beta = self.beta + p0.beta_inc if self.beta + p0.beta_inc < 1.0 else 1.0
            for j, (L, p, b) in enumerate(zip(Ls, pers, self.bufs)):
                per = C.byref(p._c)
                if not learn:
                    _lib.check(lib.uavenv_per_fill_frame_strided(per, t * n_envs, n_envs, per_new, valid_t.data_ptr() + j, U,
                                                                 nxt * n_envs, s), "uavenv_per_fill_frame_strided")
                    continue
                col = valid_t[j::U].contiguous()
                _lib.check(lib.uavenv_per_rebuild_frame(per, t * n_envs, n_envs, per_new, col.data_ptr(), nxt * n_envs, s), "rebuild")
                _lib.check(lib.uavenv_per_sample(per, B, None, (SEED + 7 + j) & M64, c, b["slots"].data_ptr(), b["prio"].data_ptr(), s),
                           "sample")
                _lib.check(lib.uavenv_per_weights(per, b["slots"].data_ptr(), b["prio"].data_ptr(), B, ring.filled * n_envs, self.beta,
                                                  n_envs, b["w"].data_ptr(), b["pairs"].data_ptr(), s), "weights")
                b["pairs"][:, 1] = b["pairs"][:, 1] * U + j
                L.learn_from_ring(ring, B, SEED, c, explicit_idx=b["pairs"], is_weights=b["w"], abs_td_out=b["abs"])
                _lib.check(lib.uavenv_per_set_f32_gated(per, b["slots"].data_ptr(), b["abs"].data_ptr(), B, p.epsilon, p.alpha, p.clip,
                                                        None, 0, s), "set")
            self.counter += 1


def measure_per(n_envs, U, batch, ring_transitions, passes, windows, check_passes):
    """The prioritised C loop against the prioritised composition from the same start; the uniform multi-update loop beside them."""
    from dqn_based_uav_3d_path_planer_amd.replay import DevicePER
    env_a, ring_a, La = build(n_envs, U, ring_transitions)
    env_b, ring_b, Lb = build(n_envs, U, ring_transitions)
    env_c, ring_c, Lc = build(n_envs, U, ring_transitions)
    pers_a = [DevicePER(ring_a.frames * n_envs, device="cuda:0", tree_order=False) for _ in range(U)]
    pers_b = [DevicePER(ring_b.frames * n_envs, device="cuda:0", tree_order=False) for _ in range(U)]
    comp = PerComposition(ring_a, La, pers_a, batch)
    loop = DQNSlotsHotLoop(ring_b, Lb, batch, seed=SEED, eps=EPS, auto_reset=True, skip_done=True, pers=pers_b)
    uniform = DQNSlotsHotLoop(ring_c, Lc, batch, seed=SEED, eps=EPS, auto_reset=True, skip_done=True, multi_update=True)
    comp.run(check_passes)
    loop.run(check_passes)
    torch.cuda.synchronize()
    equal = all(torch.equal(getattr(ring_a, k), getattr(ring_b, k)) for k in ("obs", "action", "reward", "done", "valid"))
    equal = equal and all(torch.equal(a.flat, b.flat) and a.epoch == b.epoch and float(a.loss) == float(b.loss) for a, b in zip(La, Lb))
    equal = equal and (ring_a.head, ring_a.filled) == (ring_b.head, ring_b.filled) and La[0].epoch > 0
    equal = equal and all(torch.equal(a.prio, b.prio) and torch.equal(a._chunk_prefix, b._chunk_prefix) for a, b in zip(pers_a, pers_b))
    equal = equal and comp.beta == pers_b[0].beta and bool((pers_b[0].prio > 0).any())
    if not equal:
        raise SystemExit(f"U={U}: the prioritised C loop and the composition differ after {check_passes} passes")
    warm = max(50, passes // 10)
    for f in (comp, loop, uniform):
        f.run(warm)
    t_loop, t_comp, t_uni = [], [], []
    for _ in range(windows):                          # the forms alternate
        t_loop.append(window(loop.run, passes))
        t_comp.append(window(comp.run, passes))
        t_uni.append(window(uniform.run, passes))
    N = env_a.N
    res = {"uav_per_env": U, "n_envs": n_envs, "agents": N, "batch_per_slot": batch, "ring_frames": ring_a.frames,
           "ring_transitions": (ring_a.frames - 1) * N, "passes_per_window": passes, "windows": windows,
           "equal_after_passes": check_passes, "launches_per_pass_loop": 10, "launches_per_pass_per_slot_calls": 3 + 9 * U,
           "launches_per_pass_uniform_multi_update": 5}
    for name, t in (("loop", t_loop), ("composition", t_comp), ("uniform_multi_update_for_information", t_uni)):
        med = float(np.median(t))
        res[name] = {"us_per_pass_windows": [round(x, 3) for x in t], "us_per_pass_median": round(med, 3),
                     "us_per_pass_min": round(min(t), 3), "us_per_pass_max": round(max(t), 3),
                     "agent_steps_per_s": round(N / med * 1e6), "updates_per_s": round(U / med * 1e6)}
    res["speedup_median"] = round(res["composition"]["us_per_pass_median"] / res["loop"]["us_per_pass_median"], 3)
    # the condition for switching the plugin over: the loop's slowest window beats the composition's fastest
    res["loop_faster_beyond_spread"] = bool(max(t_loop) < min(t_comp))
    res["device"] = torch.cuda.get_device_name(0)
    loop.close()
    uniform.close()
    for e in (env_a, env_b, env_c):
        e.close()
    return res


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


def measure_update(n_envs, U, batch, ring_transitions, passes, windows, check_passes):
    """The C loop with per-slot updates against the C loop with multi_update, from the same start."""
    env_a, ring_a, La = build(n_envs, U, ring_transitions)
    env_b, ring_b, Lb = build(n_envs, U, ring_transitions)
    per_slot = DQNSlotsHotLoop(ring_a, La, batch, seed=SEED, eps=EPS, auto_reset=True, skip_done=True)
    multi = DQNSlotsHotLoop(ring_b, Lb, batch, seed=SEED, eps=EPS, auto_reset=True, skip_done=True, multi_update=True)
    per_slot.run(check_passes)
    multi.run(check_passes)
    torch.cuda.synchronize()
    equal = all(torch.equal(getattr(ring_a, k), getattr(ring_b, k)) for k in ("obs", "action", "reward", "done", "valid"))
    equal = equal and all(torch.equal(a.flat, b.flat) and a.epoch == b.epoch and float(a.loss) == float(b.loss) for a, b in zip(La, Lb))
    equal = equal and (ring_a.head, ring_a.filled) == (ring_b.head, ring_b.filled) and La[0].epoch > 0
    if not equal:
        raise SystemExit(f"U={U}: the per-slot and the multi-update loop differ after {check_passes} passes")
    warm = max(50, passes // 10)
    per_slot.run(warm)
    multi.run(warm)
    t_per, t_multi = [], []
    for _ in range(windows):                          # the two forms alternate
        t_multi.append(window(multi.run, passes))
        t_per.append(window(per_slot.run, passes))
    N = env_a.N
    res = {"uav_per_env": U, "n_envs": n_envs, "agents": N, "batch_per_slot": batch, "ring_frames": ring_a.frames,
           "ring_transitions": (ring_a.frames - 1) * N, "passes_per_window": passes, "windows": windows,
           "equal_after_passes": check_passes, "launches_per_pass_per_slot": 3 + 2 * U, "launches_per_pass_multi_update": 5}
    for name, t in (("per_slot", t_per), ("multi_update", t_multi)):
        med = float(np.median(t))
        res[name] = {"us_per_pass_windows": [round(x, 3) for x in t], "us_per_pass_median": round(med, 3),
                     "us_per_pass_min": round(min(t), 3), "us_per_pass_max": round(max(t), 3),
                     "agent_steps_per_s": round(N / med * 1e6), "updates_per_s": round(U / med * 1e6)}
    res["speedup_median"] = round(res["per_slot"]["us_per_pass_median"] / res["multi_update"]["us_per_pass_median"], 3)
    # the condition for switching a caller over: the multi form's slowest window beats the per-slot form's fastest
    res["multi_update_faster_beyond_spread"] = bool(max(t_multi) < min(t_per))
    res["device"] = torch.cuda.get_device_name(0)
    per_slot.close()
    multi.close()
    env_a.close()
    env_b.close()
    return res


ROWS = ((16384, 4), (32768, 2))                       # (envs, UAV slots): N = 65 536 agents


def multi_update_rows(a):
    """One child process per shape, each under its own time limit; the first failure ends the run."""
    shapes = []
    mode = "--per" if a.per else "--multi-update"
    for n_envs, U in ROWS:
        cmd = ["timeout", "-k", "10", str(a.row_timeout), sys.executable, os.path.abspath(__file__), mode, "--row",
               str(n_envs), str(U), "--passes", str(a.passes), "--windows", str(a.windows), "--check-passes", str(a.check_passes)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"the shape {n_envs} x {U} ended with status {r.returncode}: nothing further is started")
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(shapes[-1]), flush=True)
    key = "loop_faster_beyond_spread" if a.per else "multi_update_faster_beyond_spread"
    return {"device": shapes[0]["device"], "method": "device events around windows of passes, both forms warmed up, alternating in one "
            "process per shape, median of the windows; spread = min .. max of the windows", "shapes": shapes,
            key + "_at_every_shape": all(x[key] for x in shapes)}


def profile_run(passes, multi_update=False, per=False):
    env, ring, Ls = build(16384, 4, 1 << 20)
    pers = None
    if per:
        from dqn_based_uav_3d_path_planer_amd.replay import DevicePER
        pers = [DevicePER(ring.frames * 16384, device="cuda:0", tree_order=False) for _ in range(4)]
    loop = DQNSlotsHotLoop(ring, Ls, 16384, seed=SEED, eps=EPS, auto_reset=True, skip_done=True, multi_update=multi_update, pers=pers)
    loop.run(passes)
    torch.cuda.synchronize()
    loop.close()
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--check-passes", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--multi-update", action="store_true")
    ap.add_argument("--per", action="store_true")
    ap.add_argument("--row", type=int, nargs=2, metavar=("ENVS", "SLOTS"), help="(--multi-update's / --per's children) measure this shape only")
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds a --multi-update / --per shape may take")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join("profiles", "dqn_slots_per_times.json" if a.per else
                             "dqn_slots_update_times.json" if a.multi_update else "dqn_slots_loop_times.json")
    if (a.multi_update or a.per) and not a.profile_run and a.row is None:     # (the parent never opens the device)
        out = multi_update_rows(a)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    assert torch.cuda.is_available(), "needs an MI355X"
    if a.profile_run:
        profile_run(min(a.passes, 500), multi_update=a.multi_update, per=a.per)
        return
    if a.row is not None:
        fn = measure_per if a.per else measure_update
        print(json.dumps(fn(a.row[0], a.row[1], 16384, 1 << 20, a.passes, a.windows, a.check_passes)))
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
