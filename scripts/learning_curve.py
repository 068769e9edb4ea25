"""Does the fused training loop learn?  BASELINE configs[1] as bench.py runs it (HotLoop: C-enqueued act -> step -> learn, DQN,
packed replay ring), with a greedy evaluation of held-out city26 episodes (uavenv_eval_episodes) every --every passes.

The settings (envs, learner batch, replay capacity, trainer, training epsilon, reset bank) come from bench.py's own defaults
(bench.parse()), so this measures the loop the benchmark times.  Baselines at pass 0: the untrained net (greedy), eps = 1 (the
uniform random policy) and the scripted baseline (sub-goal pursuit among the same three actions, no learning:
uavenv_eval_episodes_scripted) with look-ahead 0 and 8.  Held-out rows are planned on a seed the training bank never uses.  Output: one JSON document.
    python scripts/learning_curve.py [--passes 1000000] [--every 50000] [--episodes 16384] [--out profiles/learning_curve_configs1.json]
--actions N (configs[1] only; default 3, bench.py's): the same run with a steering table of N actions, 2 <= N + (1 for a dueling
trainer) <= 14 -- above 4 layer-2 outputs the evaluations go through the wide instantiation of the episode kernel; the scripted baseline
chooses among the same N actions.  Output: profiles/learning_curve_configs1_aN.json.

--config 2: BASELINE configs[2] as `bench.py --config 3` builds it (65 536 envs, dueling + DDQN, f16 observation rows, the f16-MFMA
learner, HotLoop), evaluated through uavenv_eval_episodes_f16: the f16 policy the learner acts with, on the halves the f16 ring
feeds it.  Same baselines, same held-out rows.
    python scripts/learning_curve.py --config 2 [--passes 1000000] [--every 50000] [--episodes 16384] [--out profiles/learning_curve_configs2.json]

--config 3: BASELINE configs[3] as `bench.py --config 4` builds it (run_config4: 4 UAV slots x 32 768 envs, APF on with the
velocities of default_rng(42), one fused SAC learner per slot, SACHotLoop), with a held-out evaluation of the four actors in one
launch (uavenv_eval_episodes_sac) every --every passes, in both modes ("mean": noise 0; "sample": as get_action flies).  Every
slot flies the same --episodes missions from the same headings (evaluate.slot_scenarios).  Baselines at pass 0: the untrained
actors in both modes, and a uniform steer ~ U[-1, 1] per step flown through uavenv_step on a scratch env (the SAC kernel takes no
caller-supplied actions), and the scripted baseline among 9 steers with look-ahead 0 and 8.
    python scripts/learning_curve.py --config 3 [--passes 40000] [--every 4000] [--episodes 4096] [--out profiles/learning_curve_configs3.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dqn_based_uav_3d_path_planer_amd import evaluate as ev  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.data import make_city26_env  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.loop import HotLoop  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing  # noqa: E402

HELD_OUT_SEED = 0x4E1D_0C7                # the training bank is planned on seed 42 (+ rank): bench.py run_dqn


def bench_settings(*argv_extra):
    """bench.py's settings for the single-GPU DQN run (its argument parser: no arguments, or --config 3 for configs[2])."""
    sys.path.insert(0, ROOT)
    import bench
    argv, sys.argv = sys.argv, ["bench.py", *argv_extra]
    try:
        a = bench.parse()
    finally:
        sys.argv = argv
    return a


def evaluation(env, learner, scn, n, max_steps, eps=0.0):
    s = ev.evaluate_policy(env, learner, n, scenarios=scn, seed=11, eps=eps, max_steps=max_steps).summary()
    return {k: s[k] for k in ("episodes", "success", "lose", "truncated", "success_rate", "lose_rate", "mean_return",
                              "mean_steps", "mean_path_len", "mean_subgoals", "mean_collisions", "average_score")}


def scripted_baselines(env, scn, n, max_steps, U=1, v0=None, **kind):
    """The scripted baseline (evaluate.evaluate_scripted_policy: sub-goal pursuit, no learning) on the same held-out missions, as
    pure pursuit (look-ahead 0) and with look-ahead 8 -> {"scripted_h0": ..., "scripted_h8": ...}; U > 1: one summary per slot."""
    out = {}
    for H in (0, 8):
        rec = ev.evaluate_scripted_policy(env, n, scenarios=scn, v0=v0, seed=11, max_steps=max_steps, lookahead=H, **kind).host_records()
        summ = [{k: s[k] for k in KEYS} for s in (ev.summarize(rec[j::U]) for j in range(U))]
        out["scripted_h%d" % H] = summ if U > 1 else summ[0]
    return out


KEYS = ("episodes", "success", "lose", "truncated", "success_rate", "lose_rate", "mean_return", "mean_steps", "mean_path_len",
        "mean_subgoals", "mean_collisions", "average_score")


def config4_settings():
    """bench.py's settings for --config 4 (its argument parser)."""
    import bench
    argv, sys.argv = sys.argv, ["bench.py", "--config", "4"]
    try:
        a = bench.parse()
    finally:
        sys.argv = argv
    return a


def uniform_steer_baseline(velocities, scn_u, v0, U, max_steps, seed):
    """The same episodes under steer ~ U[-1, 1] per step: set_state + uavenv_step(SKIP_DONE) on a scratch APF env, accounted
    on the device -> one summary per slot."""
    import numpy as np
    from dqn_based_uav_3d_path_planer_amd import _lib
    sg, sub, ns = (x.cpu().numpy() for x in scn_u)
    n = len(sg)
    env = make_city26_env(n // U, obs_dtype="packed", uav_per_env=U, apf_enabled=1, velocities=velocities)
    kin = np.concatenate([sg[:, :3], v0.cpu().numpy(), sg[:, 3:]], 1)
    env.set_state(0, kin, np.zeros(n, np.int32), ns, sub, alias=(ns >= 2).astype(np.int32))
    d = env.device
    out = env.alloc_out()
    g = torch.Generator(device=d).manual_seed(seed)
    ret = torch.zeros(n, dtype=torch.float64, device=d)
    steps = torch.zeros(n, dtype=torch.int32, device=d)
    coll = torch.zeros(n, dtype=torch.int32, device=d)
    outcome = torch.zeros(n, dtype=torch.uint8, device=d)
    cap = torch.as_tensor(ns.astype(np.int64) * env.cfg.max_step + 1, device=d)
    if max_steps > 0:
        cap = torch.clamp(cap, max=max_steps)
    t = 0
    while True:
        a = torch.rand(n, device=d, generator=g, dtype=torch.float32) * 2 - 1
        env.step(a, out, skip_done=True)
        live = (out.valid == 1) & (outcome == 0)
        ret += torch.where(live, out.reward, torch.zeros_like(out.reward))
        steps += live.to(torch.int32)
        fin = live & (out.agent_done == 1)
        outcome[fin] = torch.where(out.info[fin] == _lib.INFO_LOSE, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS).to(torch.uint8)
        outcome[live & (outcome == 0) & (steps >= cap)] = _lib.EVAL_TRUNCATED
        t += 1
        if t % 16 == 0 and not bool((outcome == 0).any()):
            break
    st = env.get_state(0, n)
    rec = np.zeros(n, dtype=ev.RECORD_DTYPE)
    rec["ret"], rec["steps"], rec["outcome"] = ret.cpu().numpy(), steps.cpu().numpy(), outcome.cpu().numpy()
    rec["total_score"], rec["path_len"], rec["subgoals"] = st[:, 13], st[:, 14], ns - st[:, 11]
    env.close()
    res = []
    for j in range(U):
        s = ev.summarize(rec[j::U])
        res.append({k: s[k] for k in KEYS if k != "mean_collisions"})      # (collisions are not accounted on this path)
    return res


def main_config3(args):
    import numpy as np
    from dqn_based_uav_3d_path_planer_amd.loop import SACHotLoop
    from dqn_based_uav_3d_path_planer_amd.sac import FusedSACLearner
    b = config4_settings()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U, envs = 4, b.envs
    env = make_city26_env(envs, bank="gpu", bank_size=max(envs, 4096), bank_seed=42, device=dev, obs_dtype="packed",
                          uav_per_env=U, apf_enabled=1)
    vel = np.random.default_rng(42).uniform(-1.0, 1.0, (len(env.buildings), 3))
    vel[:, 2] = 0.0
    env.set_buildings(env.buildings, velocities=vel)
    ring = DeviceReplayRing(env, b.replay, discrete=False)
    ring.reset(seed=1000)
    a1_plane = torch.zeros((ring.frames, env.N), dtype=torch.float32, device=dev)
    ring.attach_action1(a1_plane)
    sac_param = {"actor": {"NetWork": "PolicyNetContinuous_SAC", "w": "100", "action_bound": "1", "hiden_dim": "64",
                           "output": "2", "lr": "0.0001"},
                 "critic": {"NetWork": "QValueNetContinuous_SAC", "w": "100", "hiden_dim": "64", "action_dim": "2", "lr": "0.001"},
                 "SAC_param": {"IS_Continuous": "1", "alpha_lr": "0.0001", "target_entropy": "1", "gamma": "0.99", "tau": "0.05"}}
    torch.manual_seed(42)
    learners = [FusedSACLearner(sac_param, device=dev) for _ in range(U)]
    loop = SACHotLoop(ring, learners, b.batch, seed=7, act1_plane=a1_plane, auto_reset=True, skip_done=True)
    scn = ev.held_out_scenarios(env, args.episodes, seed=HELD_OUT_SEED)
    scn_u, v0 = ev.slot_scenarios(scn, U, float(env.cfg.max_v), seed=11)

    def evaluation(mode):
        rec = ev.evaluate_sac_policy(env, learners, args.episodes * U, scenarios=scn_u, v0=v0, seed=11, mode=mode,
                                     max_steps=args.max_steps).host_records()
        return [{k: s[k] for k in KEYS} for s in (ev.summarize(rec[j::U]) for j in range(U))]

    out = {"what": "configs[3] training (bench.py --config 4: 4 UAV slots, APF on, fused SAC, SACHotLoop) with held-out evaluations of "
                   "the four actors in one launch; one summary per UAV slot",
           "settings": {"envs": envs, "uav_per_env": U, "batch": b.batch, "replay": b.replay, "passes": args.passes,
                        "every": args.every, "eval_episodes_per_slot": args.episodes, "eval_max_steps": args.max_steps,
                        "held_out_seed": HELD_OUT_SEED},
           "baselines": {"untrained_mean": evaluation("mean"), "untrained_sample": evaluation("sample"),
                         "uniform_steer": uniform_steer_baseline(vel, scn_u, v0, U, args.max_steps, seed=11)},
           "curve": []}
    out["baselines"].update(scripted_baselines(env, scn_u, args.episodes * U, args.max_steps, U=U, v0=v0, action="steer", candidates=9))
    print(json.dumps({"baselines": out["baselines"]}), flush=True)
    done, t0 = 0, time.perf_counter()
    while done < args.passes:
        k = min(args.every, args.passes - done)
        loop.run(k)
        done += k
        row = {"pass": done, "env_steps": done * envs * U, "updates": [int(L.epoch) for L in learners],
               "actor_loss": [float(L.loss) for L in learners], "mean": evaluation("mean"), "sample": evaluation("sample")}
        row["wall_s"] = round(time.perf_counter() - t0, 2)
        out["curve"].append(row)
        print(json.dumps(row), flush=True)
    loop.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1, choices=[1, 2, 3],
                    help="BASELINE configs[1] (DQN), configs[2] (dueling DDQN, f16 rows, f16 MFMA) or configs[3] (4 x SAC, APF)")
    ap.add_argument("--passes", type=int, default=None)
    ap.add_argument("--every", type=int, default=None)
    ap.add_argument("--episodes", type=int, default=None)
    ap.add_argument("--max-steps", type=int, default=0, help="evaluation truncation (0: natural episode ends)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--actions", type=int, default=3, help="--config 1: the size of the steering table (default 3: bench.py's run)")
    args = ap.parse_args()
    if args.actions != 3 and args.config != 1:
        raise SystemExit("--actions goes with --config 1 (the f16-MFMA learner of configs[2] takes at most 4 outputs, configs[3] is SAC)")
    c3 = args.config == 3
    args.passes = args.passes if args.passes is not None else (40000 if c3 else 1000000)
    args.every = args.every if args.every is not None else (4000 if c3 else 50000)
    args.episodes = args.episodes if args.episodes is not None else (4096 if c3 else 16384)
    args.out = args.out or "profiles/learning_curve_configs%d%s.json" % (args.config, "" if args.actions == 3 else "_a%d" % args.actions)
    if c3:
        return main_config3(args)
    c2 = args.config == 2
    b = bench_settings("--config", "3") if c2 else bench_settings()
    if c2 and (b.trainer != "dueling" or b.mfma != "f16" or b.obs_dtype != "f16"):
        raise SystemExit("bench.py --config 3 is expected to be the dueling f16-MFMA learner on f16 rows")
    if not c2 and (b.trainer not in ("dqn", "ddqn", "dueling") or b.mfma != "f32"):
        raise SystemExit("bench.py's default run is expected to be the f32 DQN family")
    A = args.actions
    if A < 2 or A + (1 if b.trainer == "dueling" else 0) > 14:
        raise SystemExit("--actions: 2 <= N, and N (+ 1 for a dueling trainer) <= 14 layer-2 outputs")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    bank_size = b.bank_size or max(b.envs, 4096)            # (bench.py run_dqn: the bank without rolling refresh)
    env = make_city26_env(b.envs, bank=b.bank, bank_size=bank_size, bank_seed=42, device=dev,
                          obs_dtype=torch.float16 if c2 else "packed", n_actions=A)
    ring = DeviceReplayRing(env, b.replay, discrete=True)
    ring.reset(seed=1000)
    torch.manual_seed(42)
    net = "VAnet2" if b.trainer == "dueling" else "Qnet2"
    learner = FusedDQNLearner({"NetWork": net, "w": "100", "hiden_dim": "64", "output": str(A)}, b.trainer, device=dev, mfma=b.mfma)
    loop = HotLoop(ring, learner, b.batch, 7, eps=b.eps)
    scn = ev.held_out_scenarios(env, args.episodes, seed=HELD_OUT_SEED)
    what = ("configs[2] training (bench.py --config 3: dueling DDQN, f16 rows, f16 MFMA) with greedy held-out evaluations of the "
            "f16 policy (uavenv_eval_episodes_f16)") if c2 else "configs[1] training (bench.py defaults) with greedy held-out evaluations"
    out = {"what": what, "settings": {
               "envs": b.envs, "batch": b.batch, "replay": b.replay, "trainer": b.trainer, "mfma": b.mfma, "obs_dtype": b.obs_dtype,
               "train_eps": b.eps, "bank": b.bank, "n_actions": A,
               "bank_size": bank_size, "passes": args.passes, "every": args.every, "eval_episodes": args.episodes,
               "eval_max_steps": args.max_steps, "held_out_seed": HELD_OUT_SEED},
           "baselines": {"untrained_greedy": evaluation(env, learner, scn, args.episodes, args.max_steps),
                         "random_eps1": evaluation(env, learner, scn, args.episodes, args.max_steps, eps=1.0)},
           "curve": []}
    out["baselines"].update(scripted_baselines(env, scn, args.episodes, args.max_steps, action="index"))
    print(json.dumps({"baselines": out["baselines"]}), flush=True)
    done, t0 = 0, time.perf_counter()
    while done < args.passes:
        k = min(args.every, args.passes - done)
        loop.run(k)
        done += k
        row = {"pass": done, "env_steps": done * b.envs, "updates": int(learner.epoch), "loss": float(learner.loss)}
        row.update(evaluation(env, learner, scn, args.episodes, args.max_steps))
        row["wall_s"] = round(time.perf_counter() - t0, 2)
        out["curve"].append(row)
        print(json.dumps(row), flush=True)
    loop.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
