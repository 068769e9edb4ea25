"""Does the fused training loop learn?  BASELINE configs[1] as bench.py runs it (HotLoop: C-enqueued act -> step -> learn, DQN,
packed replay ring), with a greedy evaluation of held-out city26 episodes (uavenv_eval_episodes) every --every passes.

The settings (envs, learner batch, replay capacity, trainer, training epsilon, reset bank) come from bench.py's own defaults
(bench.parse()), so this measures the loop the benchmark times.  Baselines at pass 0: the untrained net (greedy) and eps = 1 (the
uniform random policy).  Held-out rows are planned on a seed the training bank never uses.  Output: one JSON document.
    python scripts/learning_curve.py [--passes 1000000] [--every 50000] [--episodes 16384] [--out profiles/learning_curve_configs1.json]
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


def bench_settings():
    """bench.py's defaults for the single-GPU DQN run (its argument parser, no arguments)."""
    sys.path.insert(0, ROOT)
    import bench
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        a = bench.parse()
    finally:
        sys.argv = argv
    return a


def evaluation(env, learner, scn, n, max_steps, eps=0.0):
    s = ev.evaluate_policy(env, learner, n, scenarios=scn, seed=11, eps=eps, max_steps=max_steps).summary()
    return {k: s[k] for k in ("episodes", "success", "lose", "truncated", "success_rate", "lose_rate", "mean_return",
                              "mean_steps", "mean_path_len", "mean_subgoals", "mean_collisions", "average_score")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=1000000)
    ap.add_argument("--every", type=int, default=50000)
    ap.add_argument("--episodes", type=int, default=16384)
    ap.add_argument("--max-steps", type=int, default=0, help="evaluation truncation (0: natural episode ends)")
    ap.add_argument("--out", default="profiles/learning_curve_configs1.json")
    args = ap.parse_args()
    b = bench_settings()
    if b.trainer not in ("dqn", "ddqn", "dueling") or b.mfma != "f32":
        raise SystemExit("bench.py's default run is expected to be the f32 DQN family")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    bank_size = b.bank_size or max(b.envs, 4096)            # (bench.py run_dqn: the bank without rolling refresh)
    env = make_city26_env(b.envs, bank=b.bank, bank_size=bank_size, bank_seed=42, device=dev, obs_dtype="packed")
    ring = DeviceReplayRing(env, b.replay, discrete=True)
    ring.reset(seed=1000)
    torch.manual_seed(42)
    net = "VAnet2" if b.trainer == "dueling" else "Qnet2"
    learner = FusedDQNLearner({"NetWork": net, "w": "100", "hiden_dim": "64", "output": "3"}, b.trainer, device=dev)
    loop = HotLoop(ring, learner, b.batch, 7, eps=b.eps)
    scn = ev.held_out_scenarios(env, args.episodes, seed=HELD_OUT_SEED)
    out = {"what": "configs[1] training (bench.py defaults) with greedy held-out evaluations", "settings": {
               "envs": b.envs, "batch": b.batch, "replay": b.replay, "trainer": b.trainer, "train_eps": b.eps, "bank": b.bank,
               "bank_size": bank_size, "passes": args.passes, "every": args.every, "eval_episodes": args.episodes,
               "eval_max_steps": args.max_steps, "held_out_seed": HELD_OUT_SEED},
           "baselines": {"untrained_greedy": evaluation(env, learner, scn, args.episodes, args.max_steps),
                         "random_eps1": evaluation(env, learner, scn, args.episodes, args.max_steps, eps=1.0)},
           "curve": []}
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
