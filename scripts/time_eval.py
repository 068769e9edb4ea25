"""Time greedy evaluation (uavenv_eval_episodes) against the composition of existing launches on the same episodes.

For n = 16 384, 65 536 and 262 144 held-out city26 episodes with an untrained Qnet2:
  eval   one uavenv_eval_episodes call;
  comp   set_state from the same rows and headings, then uavenv_step_policy (or uavenv_dqn_act + uavenv_step above 49 152
         agents) with eps = -1 (always greedy) and SKIP_DONE, once per step until every agent is done.
First the composition runs with its per-episode accounting on the device and every record must equal the kernel's; then both
are timed with device events, median of the repeats after a warm-up.  The composition's timed form issues exactly as many
steps as its longest episode took, and nothing else.
    python scripts/time_eval.py [--reps 5] [--out profiles/eval_times.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dqn_based_uav_3d_path_planer_amd import _lib  # noqa: E402
from dqn_based_uav_3d_path_planer_amd import evaluate as ev  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.data import make_city26_env  # noqa: E402
from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner  # noqa: E402

PARAM = {"NetWork": "Qnet2", "w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99",
         "Update_loop": "3"}
POLICY_MAX = 49152                   # uavenv_step_policy's one-launch limit (include/uavenv.h)


class Composition:
    def __init__(self, L, scn, n, v0):
        self.L, self.n = L, n
        sg, sub, ns = (x.cpu().numpy() for x in scn)
        rows = np.arange(n) % len(sg)
        self.env = make_city26_env(n, obs_dtype="packed")
        self.kin = np.concatenate([sg[rows, :3], v0, sg[rows, 3:]], 1)
        self.nsub = ns[rows]
        self.sub = sub[rows]
        d = self.env.device
        self.obs = [self.env.new_obs(), self.env.new_obs()]
        self.act = torch.zeros(n, dtype=torch.int32, device=d)
        self.r64 = torch.zeros(n, dtype=torch.float64, device=d)
        self.en = torch.zeros(n, dtype=torch.float64, device=d)
        self.info = torch.zeros(n, dtype=torch.uint8, device=d)
        self.adone = torch.zeros(n, dtype=torch.uint8, device=d)
        self.valid = torch.zeros(n, dtype=torch.uint8, device=d)

    def reset(self):
        self.env.set_state(0, self.kin, np.zeros(self.n, np.int32), self.nsub, self.sub, alias=(self.nsub >= 2).astype(np.int32))
        self.env.observe(self.obs[0])

    def step(self, t):
        e, o0, o1 = self.env, self.obs[t % 2], self.obs[(t + 1) % 2]
        if self.n <= POLICY_MAX:
            rc = e.lib.uavenv_step_policy(e._h, C.byref(self.L.net), o0.data_ptr(), -1.0, 5, t, self.act.data_ptr(), o1.data_ptr(),
                                          self.r64.data_ptr(), None, None, self.adone.data_ptr(), self.info.data_ptr(),
                                          self.valid.data_ptr(), self.en.data_ptr(), None, _lib.STEP_SKIP_DONE, e._stream())
            _lib.check(rc, "uavenv_step_policy")
        else:
            self.L.act(o0, -1.0, 5, t, index_out=self.act)
            _lib.check(e.lib.uavenv_step(e._h, self.act.data_ptr(), _lib.ACT_INDEX_I32, o1.data_ptr(), self.r64.data_ptr(), None,
                                         None, self.adone.data_ptr(), self.info.data_ptr(), self.valid.data_ptr(),
                                         self.en.data_ptr(), None, _lib.STEP_SKIP_DONE, e._stream()), "uavenv_step")

    def records(self):
        """Run to the end with the per-episode accounting on the device -> (records as the kernel writes them, steps issued)."""
        self.reset()
        n, d = self.n, self.env.device
        ret = torch.zeros(n, dtype=torch.float64, device=d)
        energy = torch.zeros(n, dtype=torch.float64, device=d)
        steps = torch.zeros(n, dtype=torch.int32, device=d)
        outcome = torch.zeros(n, dtype=torch.uint8, device=d)
        t = 0
        while True:
            self.step(t)
            live = (self.valid == 1) & (outcome == 0)
            ret += torch.where(live, self.r64, torch.zeros_like(self.r64))
            energy += torch.where(live, self.en, torch.zeros_like(self.en))
            steps += live.to(torch.int32)
            fin = live & (self.adone == 1)
            outcome[fin] = torch.where(self.info[fin] == _lib.INFO_LOSE, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS).to(torch.uint8)
            t += 1
            if t % 16 == 0 and not bool((outcome == 0).any()):
                break
        st = self.env.get_state(0, n)
        return dict(ret=ret.cpu().numpy(), energy=energy.cpu().numpy(), steps=steps.cpu().numpy(), outcome=outcome.cpu().numpy(),
                    total=st[:, 13], path_len=st[:, 14], reach=st[:, 15], subgoals=self.nsub - st[:, 11]), int(steps.max())

    def timed(self, n_steps):
        self.reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(n_steps):
            self.step(t)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,65536,262144")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/eval_times.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    L = FusedDQNLearner(PARAM, "dqn", device="cuda:0")
    probe = make_city26_env(64, obs_dtype="packed")
    scn = ev.held_out_scenarios(probe, 16384, seed=0xE7A1)
    out = {"what": "greedy evaluation of an untrained Qnet2 on held-out city26 episodes (median of %d after a warm-up, device events)" % args.reps,
           "sizes": []}
    for n in (int(x) for x in args.sizes.split(",")):
        v0 = np.random.default_rng(n).uniform(0, 2 * np.pi, n)
        v0 = np.stack([np.cos(v0), np.sin(v0)], 1)
        comp = Composition(L, scn, n, v0)
        ref, n_steps = comp.records()
        res = ev.evaluate_policy(probe, L, n, scenarios=scn, v0=v0)
        rec = res.host_records()
        ok = (np.array_equal(rec["ret"], ref["ret"]) and np.array_equal(rec["energy"], ref["energy"]) and
              np.array_equal(rec["steps"], ref["steps"]) and np.array_equal(rec["outcome"], ref["outcome"]) and
              np.array_equal(rec["total_score"], ref["total"]) and np.array_equal(rec["path_len"], ref["path_len"]) and
              np.array_equal(rec["subgoals"], ref["subgoals"]))
        if not ok:
            raise SystemExit(f"n = {n}: the kernel's records differ from the composition's; no time reported")
        agent_steps = int(rec["steps"].sum())
        t_eval = []
        for r in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            ev.evaluate_policy(probe, L, n, scenarios=scn, v0=v0)
            b.record()
            b.synchronize()
            if r:
                t_eval.append(a.elapsed_time(b))
        comp.timed(min(n_steps, 32))
        t_comp = [comp.timed(n_steps) for _ in range(args.reps)]
        me, mc = float(np.median(t_eval)), float(np.median(t_comp))
        row = {"episodes": n, "agent_steps": agent_steps, "steps_longest": n_steps, "records_equal": True,
               "eval_ms": me, "eval_ms_all": t_eval, "comp_ms": mc, "comp_ms_all": t_comp,
               "comp_form": "step_policy" if n <= POLICY_MAX else "dqn_act + step",
               "eval_agent_steps_per_s": agent_steps / (me * 1e-3), "comp_agent_steps_per_s": agent_steps / (mc * 1e-3),
               "eval_us_per_episode": me * 1e3 / n, "comp_us_per_episode": mc * 1e3 / n, "speedup": mc / me,
               "summary": res.summary()}
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all") and k != "summary"}), flush=True)
        out["sizes"].append(row)
        comp.env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
