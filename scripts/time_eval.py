"""Time greedy evaluation (uavenv_eval_episodes) against the composition of existing launches on the same episodes.

For n = 16 384, 65 536 and 262 144 held-out city26 episodes with an untrained Qnet2:
  eval   one uavenv_eval_episodes call;
  comp   set_state from the same rows and headings, then uavenv_step_policy (or uavenv_dqn_act + uavenv_step above 49 152
         agents) with eps = -1 (always greedy) and SKIP_DONE, once per step until every agent is done.
First the composition runs with its per-episode accounting on the device and every record must equal the kernel's; then both
are timed with device events, median of the repeats after a warm-up.  The composition's timed form issues exactly as many
steps as its longest episode took, and nothing else.
    python scripts/time_eval.py [--reps 5] [--out profiles/eval_times.json]

--sac: the same for SAC policy evaluation (uavenv_eval_episodes_sac; four untrained actors, one per UAV slot, mean mode) with APF
off and on, against set_state + per step uavenv_sac_act_multi (one launch for the four slots, zero noise) + uavenv_step with
SKIP_DONE in its default form (k_apf_adjust + k_step on the APF env).  Launches only, device events, a warm-up of both forms, then
the two forms alternating in the same process, median of the repeats; every record checked equal before a time is taken.
    python scripts/time_eval.py --sac [--reps 5] [--max-steps 600] [--out profiles/eval_sac_times.json]

--slots: greedy DQN evaluation with one net per UAV slot (uavenv_eval_episodes_slots; four untrained Qnet2, U = 4), APF off and on,
against what had to be done for the same records before that entry existed.  APF off: four uavenv_eval_episodes calls, one per net,
each on all n episodes (every fourth record of each is kept).  APF on: set_state + per step four uavenv_dqn_act launches, each on its
slot's rows (gathered to a contiguous block, the actions scattered back) + uavenv_step with SKIP_DONE in its default form
(k_apf_adjust + k_step).  Launches only, device events, a warm-up of both forms, then the two forms alternating in the same process,
median of the repeats; every record checked equal before a time is taken.
    python scripts/time_eval.py --slots [--reps 5] [--max-steps 600] [--out profiles/eval_slots_times.json]

--f16: greedy evaluation of an f16-MFMA net (uavenv_eval_episodes_f16; an untrained dueling VAnet2, BASELINE configs[2]'s shape) on
an f16 env and on a packed env, against set_state + per step uavenv_dqn_act (the env's obs_dtype, eps = -1) + uavenv_step with
SKIP_DONE; on the f16 env, where uavenv_step_policy takes the shape (at most 65 536 agents, its one-wavefront form), that one launch
per step is timed as well.  Launches only, device events, a warm-up of every form, then the forms alternating in the same process,
median of the repeats; every record checked equal before a time is taken.
    python scripts/time_eval.py --f16 [--reps 5] [--max-steps 600] [--out profiles/eval_f16_times.json]

--scripted: the scripted baseline (uavenv_eval_episodes_scripted; the index kind on the env's 3 actions, look-ahead 8, U = 4), APF off
and on, against set_state + per step uavenv_scripted_act + uavenv_step with SKIP_DONE and no observation (nothing reads one) in its
default form (k_apf_adjust + k_step on the APF env).  Launches only, device events, a warm-up of both forms, then the two forms
alternating in the same process, median of the repeats; every record checked equal before a time is taken.  --once N: no timing, one
launch per APF setting at N episodes (for a kernel-trace run).
    python scripts/time_eval.py --scripted [--reps 5] [--max-steps 600] [--lookahead 8] [--out profiles/eval_scripted_times.json]

--wide: heads of more than 4 layer-2 outputs (a 9-action Qnet2; a 13-action dueling VAnet2 = 14 outputs) through the wide
instantiations of k_eval_episodes / k_eval_episodes_slots: one net on a non-APF env, four nets (U = 4) with APF off and on, each against
set_state + per step one uavenv_dqn_act per net (eps = -1; four nets: slot rows gathered, actions scattered) + uavenv_step with
SKIP_DONE.  Launches only, device events, a warm-up of both forms, then the two forms alternating in the same process, median of the
repeats; every record checked equal before a time is taken.
    python scripts/time_eval.py --wide [--reps 5] [--max-steps 600] [--out profiles/eval_wide_times.json]
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


class F16Composition(Composition):
    """Composition for an f16-MFMA net on an env of f16 or packed rows: uavenv_dqn_act + uavenv_step per step, or (policy = True, f16
    rows, <= 65 536 agents) uavenv_step_policy in its one-wavefront form."""

    def __init__(self, L, scn, n, v0, obs, max_steps):
        self.L, self.n, self.max_steps, self.policy = L, n, max_steps, False
        sg, sub, ns = (x.cpu().numpy() for x in scn)
        rows = np.arange(n) % len(sg)
        self.env = make_city26_env(n, obs_dtype=torch.float16 if obs == "f16" else "packed")
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

    def step(self, t):
        e, o0, o1 = self.env, self.obs[t % 2], self.obs[(t + 1) % 2]
        if self.policy:
            flags = _lib.STEP_SKIP_DONE | (_lib.STEP_ONE_WAVE if self.n <= POLICY_MAX else 0)
            rc = e.lib.uavenv_step_policy(e._h, C.byref(self.L.net), o0.data_ptr(), -1.0, 5, t, self.act.data_ptr(), o1.data_ptr(),
                                          self.r64.data_ptr(), None, None, self.adone.data_ptr(), self.info.data_ptr(),
                                          self.valid.data_ptr(), self.en.data_ptr(), None, flags, e._stream())
            _lib.check(rc, "uavenv_step_policy")
        else:
            self.L.act(o0, -1.0, 5, t, index_out=self.act)
            _lib.check(e.lib.uavenv_step(e._h, self.act.data_ptr(), _lib.ACT_INDEX_I32, o1.data_ptr(), self.r64.data_ptr(), None,
                                         None, self.adone.data_ptr(), self.info.data_ptr(), self.valid.data_ptr(),
                                         self.en.data_ptr(), None, _lib.STEP_SKIP_DONE, e._stream()), "uavenv_step")

    def records(self):
        """Composition.records with the truncation at max_steps / the natural bound."""
        self.reset()
        n, d = self.n, self.env.device
        ret = torch.zeros(n, dtype=torch.float64, device=d)
        energy = torch.zeros(n, dtype=torch.float64, device=d)
        steps = torch.zeros(n, dtype=torch.int32, device=d)
        outcome = torch.zeros(n, dtype=torch.uint8, device=d)
        cap = torch.as_tensor(self.nsub.astype(np.int64) * self.env.cfg.max_step + 1, device=d)
        if self.max_steps > 0:
            cap = torch.clamp(cap, max=self.max_steps)
        t = 0
        while True:
            self.step(t)
            live = (self.valid == 1) & (outcome == 0)
            ret += torch.where(live, self.r64, torch.zeros_like(self.r64))
            energy += torch.where(live, self.en, torch.zeros_like(self.en))
            steps += live.to(torch.int32)
            fin = live & (self.adone == 1)
            outcome[fin] = torch.where(self.info[fin] == _lib.INFO_LOSE, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS).to(torch.uint8)
            outcome[live & (outcome == 0) & (steps >= cap)] = _lib.EVAL_TRUNCATED
            t += 1
            if t % 16 == 0 and not bool((outcome == 0).any()):
                break
        return dict(ret=ret.cpu().numpy(), energy=energy.cpu().numpy(), steps=steps.cpu().numpy(), outcome=outcome.cpu().numpy()), \
            int(steps.max())


def main_f16(args):
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    L = FusedDQNLearner(dict(PARAM, NetWork="VAnet2"), "dueling", device="cuda:0", mfma="f16")
    probe = make_city26_env(64, obs_dtype="packed")
    scn = ev.held_out_scenarios(probe, 16384, seed=0xE7A1)
    probe.close()
    out = {"what": "greedy evaluation of an untrained f16-MFMA dueling VAnet2 in one launch (uavenv_eval_episodes_f16) on held-out city26 "
                   "episodes against uavenv_dqn_act + uavenv_step per step on an env of the same rows, and on f16 rows up to 65 536 agents "
                   "against uavenv_step_policy per step.  Launches only, device events, a warm-up, the forms alternating, median of %d"
                   % args.reps,
           "max_steps": args.max_steps, "sizes": []}

    def same(rec, ref):
        return (np.array_equal(rec["ret"], ref["ret"]) and np.array_equal(rec["energy"], ref["energy"]) and
                np.array_equal(rec["steps"], ref["steps"]) and np.array_equal(rec["outcome"], ref["outcome"]))

    for obs in ("f16", "packed"):
        for n in (int(x) for x in args.sizes.split(",")):
            v0 = np.random.default_rng(n).uniform(0, 2 * np.pi, n)
            v0 = np.stack([np.cos(v0), np.sin(v0)], 1)
            comp = F16Composition(L, scn, n, v0, obs, args.max_steps)
            kw = dict(scenarios=scn, v0=v0, max_steps=args.max_steps)
            res = ev.evaluate_policy(comp.env, L, n, **kw)
            rec = res.host_records()
            ref, n_steps = comp.records()
            with_policy = obs == "f16" and n <= 65536 and n % 2 == 0
            if with_policy:
                comp.policy = True
                try:
                    ref_p, n_steps_p = comp.records()
                except _lib.UavEnvError:             # uavenv_step_policy does not take this shape (EINVAL, nothing enqueued)
                    with_policy = False
                comp.policy = False
            if not same(rec, ref) or (with_policy and not (same(rec, ref_p) and n_steps_p == n_steps)):
                raise SystemExit(f"{obs} rows, n = {n}: the kernel's records differ from the composition's; no time reported")
            agent_steps = int(rec["steps"].sum())

            def timed_eval():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                ev.evaluate_policy(comp.env, L, n, **kw)
                b.record()
                b.synchronize()
                return a.elapsed_time(b)

            def timed_comp(policy, steps):
                comp.policy = policy
                return comp.timed(steps)

            timed_eval()
            timed_comp(False, min(n_steps, 32))
            if with_policy:
                timed_comp(True, min(n_steps, 32))
            t_eval, t_comp, t_pol = [], [], []
            for _ in range(args.reps):               # the forms alternating
                t_eval.append(timed_eval())
                t_comp.append(timed_comp(False, n_steps))
                if with_policy:
                    t_pol.append(timed_comp(True, n_steps))
            me, mc = float(np.median(t_eval)), float(np.median(t_comp))
            row = {"obs": obs, "episodes": n, "agent_steps": agent_steps, "steps_longest": n_steps, "records_equal": True,
                   "eval_ms": me, "eval_ms_all": t_eval, "comp_ms": mc, "comp_ms_all": t_comp, "comp_form": "dqn_act + step",
                   "eval_agent_steps_per_s": agent_steps / (me * 1e-3), "comp_agent_steps_per_s": agent_steps / (mc * 1e-3),
                   "eval_us_per_episode": me * 1e3 / n, "comp_us_per_episode": mc * 1e3 / n, "speedup": mc / me}
            if with_policy:
                mp = float(np.median(t_pol))
                row.update({"step_policy_ms": mp, "step_policy_ms_all": t_pol, "speedup_vs_step_policy": mp / me})
            row["summary"] = res.summary()
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all") and k != "summary"}), flush=True)
            out["sizes"].append(row)
            comp.env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


SAC_PARAM = {"actor": {"NetWork": "PolicyNetContinuous_SAC", "w": "100", "action_bound": "1", "hiden_dim": "64", "output": "2",
                       "lr": "0.0001"},
             "critic": {"NetWork": "QValueNetContinuous_SAC", "w": "100", "hiden_dim": "64", "action_dim": "2", "lr": "0.001"},
             "SAC_param": {"IS_Continuous": "1", "alpha_lr": "0.0001", "target_entropy": "1", "gamma": "0.99", "tau": "0.05"}}


def apf_velocities(nb):
    """bench.py run_config4's moving cylinders (default_rng(42)), every third one static as in tests/golden/apf_episodes.npz"""
    v = np.random.default_rng(42).uniform(-1.0, 1.0, (nb, 3))
    v[:, 2] = 0.0
    v[::3] = 0.0
    return v


class SacComposition:
    """n agents of a fresh env (uav_per_env = U) = the n episodes; agent i is UAV slot i mod U, acted for by learner i mod U."""

    def __init__(self, Ls, scn, n, v0, apf, max_steps):
        U = len(Ls)
        self.Ls, self.n, self.U, self.max_steps = Ls, n, U, max_steps
        sg, sub, ns = (x.cpu().numpy() for x in scn)
        rows = np.arange(n) % len(sg)
        self.env = make_city26_env(n // U, obs_dtype="packed", uav_per_env=U, apf_enabled=apf)
        if apf:
            self.env.set_buildings(self.env.buildings, velocities=apf_velocities(len(self.env.buildings)))
        self.kin = np.concatenate([sg[rows, :3], v0, sg[rows, 3:]], 1)
        self.nsub = ns[rows]
        self.sub = sub[rows]
        d = self.env.device
        self.obs = [self.env.new_obs(), self.env.new_obs()]
        self.act0 = torch.zeros(n, dtype=torch.float32, device=d)
        self.act1 = torch.zeros(n, dtype=torch.float32, device=d)
        self.zero = torch.zeros((n // U, 2), dtype=torch.float32, device=d)
        self.r64 = torch.zeros(n, dtype=torch.float64, device=d)
        self.en = torch.zeros(n, dtype=torch.float64, device=d)
        self.info = torch.zeros(n, dtype=torch.uint8, device=d)
        self.adone = torch.zeros(n, dtype=torch.uint8, device=d)
        self.valid = torch.zeros(n, dtype=torch.uint8, device=d)
        self.actors = (C.c_void_p * U)(*[L._blocks[0].data_ptr() for L in Ls])
        self.eps = (C.c_void_p * U)(*[self.zero.data_ptr()] * U)
        self.first = (C.c_int32 * U)(*range(U))
        self.act_multi = self.env.lib.uavenv_sac_act_multi
        self.act_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p,
                                   C.c_void_p, C.c_int32, C.c_void_p]

    def reset(self):
        self.env.set_state(0, self.kin, np.zeros(self.n, np.int32), self.nsub, self.sub, alias=(self.nsub >= 2).astype(np.int32))
        self.env.observe(self.obs[0])

    def step(self, t):
        e, o0, o1 = self.env, self.obs[t % 2], self.obs[(t + 1) % 2]
        rc = self.act_multi(self.actors, o0.data_ptr(), self.first, self.U, self.n // self.U, self.eps, float(self.Ls[0].action_bound),
                            self.act0.data_ptr(), self.act1.data_ptr(), self.U, e._stream())
        if rc != 0:
            raise RuntimeError(f"uavenv_sac_act_multi: {rc}")
        _lib.check(e.lib.uavenv_step(e._h, self.act0.data_ptr(), _lib.ACT_STEER_F32, o1.data_ptr(), self.r64.data_ptr(), None,
                                     None, self.adone.data_ptr(), self.info.data_ptr(), self.valid.data_ptr(),
                                     self.en.data_ptr(), None, _lib.STEP_SKIP_DONE, e._stream()), "uavenv_step")

    def records(self):
        """Run to the end with the per-episode accounting on the device -> (what the kernel's records must hold, steps issued)."""
        self.reset()
        n, d = self.n, self.env.device
        ret = torch.zeros(n, dtype=torch.float64, device=d)
        energy = torch.zeros(n, dtype=torch.float64, device=d)
        steps = torch.zeros(n, dtype=torch.int32, device=d)
        outcome = torch.zeros(n, dtype=torch.uint8, device=d)
        total = torch.zeros(n, dtype=torch.float64, device=d)
        cap = torch.as_tensor(self.nsub.astype(np.int64) * self.env.cfg.max_step + 1, device=d)
        if self.max_steps > 0:
            cap = torch.clamp(cap, max=self.max_steps)
        t = 0
        while True:
            self.step(t)
            live = (self.valid == 1) & (outcome == 0)
            ret += torch.where(live, self.r64, torch.zeros_like(self.r64))
            energy += torch.where(live, self.en, torch.zeros_like(self.en))
            steps += live.to(torch.int32)
            fin = live & (self.adone == 1)
            outcome[fin] = torch.where(self.info[fin] == _lib.INFO_LOSE, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS).to(torch.uint8)
            outcome[live & (outcome == 0) & (steps >= cap)] = _lib.EVAL_TRUNCATED
            t += 1
            if t % 16 == 0 and not bool((outcome == 0).any()):
                break
        return dict(ret=ret.cpu().numpy(), energy=energy.cpu().numpy(), steps=steps.cpu().numpy(), outcome=outcome.cpu().numpy()), \
            int(steps.max())

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


def main_sac(args):
    from dqn_based_uav_3d_path_planer_amd.sac import FusedSACLearner
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    U = 4
    Ls = [FusedSACLearner(SAC_PARAM, "cuda:0") for _ in range(U)]
    probe = make_city26_env(64, obs_dtype="packed")
    scn = ev.held_out_scenarios(probe, 16384, seed=0xE7A1)
    probe.close()
    out = {"what": "SAC policy evaluation (mean mode) of four untrained actors, one per UAV slot, on held-out city26 episodes against "
                   "uavenv_sac_act_multi + uavenv_step (k_apf_adjust + k_step with APF on); launches only, device events, a warm-up, "
                   "the two forms alternating, median of %d" % args.reps,
           "max_steps": args.max_steps, "sizes": []}
    for apf in (0, 1):
        for n in (int(x) for x in args.sizes.split(",")):
            v0 = np.random.default_rng(n).uniform(0, 2 * np.pi, n)
            v0 = np.stack([np.cos(v0), np.sin(v0)], 1)
            comp = SacComposition(Ls, scn, n, v0, apf, args.max_steps)
            ref, n_steps = comp.records()
            kw = dict(scenarios=scn, v0=v0, mode="mean", max_steps=args.max_steps)
            res = ev.evaluate_sac_policy(comp.env, Ls, n, **kw)
            rec = res.host_records()
            ok = (np.array_equal(rec["ret"], ref["ret"]) and np.array_equal(rec["energy"], ref["energy"]) and
                  np.array_equal(rec["steps"], ref["steps"]) and np.array_equal(rec["outcome"], ref["outcome"]))
            if not ok:
                raise SystemExit(f"apf {apf}, n = {n}: the kernel's records differ from the composition's; no time reported")
            agent_steps = int(rec["steps"].sum())

            def timed_eval():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                ev.evaluate_sac_policy(comp.env, Ls, n, **kw)
                b.record()
                b.synchronize()
                return a.elapsed_time(b)

            timed_eval()
            comp.timed(min(n_steps, 32))
            t_eval, t_comp = [], []
            for _ in range(args.reps):               # the two forms alternating
                t_eval.append(timed_eval())
                t_comp.append(comp.timed(n_steps))
            me, mc = float(np.median(t_eval)), float(np.median(t_comp))
            row = {"apf": apf, "episodes": n, "agent_steps": agent_steps, "steps_longest": n_steps, "records_equal": True,
                   "eval_ms": me, "eval_ms_all": t_eval, "comp_ms": mc, "comp_ms_all": t_comp,
                   "comp_form": "sac_act_multi + " + ("apf_adjust + step" if apf else "step"),
                   "eval_agent_steps_per_s": agent_steps / (me * 1e-3), "comp_agent_steps_per_s": agent_steps / (mc * 1e-3),
                   "eval_us_per_episode": me * 1e3 / n, "comp_us_per_episode": mc * 1e3 / n, "speedup": mc / me,
                   "summary": res.summary()}
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all") and k != "summary"}), flush=True)
            out["sizes"].append(row)
            comp.env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


class SlotsComposition(SacComposition):
    """SacComposition with DQN nets: per step one uavenv_dqn_act per UAV slot on that slot's rows, then uavenv_step."""

    def __init__(self, Ls, scn, n, v0, apf, max_steps):
        U = len(Ls)
        self.Ls, self.n, self.U, self.max_steps = Ls, n, U, max_steps
        sg, sub, ns = (x.cpu().numpy() for x in scn)
        rows = np.arange(n) % len(sg)
        self.env = make_city26_env(n // U, obs_dtype="packed", uav_per_env=U, apf_enabled=apf)
        if apf:
            self.env.set_buildings(self.env.buildings, velocities=apf_velocities(len(self.env.buildings)))
        self.kin = np.concatenate([sg[rows, :3], v0, sg[rows, 3:]], 1)
        self.nsub = ns[rows]
        self.sub = sub[rows]
        d = self.env.device
        self.obs = [self.env.new_obs(), self.env.new_obs()]
        self.act = torch.zeros(n, dtype=torch.int32, device=d)
        self.rows_j = torch.zeros((n // U, self.obs[0].shape[1]), dtype=self.obs[0].dtype, device=d)
        self.act_j = torch.zeros(n // U, dtype=torch.int32, device=d)
        self.r64 = torch.zeros(n, dtype=torch.float64, device=d)
        self.en = torch.zeros(n, dtype=torch.float64, device=d)
        self.info = torch.zeros(n, dtype=torch.uint8, device=d)
        self.adone = torch.zeros(n, dtype=torch.uint8, device=d)
        self.valid = torch.zeros(n, dtype=torch.uint8, device=d)

    def step(self, t):
        e, o0, o1 = self.env, self.obs[t % 2], self.obs[(t + 1) % 2]
        for j, L in enumerate(self.Ls):
            self.rows_j.copy_(o0[j::self.U])
            L.act(self.rows_j, -1.0, 5, t, index_out=self.act_j)
            self.act[j::self.U] = self.act_j
        _lib.check(e.lib.uavenv_step(e._h, self.act.data_ptr(), _lib.ACT_INDEX_I32, o1.data_ptr(), self.r64.data_ptr(), None,
                                     None, self.adone.data_ptr(), self.info.data_ptr(), self.valid.data_ptr(),
                                     self.en.data_ptr(), None, _lib.STEP_SKIP_DONE, e._stream()), "uavenv_step")


def main_slots(args):
    torch.cuda.set_device(0)
    U = 4
    Ls = []
    for j in range(U):
        torch.manual_seed(j)
        Ls.append(FusedDQNLearner(PARAM, "dqn", device="cuda:0"))
    probe = make_city26_env(64, obs_dtype="packed")
    scn = ev.held_out_scenarios(probe, 16384, seed=0xE7A1)
    probe.close()
    out = {"what": "greedy evaluation of four untrained Qnet2, one per UAV slot, in one launch (uavenv_eval_episodes_slots) on held-out "
                   "city26 episodes against what gave the same records before: APF off, four uavenv_eval_episodes calls on all the "
                   "episodes; APF on, per step four uavenv_dqn_act (slot rows gathered, actions scattered) + uavenv_step (k_apf_adjust + "
                   "k_step).  Launches only, device events, a warm-up, the two forms alternating, median of %d" % args.reps,
           "max_steps": args.max_steps, "sizes": []}
    for apf in (0, 1):
        for n in (int(x) for x in args.sizes.split(",")):
            v0 = np.random.default_rng(n).uniform(0, 2 * np.pi, n)
            v0 = np.stack([np.cos(v0), np.sin(v0)], 1)
            kw = dict(scenarios=scn, v0=v0, max_steps=args.max_steps)
            if apf:
                comp = SlotsComposition(Ls, scn, n, v0, apf, args.max_steps)
                env = comp.env
                ref, n_steps = comp.records()
            else:
                comp, n_steps = None, 0
                env = make_city26_env(64, obs_dtype="packed", uav_per_env=U)
            res = ev.evaluate_policy(env, Ls, n, **kw)
            rec = res.host_records()
            if apf:
                ok = (np.array_equal(rec["ret"], ref["ret"]) and np.array_equal(rec["energy"], ref["energy"]) and
                      np.array_equal(rec["steps"], ref["steps"]) and np.array_equal(rec["outcome"], ref["outcome"]))
                parent_steps = agent_steps = int(rec["steps"].sum())
            else:
                olds = [ev.evaluate_policy(env, Ls[j], n, **kw).host_records() for j in range(U)]
                ok = all(olds[j][j::U].tobytes() == rec[j::U].tobytes() for j in range(U))
                parent_steps = int(sum(int(o["steps"].sum()) for o in olds))
            if not ok:
                raise SystemExit(f"apf {apf}, n = {n}: the one-launch records differ from the parent form's; no time reported")
            agent_steps = int(rec["steps"].sum())

            def timed(fn):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                b.synchronize()
                return a.elapsed_time(b)

            def one_launch():
                ev.evaluate_policy(env, Ls, n, **kw)

            def four_calls():
                for L in Ls:
                    ev.evaluate_policy(env, L, n, **kw)

            timed(one_launch)
            if apf:
                comp.timed(min(n_steps, 32))
            else:
                timed(four_calls)
            t_eval, t_comp = [], []
            for _ in range(args.reps):               # the two forms alternating
                t_eval.append(timed(one_launch))
                t_comp.append(comp.timed(n_steps) if apf else timed(four_calls))
            me, mc = float(np.median(t_eval)), float(np.median(t_comp))
            row = {"apf": apf, "nets": U, "episodes": n, "agent_steps": agent_steps, "steps_longest": n_steps, "records_equal": True,
                   "eval_ms": me, "eval_ms_all": t_eval, "comp_ms": mc, "comp_ms_all": t_comp,
                   "comp_form": "4 x (gather + dqn_act + scatter) + apf_adjust + step" if apf else "4 x uavenv_eval_episodes on all episodes",
                   "comp_agent_steps": parent_steps,
                   "eval_agent_steps_per_s": agent_steps / (me * 1e-3), "eval_us_per_episode": me * 1e3 / n,
                   "comp_us_per_episode": mc * 1e3 / n, "speedup": mc / me, "summary": res.summary()}
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all") and k != "summary"}), flush=True)
            out["sizes"].append(row)
            env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


class ScriptedComposition(SacComposition):
    """SacComposition with the scripted baseline's act launch in the actors' place; the step launch writes no observation."""

    def __init__(self, scn, n, v0, apf, max_steps, lookahead, U=4):
        self.n, self.U, self.max_steps = n, U, max_steps
        sg, sub, ns = (x.cpu().numpy() for x in scn)
        rows = np.arange(n) % len(sg)
        self.env = make_city26_env(n // U, obs_dtype="packed", uav_per_env=U, apf_enabled=apf)
        if apf:
            self.env.set_buildings(self.env.buildings, velocities=apf_velocities(len(self.env.buildings)))
        self.kin = np.concatenate([sg[rows, :3], v0, sg[rows, 3:]], 1)
        self.nsub = ns[rows]
        self.sub = sub[rows]
        d = self.env.device
        self.act = torch.zeros(n, dtype=torch.int32, device=d)
        self.r64 = torch.zeros(n, dtype=torch.float64, device=d)
        self.en = torch.zeros(n, dtype=torch.float64, device=d)
        self.info = torch.zeros(n, dtype=torch.uint8, device=d)
        self.adone = torch.zeros(n, dtype=torch.uint8, device=d)
        self.valid = torch.zeros(n, dtype=torch.uint8, device=d)
        self.pol = ev._scripted_policy(self.env, "index", None, lookahead)

    def reset(self):
        self.env.set_state(0, self.kin, np.zeros(self.n, np.int32), self.nsub, self.sub, alias=(self.nsub >= 2).astype(np.int32))

    def step(self, t):
        e = self.env
        _lib.check(e.lib.uavenv_scripted_act(e._h, C.byref(self.pol), self.act.data_ptr(), e._stream()), "uavenv_scripted_act")
        _lib.check(e.lib.uavenv_step(e._h, self.act.data_ptr(), _lib.ACT_INDEX_I32, None, self.r64.data_ptr(), None,
                                     None, self.adone.data_ptr(), self.info.data_ptr(), self.valid.data_ptr(),
                                     self.en.data_ptr(), None, _lib.STEP_SKIP_DONE | _lib.STEP_NO_OBS, e._stream()), "uavenv_step")


def scripted_v0(n):
    t = np.random.default_rng(n).uniform(0, 2 * np.pi, n)
    return np.stack([np.cos(t), np.sin(t)], 1)


def main_scripted(args):
    torch.cuda.set_device(0)
    probe = make_city26_env(64, obs_dtype="packed")
    scn = ev.held_out_scenarios(probe, 16384, seed=0xE7A1)
    probe.close()
    U, H = 4, args.lookahead
    if args.once > 0:                                # one launch per APF setting (for a kernel-trace run)
        for apf in (0, 1):
            env = make_city26_env(64, obs_dtype="packed", uav_per_env=U, apf_enabled=apf)
            if apf:
                env.set_buildings(env.buildings, velocities=apf_velocities(len(env.buildings)))
            s = ev.evaluate_scripted_policy(env, args.once, scenarios=scn, v0=scripted_v0(args.once), lookahead=H,
                                            max_steps=args.max_steps).summary()
            print(json.dumps({"apf": apf, "episodes": args.once, "mean_steps": s["mean_steps"]}), flush=True)
            env.close()
        return
    out = {"what": "the scripted baseline (index kind, 3 actions, look-ahead %d, U = 4) on held-out city26 episodes in one launch "
                   "(uavenv_eval_episodes_scripted) against uavenv_scripted_act + uavenv_step without observations (k_apf_adjust + k_step "
                   "with APF on); launches only, device events, a warm-up, the two forms alternating, median of %d" % (H, args.reps),
           "max_steps": args.max_steps, "lookahead": H, "sizes": []}
    for apf in (0, 1):
        for n in (int(x) for x in args.sizes.split(",")):
            v0 = scripted_v0(n)
            comp = ScriptedComposition(scn, n, v0, apf, args.max_steps, H, U)
            ref, n_steps = comp.records()
            kw = dict(scenarios=scn, v0=v0, lookahead=H, max_steps=args.max_steps)
            res = ev.evaluate_scripted_policy(comp.env, n, **kw)
            rec = res.host_records()
            ok = (np.array_equal(rec["ret"], ref["ret"]) and np.array_equal(rec["energy"], ref["energy"]) and
                  np.array_equal(rec["steps"], ref["steps"]) and np.array_equal(rec["outcome"], ref["outcome"]))
            if not ok:
                raise SystemExit(f"apf {apf}, n = {n}: the kernel's records differ from the composition's; no time reported")
            agent_steps = int(rec["steps"].sum())

            def timed_eval():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                ev.evaluate_scripted_policy(comp.env, n, **kw)
                b.record()
                b.synchronize()
                return a.elapsed_time(b)

            timed_eval()
            comp.timed(min(n_steps, 32))
            t_eval, t_comp = [], []
            for _ in range(args.reps):               # the two forms alternating
                t_eval.append(timed_eval())
                t_comp.append(comp.timed(n_steps))
            me, mc = float(np.median(t_eval)), float(np.median(t_comp))
            row = {"apf": apf, "episodes": n, "agent_steps": agent_steps, "steps_longest": n_steps, "records_equal": True,
                   "eval_ms": me, "eval_ms_all": t_eval, "comp_ms": mc, "comp_ms_all": t_comp,
                   "comp_form": "scripted_act + " + ("apf_adjust + step" if apf else "step") + " (no observation)",
                   "eval_agent_steps_per_s": agent_steps / (me * 1e-3), "comp_agent_steps_per_s": agent_steps / (mc * 1e-3),
                   "eval_us_per_episode": me * 1e3 / n, "comp_us_per_episode": mc * 1e3 / n, "speedup": mc / me,
                   "summary": res.summary()}
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all") and k != "summary"}), flush=True)
            out["sizes"].append(row)
            comp.env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def main_slots_once(args):
    """One uavenv_eval_episodes_slots launch per APF setting at `--once` episodes per net (for a kernel-trace run)."""
    torch.cuda.set_device(0)
    U = 4
    Ls = []
    for j in range(U):
        torch.manual_seed(j)
        Ls.append(FusedDQNLearner(PARAM, "dqn", device="cuda:0"))
    n = args.once * U
    probe = make_city26_env(64, obs_dtype="packed")
    scn = ev.held_out_scenarios(probe, 16384, seed=0xE7A1)
    probe.close()
    for apf in (0, 1):
        env = make_city26_env(64, obs_dtype="packed", uav_per_env=U, apf_enabled=apf)
        if apf:
            env.set_buildings(env.buildings, velocities=apf_velocities(len(env.buildings)))
        v0 = np.random.default_rng(n).uniform(0, 2 * np.pi, n)
        v0 = np.stack([np.cos(v0), np.sin(v0)], 1)
        s = ev.evaluate_policy(env, Ls, n, scenarios=scn, v0=v0, max_steps=args.max_steps).summary()
        print(json.dumps({"apf": apf, "episodes": n, "mean_steps": s["mean_steps"]}), flush=True)
        env.close()


class WideComposition(SlotsComposition):
    """SlotsComposition on an env of A actions (nets of more than 4 layer-2 outputs); U = len(Ls) may be 1."""

    def __init__(self, Ls, scn, n, v0, apf, max_steps, A):
        U = len(Ls)
        self.Ls, self.n, self.U, self.max_steps = Ls, n, U, max_steps
        sg, sub, ns = (x.cpu().numpy() for x in scn)
        rows = np.arange(n) % len(sg)
        self.env = make_city26_env(n // U, obs_dtype="packed", uav_per_env=U, apf_enabled=apf, n_actions=A)
        if apf:
            self.env.set_buildings(self.env.buildings, velocities=apf_velocities(len(self.env.buildings)))
        self.kin = np.concatenate([sg[rows, :3], v0, sg[rows, 3:]], 1)
        self.nsub = ns[rows]
        self.sub = sub[rows]
        d = self.env.device
        self.obs = [self.env.new_obs(), self.env.new_obs()]
        self.act = torch.zeros(n, dtype=torch.int32, device=d)
        self.rows_j = torch.zeros((n // U, self.obs[0].shape[1]), dtype=self.obs[0].dtype, device=d)
        self.act_j = torch.zeros(n // U, dtype=torch.int32, device=d)
        self.r64 = torch.zeros(n, dtype=torch.float64, device=d)
        self.en = torch.zeros(n, dtype=torch.float64, device=d)
        self.info = torch.zeros(n, dtype=torch.uint8, device=d)
        self.adone = torch.zeros(n, dtype=torch.uint8, device=d)
        self.valid = torch.zeros(n, dtype=torch.uint8, device=d)

    def step(self, t):
        if self.U > 1:
            return SlotsComposition.step(self, t)
        e, o0, o1 = self.env, self.obs[t % 2], self.obs[(t + 1) % 2]
        self.Ls[0].act(o0, -1.0, 5, t, index_out=self.act)           # (one net: no gather, no scatter)
        _lib.check(e.lib.uavenv_step(e._h, self.act.data_ptr(), _lib.ACT_INDEX_I32, o1.data_ptr(), self.r64.data_ptr(), None,
                                     None, self.adone.data_ptr(), self.info.data_ptr(), self.valid.data_ptr(),
                                     self.en.data_ptr(), None, _lib.STEP_SKIP_DONE, e._stream()), "uavenv_step")


def main_wide(args):
    """Heads of more than 4 layer-2 outputs (the wide instantiations of k_eval_episodes / k_eval_episodes_slots): a 9-action Qnet2
    and a 13-action dueling VAnet2 (14 outputs), untrained; one net on a non-APF env, and four nets (U = 4) with APF off and on;
    each against the composed launches that take such heads: set_state + per step uavenv_dqn_act per net (eps = -1) + uavenv_step."""
    torch.cuda.set_device(0)
    probe = make_city26_env(64, obs_dtype="packed")
    scn = ev.held_out_scenarios(probe, 16384, seed=0xE7A1)
    probe.close()
    out = {"what": "greedy evaluation of untrained wide heads (Qnet2 with 9 actions; dueling VAnet2 with 13 actions = 14 layer-2 "
                   "outputs) in one launch on held-out city26 episodes against set_state + per step uavenv_dqn_act per net (eps = -1; "
                   "four nets: slot rows gathered, actions scattered) + uavenv_step (k_apf_adjust + k_step with APF on).  Launches only, "
                   "device events, a warm-up, the two forms alternating, median of %d" % args.reps,
           "max_steps": args.max_steps, "sizes": []}
    for net, kind, A in (("Qnet2", "dqn", 9), ("VAnet2", "dueling", 13)):
        for U, apf in ((1, 0), (4, 0), (4, 1)):
            Ls = []
            for j in range(U):
                torch.manual_seed(j)
                Ls.append(FusedDQNLearner(dict(PARAM, NetWork=net, output=str(A)), kind, device="cuda:0"))
            for n in (int(x) for x in args.sizes.split(",")):
                v0 = np.random.default_rng(n).uniform(0, 2 * np.pi, n)
                v0 = np.stack([np.cos(v0), np.sin(v0)], 1)
                comp = WideComposition(Ls, scn, n, v0, apf, args.max_steps, A)
                ref, n_steps = comp.records()
                kw = dict(scenarios=scn, v0=v0, max_steps=args.max_steps)
                who = Ls if U > 1 else Ls[0]
                res = ev.evaluate_policy(comp.env, who, n, **kw)
                rec = res.host_records()
                ok = (np.array_equal(rec["ret"], ref["ret"]) and np.array_equal(rec["energy"], ref["energy"]) and
                      np.array_equal(rec["steps"], ref["steps"]) and np.array_equal(rec["outcome"], ref["outcome"]))
                if not ok:
                    raise SystemExit(f"{net} A = {A}, U = {U}, apf {apf}, n = {n}: the kernel's records differ from the composition's; "
                                     "no time reported")
                agent_steps = int(rec["steps"].sum())

                def timed_eval():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    ev.evaluate_policy(comp.env, who, n, **kw)
                    b.record()
                    b.synchronize()
                    return a.elapsed_time(b)

                timed_eval()
                comp.timed(min(n_steps, 32))
                t_eval, t_comp = [], []
                for _ in range(args.reps):               # the two forms alternating
                    t_eval.append(timed_eval())
                    t_comp.append(comp.timed(n_steps))
                me, mc = float(np.median(t_eval)), float(np.median(t_comp))
                row = {"net": net, "n_actions": A, "outputs": A + (kind == "dueling"), "nets": U, "apf": apf, "episodes": n,
                       "agent_steps": agent_steps, "steps_longest": n_steps, "records_equal": True,
                       "eval_ms": me, "eval_ms_all": t_eval, "comp_ms": mc, "comp_ms_all": t_comp,
                       "comp_form": ("4 x (gather + dqn_act + scatter)" if U > 1 else "dqn_act") + (" + apf_adjust + step" if apf else " + step"),
                       "eval_agent_steps_per_s": agent_steps / (me * 1e-3), "comp_agent_steps_per_s": agent_steps / (mc * 1e-3),
                       "eval_us_per_episode": me * 1e3 / n, "comp_us_per_episode": mc * 1e3 / n, "speedup": mc / me,
                       "summary": res.summary()}
                print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all") and k != "summary"}), flush=True)
                out["sizes"].append(row)
                comp.env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,65536,262144")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sac", action="store_true", help="time uavenv_eval_episodes_sac (APF off and on) instead")
    ap.add_argument("--max-steps", type=int, default=600, help="--sac / --slots / --f16: truncate episodes (0: natural ends)")
    ap.add_argument("--slots", action="store_true", help="time uavenv_eval_episodes_slots (four DQN nets, APF off and on) instead")
    ap.add_argument("--f16", action="store_true", help="time uavenv_eval_episodes_f16 (an f16-MFMA net on f16 and packed rows) instead")
    ap.add_argument("--once", type=int, default=0, help="--slots / --scripted: no timing, one launch per APF setting at this many episodes (per net)")
    ap.add_argument("--scripted", action="store_true", help="time uavenv_eval_episodes_scripted (the scripted baseline, APF off and on) instead")
    ap.add_argument("--lookahead", type=int, default=8, help="--scripted: the policy's look-ahead")
    ap.add_argument("--wide", action="store_true", help="time the wide heads (9-action Qnet2, 13-action VAnet2: one net, four nets, APF off and on) instead")
    args = ap.parse_args()
    if args.wide:
        args.out = args.out or "profiles/eval_wide_times.json"
        return main_wide(args)
    if args.scripted:
        args.out = args.out or "profiles/eval_scripted_times.json"
        return main_scripted(args)
    if args.f16:
        args.out = args.out or "profiles/eval_f16_times.json"
        return main_f16(args)
    if args.out is None:
        args.out = "profiles/eval_slots_times.json" if args.slots else "profiles/eval_sac_times.json" if args.sac else "profiles/eval_times.json"
    if args.slots:
        return main_slots_once(args) if args.once > 0 else main_slots(args)
    if args.sac:
        return main_sac(args)
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
