"""Policy evaluation: whole episodes in one GPU launch -- greedy DQN (csrc/uavenv.hip k_eval_episodes, include/uavenv.h
uavenv_eval_episodes; an f16-MFMA learner: k_eval_episodes_h, uavenv_eval_episodes_f16; one net per UAV slot and APF envs:
k_eval_episodes_slots, uavenv_eval_episodes_slots), the continuous SAC actor, APF on or off (k_eval_episodes_sac,
uavenv_eval_episodes_sac), and the scripted baseline they are held to: sub-goal pursuit with look-ahead, no learning
(k_eval_episodes_scripted, uavenv_eval_episodes_scripted; its act launch alone: uavenv_scripted_act).

The reference meant to have this (Envs/PathPlan_City.py:349-351 Evaluation_Action, :543-552 run_XML_scene / Load_Scene_FromXML)
and acts greedily when Is_Train == 0 (Trainer/DuelingDQN_Trainer.py:90).  Episode e flies scenario row (first + e) mod m of a
scenario set -- the env's reset bank, or a held-out set (held_out_scenarios) -- with the greedy action of the learner's q_local,
and leaves one 64-byte record.  The env's agents, tick and replay are not touched: evaluating between training calls does not
change the training run.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib

RECORD_DTYPE = np.dtype([("ret", "<f8"), ("total_score", "<f8"), ("path_len", "<f8"), ("energy", "<f8"), ("v0x", "<f8"),
                         ("v0y", "<f8"), ("steps", "<i4"), ("subgoals", "<i4"), ("collisions", "<i4"), ("outcome", "u1"),
                         ("reach_goal", "u1"), ("slot", "u1"), ("reserved", "u1")])
assert RECORD_DTYPE.itemsize == _lib.EVAL_RECORD_BYTES
OUTCOMES = {"success": _lib.EVAL_SUCCESS, "lose": _lib.EVAL_LOSE, "truncated": _lib.EVAL_TRUNCATED,
            "invalid": _lib.EVAL_INVALID}


def summarize(rec: np.ndarray) -> dict:
    """Counts and means of a structured array of RECORD_DTYPE (the means over the valid episodes)."""
    rec = np.asarray(rec)
    out = {"episodes": int(len(rec))}
    for name, code in OUTCOMES.items():
        out[name] = int((rec["outcome"] == code).sum())
    valid = rec[rec["outcome"] != _lib.EVAL_INVALID]
    nv = len(valid)
    out["success_rate"] = out["success"] / nv if nv else 0.0
    out["lose_rate"] = out["lose"] / nv if nv else 0.0

    def mean(field):
        return float(valid[field].astype(np.float64).mean()) if nv else 0.0

    out["mean_return"] = mean("ret")
    out["mean_steps"] = mean("steps")
    out["mean_path_len"] = mean("path_len")
    out["mean_energy"] = mean("energy")
    out["mean_subgoals"] = mean("subgoals")
    out["mean_collisions"] = mean("collisions")
    out["average_score"] = mean("total_score")
    return out


@dataclass
class EvalResult:
    """records: uint8 device tensor [n, 64] (UavEvalRecord); positions / actions: the optional trajectory, device tensors
    [n, T + 1, 3] f64 (NaN past an episode's end) and [n, T] int8 (-1 past the end) -- from evaluate_sac_policy the actions
    are [n, T, 2] f32, the two components get_action returns (NaN past the end)."""
    records: object
    positions: Optional[object] = None
    actions: Optional[object] = None

    def host_records(self) -> np.ndarray:
        return self.records.cpu().numpy().reshape(-1).view(RECORD_DTYPE)

    def summary(self) -> dict:
        return summarize(self.host_records())


def _check_args(n_episodes, first, eps, max_steps, trajectory_steps, max_workgroups):
    if int(n_episodes) != n_episodes or n_episodes <= 0:
        raise ValueError(f"n_episodes must be a positive integer (got {n_episodes!r})")
    if int(first) != first or first < 0:
        raise ValueError(f"first must be a non-negative integer (got {first!r})")
    if not np.isfinite(eps) or eps < 0.0 or eps > 1.0:
        raise ValueError(f"eps must lie in [0, 1] (got {eps!r})")
    for name, val in (("max_steps", max_steps), ("trajectory_steps", trajectory_steps), ("max_workgroups", max_workgroups)):
        if int(val) != val or val < 0:
            raise ValueError(f"{name} must be a non-negative integer (got {val!r})")


def _check_scenarios(scenarios, K):
    if scenarios is None:
        return None
    if len(scenarios) < 3:
        raise ValueError("scenarios = (start_goal [m,6], sub_goals [m,K,3], n_sub [m]), e.g. env.rrt_plan(...)[:3]")
    sg, sub, ns = scenarios[0], scenarios[1], scenarios[2]
    m = int(sg.shape[0]) if hasattr(sg, "shape") else -1
    if m <= 0 or tuple(sg.shape) != (m, 6) or tuple(sub.shape) != (m, K, 3) or tuple(ns.shape) != (m,):
        raise ValueError(f"scenario arrays must be [m,6], [m,{K},3], [m] with m > 0")
    return m


def _prepare(env, a, n, T, m, scenarios, first, seed, max_steps, v0, max_workgroups, act_tail, act_fill, act_dtype):
    """What evaluate_policy and evaluate_sac_policy share once their checks have passed: the v0 and scenario tensors on the env's
    device, the records and the trajectory tensors (actions [n, T, *act_tail] of act_dtype, filled with act_fill), and the
    common fields of the argument struct `a` (UavEvalArgs or UavSacEvalArgs).  -> (records, pos, act, keep): keep holds what
    the launch reads and nothing else references."""
    import torch
    dev = env.device
    if v0 is not None:
        v0 = torch.as_tensor(v0, dtype=torch.float64, device=dev).contiguous()
    if scenarios is not None:
        sg = torch.as_tensor(scenarios[0], dtype=torch.float64, device=dev).contiguous()
        sub = torch.as_tensor(scenarios[1], dtype=torch.float64, device=dev).contiguous()
        ns = torch.as_tensor(scenarios[2], dtype=torch.int32, device=dev).contiguous()
    records = torch.zeros((n, _lib.EVAL_RECORD_BYTES), dtype=torch.uint8, device=dev)
    pos = act = None
    if T > 0:
        pos = torch.full((n, T + 1, 3), float("nan"), dtype=torch.float64, device=dev)
        act = torch.full((n, T) + tuple(act_tail), act_fill, dtype=act_dtype, device=dev)
    a.n, a.first = n, int(first)
    if scenarios is not None:
        a.start_goal, a.sub, a.nsub, a.m = sg.data_ptr(), sub.data_ptr(), ns.data_ptr(), m
    a.max_steps = int(max_steps)
    a.v0 = None if v0 is None else v0.data_ptr()
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.traj_steps = T
    a.records = records.data_ptr()
    a.traj_pos = None if pos is None else pos.data_ptr()
    a.traj_act = None if act is None else act.data_ptr()
    a.max_workgroups = int(max_workgroups)
    return records, pos, act, (v0, scenarios if scenarios is None else (sg, sub, ns))


def evaluate_policy(env, learner, n_episodes: int, *, scenarios=None, first: int = 0, seed: int = 0, eps: float = 0.0,
                    max_steps: int = 0, v0=None, trajectory_steps: int = 0, max_workgroups: int = 0) -> EvalResult:
    """n_episodes greedy episodes of learner.q_local (a FusedDQNLearner) on env (a VecPathPlanEnv, APF on or off).

    learner: one FusedDQNLearner, or a list / tuple of 1 or env.uav_per_env of them -- episode e is then flown by learner e mod U,
    as UAV slot e mod U, all of them in ONE launch (uavenv_eval_episodes_slots; max_workgroups then bounds the workgroups per
    learner).  A single learner on a non-APF env goes through uavenv_eval_episodes; a list, or an APF env, through the slots entry
    (an APF env keeps one [K, 3] f64 sub-goal list per resident lane, 256 lanes per workgroup).  A single learner with
    mfma = "f16" goes through uavenv_eval_episodes_f16 -- the f16-MFMA forward it acts with, on the halves an f16 or packed env
    feeds it -- and needs a non-APF env with f16 or packed rows; the list and APF forms take f32-MFMA learners only.
    Heads: f32-MFMA learners of up to _lib.EVAL_MAX_OUTPUTS = 14 layer-2 outputs (n_actions + 1 for a dueling net) -- above 4 the
    same entries launch the kernels' wide instantiation, with the same Q values bit for bit as the learner's act launch -- and
    f16-MFMA learners of up to 4; ValueError beyond, before anything is enqueued.

    scenarios: None (the env's bank) or (start_goal [m,6] f64, sub_goals [m,K,3] f64, n_sub [m] i32) device tensors, e.g.
    held_out_scenarios(env, m, seed).  v0: [n,2] raw initial V_vector per episode (default: headings from Philox(seed, e)).
    eps > 0 takes a uniform action with probability eps (eps = 1: the random policy).  max_steps > 0 truncates.  Enqueued on
    the current stream; the records are read when summary() / host_records() is called."""
    # every check first: nothing is read from the device or enqueued before the arguments are known to be good
    _check_args(n_episodes, first, eps, max_steps, trajectory_steps, max_workgroups)
    m = _check_scenarios(scenarios, env.K)
    n, T = int(n_episodes), int(trajectory_steps)
    as_list = isinstance(learner, (list, tuple))
    ls = list(learner) if as_list else [learner]
    if not ls or any(getattr(L, "net", None) is None for L in ls):
        raise ValueError("evaluate_policy needs a fused learner (FusedDQNLearner), or a list of them")
    if as_list:
        kinds = {(getattr(L.net, "n_actions", None), getattr(L.net, "dueling", None)) for L in ls}
        if any(k is None for kind in kinds for k in kind):
            raise ValueError("evaluate_policy needs fused learners (FusedDQNLearner)")
        if len(kinds) != 1:
            raise ValueError(f"the learners must share one kind and action count (got (n_actions, dueling) = {sorted(kinds)})")
        if any(getattr(L, "mfma", "f32") != "f32" for L in ls):
            raise ValueError("the per-slot form (a list of learners) takes f32-MFMA nets only; evaluate an f16-MFMA learner on its own")
    f16 = not as_list and getattr(learner, "mfma", "f32") == "f16"
    n2 = max(int(getattr(L.net, "n_actions", 0)) + (1 if getattr(L.net, "dueling", 0) else 0) for L in ls)
    if n2 > _lib.EVAL_MAX_OUTPUTS:
        raise ValueError(f"the episode kernels take heads of at most {_lib.EVAL_MAX_OUTPUTS} layer-2 outputs (n_actions + dueling; got {n2})")
    if f16 and n2 > 4:
        raise ValueError(f"an f16-MFMA learner is evaluated with at most 4 layer-2 outputs (n_actions + dueling; got {n2})")
    if v0 is not None and tuple(np.shape(v0)) != (n, 2):
        raise ValueError(f"v0 must be [{n}, 2] (got {tuple(np.shape(v0))})")
    if as_list and len(ls) != 1 and len(ls) != env.uav_per_env:
        raise ValueError(f"one learner or uav_per_env = {env.uav_per_env} of them (got {len(ls)})")
    if f16 and int(env.cfg.apf_enabled) == 1:
        raise ValueError("an f16-MFMA learner is evaluated on non-APF envs only (the APF form takes f32-MFMA nets)")
    if f16 and env.obs_code not in (_lib.OBS_F16, _lib.OBS_PACKED):
        raise ValueError("an f16-MFMA learner is evaluated on an env with f16 or packed rows (what it acts on), not f32 rows")
    import torch
    a = _lib.UavEvalArgs()
    records, pos, act, keep = _prepare(env, a, n, T, m, scenarios, first, seed, max_steps, v0, max_workgroups, (), -1, torch.int8)
    a.eps = float(eps)
    if f16:
        _lib.check(env.lib.uavenv_eval_episodes_f16(env._h, C.byref(learner.net), C.byref(a), env._stream()), "uavenv_eval_episodes_f16")
    elif as_list or int(env.cfg.apf_enabled) == 1:
        nets = (C.POINTER(_lib.UavDqnNet) * len(ls))(*[C.pointer(L.net) for L in ls])
        _lib.check(env.lib.uavenv_eval_episodes_slots(env._h, nets, len(ls), C.byref(a), env._stream()), "uavenv_eval_episodes_slots")
    else:
        _lib.check(env.lib.uavenv_eval_episodes(env._h, C.byref(learner.net), C.byref(a), env._stream()), "uavenv_eval_episodes")
    res = EvalResult(records, pos, act)
    res._keep = keep + (ls,)           # alive until the launch has read them
    return res


SAC_MODES = {"mean": _lib.EVAL_SAC_MEAN, "sample": _lib.EVAL_SAC_SAMPLE}


def evaluate_sac_policy(env, learners, n_episodes: int, *, scenarios=None, first: int = 0, seed: int = 0, mode: str = "mean",
                        max_steps: int = 0, v0=None, trajectory_steps: int = 0, max_workgroups: int = 0) -> EvalResult:
    """n_episodes episodes of the SAC actor(s) on env (a VecPathPlanEnv, APF on or off) in one launch (csrc/uavenv.hip
    k_eval_episodes_sac, include/uavenv.h uavenv_eval_episodes_sac).

    learners: one FusedSACLearner, or a list of env.uav_per_env of them -- episode e is then flown by learner e mod U, as UAV
    slot e mod U.  The reference's get_action always samples (Trainer/SAC_Trainer.py:444-448), so mode is "mean" (noise 0: the
    action of the distribution's centre) or "sample" (noise ~ N(0, 1) from Philox on `seed`; sac_noise gives the same numbers).
    The other arguments, the records and the positions are evaluate_policy's; actions are [n, T, 2] f32.  max_workgroups
    bounds the workgroups per learner (an APF env keeps one [K, 3] f64 sub-goal list per resident lane, 256 lanes per
    workgroup).  Enqueued on the current stream."""
    # every check first: nothing is read from the device or enqueued before the arguments are known to be good
    _check_args(n_episodes, first, 0.0, max_steps, trajectory_steps, max_workgroups)
    if mode not in SAC_MODES:
        raise ValueError(f"mode must be one of {sorted(SAC_MODES)} (got {mode!r})")
    m = _check_scenarios(scenarios, env.K)
    n, T = int(n_episodes), int(trajectory_steps)
    ls = list(learners) if isinstance(learners, (list, tuple)) else [learners]
    if not ls or any(getattr(L, "_blocks", None) is None or getattr(L, "action_bound", None) is None for L in ls):
        raise ValueError("evaluate_sac_policy needs fused SAC learners (FusedSACLearner)")
    bound = float(ls[0].action_bound)
    if not np.isfinite(bound) or bound <= 0.0 or any(float(L.action_bound) != bound for L in ls):
        raise ValueError("the learners must share one positive, finite action_bound")
    if v0 is not None and tuple(np.shape(v0)) != (n, 2):
        raise ValueError(f"v0 must be [{n}, 2] (got {tuple(np.shape(v0))})")
    if len(ls) != 1 and len(ls) != env.uav_per_env:
        raise ValueError(f"one learner or uav_per_env = {env.uav_per_env} of them (got {len(ls)})")
    import torch
    a = _lib.UavSacEvalArgs()
    records, pos, act, keep = _prepare(env, a, n, T, m, scenarios, first, seed, max_steps, v0, max_workgroups, (2,), float("nan"),
                                       torch.float32)
    actors = (C.c_void_p * len(ls))(*[L._blocks[0].data_ptr() for L in ls])
    a.actors, a.n_actors = actors, len(ls)
    a.action_bound = bound
    a.mode = SAC_MODES[mode]
    _lib.check(env.lib.uavenv_eval_episodes_sac(env._h, C.byref(a), env._stream()), "uavenv_eval_episodes_sac")
    res = EvalResult(records, pos, act)
    res._keep = keep + (ls,)           # alive until the launch has read them
    return res


SCRIPTED_KINDS = {"index": _lib.ACT_INDEX_I32, "steer": _lib.ACT_STEER_F32}


def _scripted_policy(env, action, candidates, lookahead):
    """The checked UavScriptedPolicy of (action, candidates, lookahead) for env: action "index" takes the env's n_actions as its
    candidates (candidates None or 0), "steer" an odd number of f32 steers (default 9).  Reads env.cfg only."""
    if action not in SCRIPTED_KINDS:
        raise ValueError(f"action must be one of {sorted(SCRIPTED_KINDS)} (got {action!r})")
    if isinstance(lookahead, bool) or int(lookahead) != lookahead or not 0 <= lookahead <= _lib.SCRIPTED_MAX_LOOKAHEAD:
        raise ValueError(f"lookahead must be an integer in 0..{_lib.SCRIPTED_MAX_LOOKAHEAD} (got {lookahead!r})")
    if action == "index":
        if candidates not in (None, 0):
            raise ValueError(f"action='index' takes the env's n_actions as its candidates: leave candidates None (got {candidates!r})")
        A = int(env.cfg.n_actions)
        if not 2 <= A <= _lib.SCRIPTED_MAX_INDEX_ACTIONS:
            raise ValueError(f"action='index' needs an env with 2..{_lib.SCRIPTED_MAX_INDEX_ACTIONS} actions (it has {A})")
        c = 0
    else:
        c = 9 if candidates is None else candidates
        if isinstance(c, bool) or int(c) != c or not 3 <= c <= _lib.SCRIPTED_MAX_STEER_CANDIDATES or int(c) % 2 == 0:
            raise ValueError(f"candidates must be an odd integer in 3..{_lib.SCRIPTED_MAX_STEER_CANDIDATES} (got {candidates!r})")
    pol = _lib.UavScriptedPolicy()
    pol.action_kind, pol.candidates, pol.lookahead = SCRIPTED_KINDS[action], int(c), int(lookahead)
    return pol


def evaluate_scripted_policy(env, n_episodes: int, *, action: str = "index", candidates=None, lookahead: int = 8, scenarios=None,
                             first: int = 0, seed: int = 0, eps: float = 0.0, max_steps: int = 0, v0=None,
                             trajectory_steps: int = 0, max_workgroups: int = 0) -> EvalResult:
    """n_episodes episodes of the scripted baseline -- sub-goal pursuit with look-ahead, a controller that learns nothing -- on env
    (a VecPathPlanEnv, APF on or off) in one launch (csrc/uavenv.hip k_eval_episodes_scripted, include/uavenv.h
    uavenv_eval_episodes_scripted): the yardstick for evaluate_policy / evaluate_sac_policy, on the same missions.

    The policy steers at the current sub-goal (the steer that turns the heading onto its bearing, clamped to [-1, 1]) and takes
    the nearest candidate steer whose next `lookahead` positions are free; with every candidate blocked, the nearest one.
    action = "index": the candidates are the env's n_actions discrete steers (what a DQN learner chooses from); actions are
    [n, T] int8; eps > 0 takes evaluate_policy's uniform draw with probability eps.  action = "steer": `candidates` (odd, 3..17,
    default 9) f32 steers spread over [-1, 1] (what a SAC actor's component 0 is); actions are [n, T] f32 (NaN past the end);
    eps must be 0.  The other arguments, the records and the positions are evaluate_policy's.  Enqueued on the current stream."""
    # every check first: nothing is read from the device or enqueued before the arguments are known to be good
    _check_args(n_episodes, first, eps, max_steps, trajectory_steps, max_workgroups)
    pol = _scripted_policy(env, action, candidates, lookahead)
    if action == "steer" and eps > 0.0:
        raise ValueError("eps > 0 needs action='index' (the exploration draw is an index draw)")
    m = _check_scenarios(scenarios, env.K)
    n, T = int(n_episodes), int(trajectory_steps)
    if v0 is not None and tuple(np.shape(v0)) != (n, 2):
        raise ValueError(f"v0 must be [{n}, 2] (got {tuple(np.shape(v0))})")
    import torch
    a = _lib.UavEvalArgs()
    if action == "index":
        records, pos, act, keep = _prepare(env, a, n, T, m, scenarios, first, seed, max_steps, v0, max_workgroups, (), -1, torch.int8)
    else:
        records, pos, act, keep = _prepare(env, a, n, T, m, scenarios, first, seed, max_steps, v0, max_workgroups, (), float("nan"),
                                           torch.float32)
    a.eps = float(eps)
    _lib.check(env.lib.uavenv_eval_episodes_scripted(env._h, C.byref(pol), C.byref(a), env._stream()), "uavenv_eval_episodes_scripted")
    res = EvalResult(records, pos, act)
    res._keep = keep
    return res


def scripted_act(env, actions_out, *, action: str = "index", candidates=None, lookahead: int = 8):
    """The scripted baseline's act launch alone (uavenv_scripted_act): actions_out[i] = the action of agent i of env in its
    current state -- a contiguous [N] int32 tensor for action = "index", float32 for "steer", on the env's device -- ready for
    env.step(actions_out, ...), so scripted transitions can fill a replay ring.  The env is only read.  -> actions_out."""
    pol = _scripted_policy(env, action, candidates, lookahead)
    import torch
    want = torch.int32 if action == "index" else torch.float32
    if not isinstance(actions_out, torch.Tensor) or actions_out.dtype != want:
        raise ValueError(f"actions_out must be a {want} tensor for action={action!r}")
    if actions_out.numel() != env.N or not actions_out.is_contiguous() or actions_out.device != env.device:
        raise ValueError("actions_out must be a contiguous [N] tensor on the env device")
    _lib.check(env.lib.uavenv_scripted_act(env._h, C.byref(pol), actions_out.data_ptr(), env._stream()), "uavenv_scripted_act")
    return actions_out


def sac_noise(n: int, steps: int, seed: int, device="cuda:0"):
    """[n, steps, 2] f32: the noise evaluate_sac_policy(mode="sample", seed=seed) uses for episode e, step t, component d
    (uavenv_eval_noise_fill) -- to hand the same draws to FusedSACLearner.act_rows."""
    if int(n) != n or n <= 0 or int(steps) != steps or steps <= 0 or int(n) * int(steps) >= 1 << 31:
        raise ValueError(f"n and steps must be positive integers with n * steps < 2^31 (got {n!r}, {steps!r})")
    import torch
    dev = torch.device(device)
    out = torch.empty((int(n), int(steps), 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().uavenv_eval_noise_fill(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(steps), out.data_ptr(), stream),
                   "uavenv_eval_noise_fill")
    return out


def slot_scenarios(scenarios, uav_per_env: int, max_v: float, seed: int):
    """Every row r of a scenario set repeated uav_per_env times (at r * U + j) with ONE initial heading per row, drawn from
    numpy's PCG64 on `seed`: episode r * U + j then flies mission r, from the same start, heading and path, as UAV slot j
    (slot = episode mod U), so the slots' results compare mission for mission.  -> ((start_goal, sub_goals, n_sub), v0) with
    v0 = the raw initial V_vector [m * U, 2]."""
    import torch
    sg, sub, ns = scenarios
    U = int(uav_per_env)
    if U <= 0:
        raise ValueError(f"uav_per_env must be positive (got {uav_per_env!r})")
    m = int(sg.shape[0])
    t = np.random.default_rng(int(seed)).uniform(0.0, 2.0 * np.pi, m)
    v0 = np.repeat(np.stack([max_v * np.cos(t), max_v * np.sin(t)], 1), U, axis=0)
    rep = tuple(torch.as_tensor(x).repeat_interleave(U, dim=0).contiguous() for x in (sg, sub, ns))
    return rep, torch.as_tensor(v0, dtype=torch.float64, device=rep[0].device)


def held_out_scenarios(env, m: int, seed: int, max_iter: int = 10000):
    """The first m valid rows (2 <= n_sub <= K) of the GPU planner on `seed` -- pick a seed the training bank never used.
    n_sub = 1 is the planner's give-up marker (a path of [goal] only, csrc/rrt.hip) and n_sub < 0 a path longer than K."""
    if int(m) != m or m <= 0:
        raise ValueError(f"m must be a positive integer (got {m!r})")
    import torch
    sgs, subs, nss, have, k = [], [], [], 0, 0
    while have < m:
        ask = max(2 * (m - have), 1024)
        sg, sub, ns, _ = env.rrt_plan(ask, seed=int(seed) + k * 0x9E3779B1, max_iter=max_iter)
        ok = (ns >= 2) & (ns <= env.K)
        sgs.append(sg[ok]); subs.append(sub[ok]); nss.append(ns[ok])
        have += int(ok.sum())
        k += 1
        if k >= 8 and have < m:
            raise RuntimeError(f"held_out_scenarios: only {have} of {m} planned paths are valid after {k} rounds")
    return torch.cat(sgs)[:m].contiguous(), torch.cat(subs)[:m].contiguous(), torch.cat(nss)[:m].contiguous()
