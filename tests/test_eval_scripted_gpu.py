"""The scripted baseline on the device (uavenv_scripted_act: k_scripted_act; uavenv_eval_episodes_scripted:
k_eval_episodes_scripted), APF off and on, against
  * an independent float64 reference of the rule (tests/scripted_policy_ref.py) on the C oracle's state;
  * the composition of the launches: set_state -> scripted_act -> env.step(skip_done), accumulated on the host -- bit for bit;
  * the net entries (uavenv_eval_episodes, uavenv_eval_episodes_slots) under eps = 1, where the policy does not matter;
  * the C oracle (oracle/uav_oracle.c), which shares no code with the device step.
Where the device and the reference may legitimately differ -- a decision whose margin is below 1e-6 (scripted_policy_ref.FRAGILE) --
either side's action is accepted, and such decisions are counted and capped."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev
from dqn_based_uav_3d_path_planer_amd.data import load_city26
from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
from test_eval_sac_gpu import _env, _hand_rows, _oracle_batch, _scenarios, _state_bytes, _v0, _velocities

import scripted_policy_ref as spr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (action, candidates, lookahead): the index kind on the env's 3 actions with and without look-ahead, the steer kind
POLICIES = [("index", None, 4), ("index", None, 0), ("steer", 9, 4)]
IDS = ["index-H4", "index-H0", "steer9-H4"]
DQN_PARAM = {"w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99", "Update_loop": "3", "NetWork": "Qnet2"}


def _kw(pol):
    return dict(action=pol[0], candidates=pol[1], lookahead=pol[2])


def _ref_policy(pol, apf):
    c = load_city26()
    return spr.city_policy(c, pol[0], 3 if pol[0] == "index" else pol[1], pol[2], velocities=_velocities() if apf else None)[0]


def _act_dtype(pol):
    return torch.int32 if pol[0] == "index" else torch.float32


# ---- 1. the act kernel against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", POLICIES, ids=IDS)
@pytest.mark.parametrize("U", [1, 4])
@pytest.mark.parametrize("apf", [0, 1])
def test_act_kernel_matches_the_reference(apf, U, pol):
    """1024 agents in varied states (a bank reset, then 50 steps of random steers: some are done, some have collided, with APF the
    sub-goal lists have moved): scripted_act's output equals the reference's decision on uavenv_get_state's view of each agent --
    equal indices / equal f32 bits -- at every agent whose decision is not fragile; fragile ones are at most 0.5 %; a done agent
    gets the middle candidate; the env's state bytes do not change."""
    env = _env(1024 // U, apf, U)
    env.reset(seed=31 + 2 * apf + U)
    # (eight agents with an empty list: done after their first step, and left alone by the steps after it)
    kin = np.tile([100.0, 100.0, 90.0, 1.0, 0.0, 300.0, 300.0, 90.0], (8, 1))
    env.set_state(0, kin, np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros((8, env.K, 3)))
    g = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(50):
        env.step((torch.rand(env.N, device=DEV, generator=g) * 2 - 1).float(), skip_done=True)
    before, tick = _state_bytes(env), env.lib.uavenv_tick(env._h)
    out = torch.full((env.N,), 77, dtype=_act_dtype(pol), device=DEV)
    assert ev.scripted_act(env, out, **_kw(pol)) is out
    got = out.cpu().numpy()
    assert _state_bytes(env) == before and env.lib.uavenv_tick(env._h) == tick
    st, sub, _ = env.get_state(0, env.N, want_sub=True)
    ref = _ref_policy(pol, apf)
    d = ref.decide_state(st, sub)
    done = st[:, 10] == 1
    assert done[:8].all() and (~done).sum() > 500
    want = ref.action(d)
    mid = ref.C // 2
    want[done] = mid if pol[0] == "index" else np.float32(spr.candidate_steers("steer", ref.C)[mid])
    fragile = d.fragile & ~done
    same = got.view(np.uint32) == want.view(np.uint32)
    print(f"act apf={apf} U={U} {pol}: {int(fragile.sum())} fragile, {int((~same).sum())} differ, {int(done.sum())} done, "
          f"{int(d.blocked.any(1).sum())} with a blocked candidate")
    assert same[~fragile].all()
    assert fragile.sum() <= 0.005 * env.N
    if pol[2] > 0:
        assert d.blocked[~done].any() and not d.blocked[~done].all()             # the look-ahead mattered for some agents
    assert len(np.unique(got[~done])) >= 3
    env.close()


# ---- 2. episodes equal the composition, bit for bit -------------------------------------------------------------------------------
def _compose(pol, U, apf, scn, rows, v0, max_steps):
    """The same episodes through the act launch and the step launches: agent i of a fresh env (uav_per_env = U) is episode i, UAV
    slot i mod U (tests/test_eval_slots_gpu.py::_compose with scripted_act in the nets' place)."""
    n = len(rows)
    assert n % U == 0
    sg, sub, ns = (x.cpu().numpy() for x in scn)
    env2 = _env(n // U, apf, U)
    kin = np.concatenate([sg[rows, :3], v0, sg[rows, 3:]], 1)
    nsub = ns[rows]
    env2.set_state(0, kin, np.zeros(n, np.int32), nsub, sub[rows], alias=(nsub >= 2).astype(np.int32))
    out = env2.alloc_out(want_energy=True)
    act = torch.zeros(n, dtype=_act_dtype(pol), device=DEV)
    st = env2.get_state(0, n)
    final = st.copy()
    ret, energy = np.zeros(n), np.zeros(n)
    steps, coll = np.zeros(n, np.int64), np.zeros(n, np.int64)
    outcome = np.zeros(n, np.int64)
    pos, acts = [st[:, :3].copy()], []
    cap = nsub.astype(np.int64) * env2.cfg.max_step + 1
    t = 0
    while (outcome == 0).any():
        ev.scripted_act(env2, act, **_kw(pol))
        env2.step(act, out, skip_done=True)
        nst = env2.get_state(0, n)
        v = (out.valid.cpu().numpy() == 1) & (outcome == 0)        # (a truncated agent flies on here; its episode has ended)
        ret[v] += out.reward.cpu().numpy()[v]
        energy[v] += out.energy.cpu().numpy()[v]
        steps[v] += 1
        same = (nst[:, 0] == st[:, 0]) & (nst[:, 1] == st[:, 1]) & (nst[:, 2] == st[:, 2])
        coll[v & same & (st[:, 11] > 0)] += 1                       # a moved step whose position did not change
        a = act.cpu().numpy().astype(np.float64)
        a[~v] = -1 if pol[0] == "index" else np.nan
        acts.append(a)
        p = nst[:, :3].copy()
        p[~v] = np.nan
        pos.append(p)
        inf = out.info.cpu().numpy()
        d = v & (out.agent_done.cpu().numpy() == 1)
        outcome[d] = np.where(inf[d] == _lib.INFO_LOSE, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS)
        tr = v & (outcome == 0) & (((max_steps > 0) & (steps >= max_steps)) | (steps >= cap))
        outcome[tr] = _lib.EVAL_TRUNCATED
        final[v] = nst[v]
        st = nst
        t += 1
        assert t < 20000, "the composition did not finish"
    env2.close()
    return dict(ret=ret, energy=energy, steps=steps, coll=coll, outcome=outcome, state=final, nsub=nsub,
                pos=np.stack(pos, 1), act=np.stack(acts, 1))


def _check_equal(rec, res, ref, v0, T, U, index):
    assert (rec["outcome"] == ref["outcome"]).all()
    assert (rec["steps"] == ref["steps"]).all()
    assert np.array_equal(rec["ret"], ref["ret"])
    assert np.array_equal(rec["energy"], ref["energy"])
    assert (rec["collisions"] == ref["coll"]).all()
    assert (rec["subgoals"] == ref["nsub"] - ref["state"][:, 11]).all()
    assert np.array_equal(rec["total_score"], ref["state"][:, 13])
    assert np.array_equal(rec["path_len"], ref["state"][:, 14])
    assert (rec["reach_goal"] == ref["state"][:, 15]).all()
    assert np.array_equal(rec["v0x"], v0[:, 0]) and np.array_equal(rec["v0y"], v0[:, 1])
    assert (rec["slot"] == np.arange(len(rec)) % U).all() and (rec["reserved"] == 0).all()
    pos = res.positions.cpu().numpy()
    act = res.actions.cpu().numpy().astype(np.float64)             # (int8 indices and f32 steers are exact in f64)
    assert res.actions.dtype == (torch.int8 if index else torch.float32) and tuple(res.actions.shape) == (len(rec), T)
    k = min(T + 1, ref["pos"].shape[1])
    assert np.array_equal(pos[:, :k], ref["pos"][:, :k], equal_nan=True)
    assert np.array_equal(act[:, :k - 1], ref["act"][:, :k - 1], equal_nan=True)
    assert np.isnan(pos[:, k:]).all()
    assert (act[:, k - 1:] == -1).all() if index else np.isnan(act[:, k - 1:]).all()


@pytest.mark.parametrize("pol", POLICIES, ids=IDS)
@pytest.mark.parametrize("U", [1, 4])
@pytest.mark.parametrize("apf", [0, 1])
def test_episodes_equal_the_composed_launches(apf, U, pol):
    scn = _scenarios()
    env = _env(64, apf, U)
    n, T, cap = 2048, 600, 600
    m = scn[0].shape[0]
    rows = np.arange(n) % m
    v0 = _v0(n, 1000 * apf + 100 * U + pol[2])
    # one workgroup: every lane flies 8 episodes one after another
    res = ev.evaluate_scripted_policy(env, n, scenarios=scn, v0=v0, max_steps=cap, trajectory_steps=T, max_workgroups=1, **_kw(pol))
    rec = res.host_records()
    ref = _compose(pol, U, apf, scn, rows, v0, cap)
    _check_equal(rec, res, ref, v0, T, U, pol[0] == "index")
    print(f"episodes apf={apf} U={U} {pol}: {ev.summarize(rec)}")
    assert (rec["steps"] > 0).all() and rec["collisions"].sum() > 0 and rec["subgoals"].sum() > 0
    env.close()


# ---- 3. eps = 1 ties the new loop to the old kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("apf", [0, 1])
def test_eps_one_is_the_random_policy_of_the_net_entries(apf):
    """Index kind, eps = 1: every action is the exploration draw, so the records, positions and actions are byte for byte those of
    uavenv_eval_episodes (non-APF) / uavenv_eval_episodes_slots (APF) with eps = 1 and any net."""
    env = _env(64, apf, 1)
    torch.manual_seed(3)
    L = FusedDQNLearner(DQN_PARAM, "dqn", device=DEV)
    n = 3000 + 37
    kw = dict(seed=9, eps=1.0, first=5, max_steps=300, trajectory_steps=8)
    new = ev.evaluate_scripted_policy(env, n, action="index", lookahead=4, **kw)
    old = ev.evaluate_policy(env, [L] if apf else L, n, **kw)
    assert new.records.cpu().numpy().tobytes() == old.records.cpu().numpy().tobytes()
    assert new.positions.cpu().numpy().tobytes() == old.positions.cpu().numpy().tobytes()
    assert new.actions.cpu().numpy().tobytes() == old.actions.cpu().numpy().tobytes()
    rec = new.host_records()
    assert (rec["steps"] > 0).all()
    half = ev.evaluate_scripted_policy(env, n, action="index", lookahead=4, **dict(kw, eps=0.5)).host_records()
    none = ev.evaluate_scripted_policy(env, n, action="index", lookahead=4, **dict(kw, eps=0.0)).host_records()
    assert half.tobytes() != rec.tobytes() and half.tobytes() != none.tobytes()
    env.close()


# ---- 4. every ending ---------------------------------------------------------------------------------------------------------------
def _oracle_fly_policy(apf, ref, sg, sub, ns, rows, v0, cap, max_step):
    """Whole episodes of the reference policy on the C oracle alone -> outcome, steps, collisions, reach_goal, sub-goals popped,
    and per episode whether any of its decisions was fragile."""
    n = len(rows)
    batch = _oracle_batch(apf, sg, sub, ns, rows, v0)
    steps, coll, outcome = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    fragile = np.zeros(n, bool)
    reach, popped = np.zeros(n, np.int64), np.zeros(n, np.int64)
    capn = ns[rows].astype(np.int64) * max_step + 1
    while (outcome == 0).any():
        live = outcome == 0
        d = ref.decide_batch(batch)
        fragile |= live & d.fragile
        p0 = np.stack([batch.view["px"], batch.view["py"], batch.view["pz"]], 1).copy()
        left = batch.view["n_sub"].copy()
        _, _, info, _ = batch.step(np.where(live, d.steer, 0.0), want_obs=False)
        steps[live] += 1
        p1 = np.stack([batch.view["px"], batch.view["py"], batch.view["pz"]], 1)
        coll[live & (p0 == p1).all(1) & (left > 0)] += 1
        dn = live & (batch.view["done"] == 1)
        outcome[dn] = np.where(info[dn] == 2, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS)
        tr = live & (outcome == 0) & ((steps >= cap) | (steps >= capn))
        outcome[tr] = _lib.EVAL_TRUNCATED
        end = live & (outcome != 0)                     # (the oracle steps an ended agent on: its fields are taken here)
        reach[end] = batch.view["reach_goal"][end]
        popped[end] = ns[rows][end] - batch.view["n_sub"][end]
    return outcome, steps, coll, reach, popped, fragile


@pytest.mark.parametrize("apf", [0, 1])
def test_every_ending_is_exercised(apf):
    """The hand-built rows and the packaged bank under pure pursuit (index kind, H = 0) and with look-ahead (H = 4), cap 200.  The C
    oracle flown by the reference policy alone, on the CPU, says how each episode ends -- success by empty list (row 0), by the
    final sub-goal (row 1), by the goal within 7 m (row 2), lose, truncation, collisions -- and the kernel's records must show those
    endings for every episode without a fragile decision."""
    c = load_city26()
    a, b, d = _hand_rows(48)
    sg = np.concatenate([a, c["start_goal"]]); sub = np.concatenate([b, c["sub_goals"]])
    ns = np.concatenate([d, c["n_sub"]]).astype(np.int32)
    n, cap = len(sg), 200
    rows = np.arange(n)
    v0 = _v0(n, 7)
    env = _env(64, apf)
    scn = (torch.tensor(sg, device=DEV), torch.tensor(sub, device=DEV), torch.tensor(ns, device=DEV))
    seen = np.zeros(3, bool)
    for pol in (("index", None, 0), ("index", None, 4)):
        o, s, cl, rg, popped, fr = _oracle_fly_policy(apf, _ref_policy(pol, apf), sg, sub, ns, rows, v0, cap, int(c["max_step"]))
        # the oracle alone shows the endings
        assert o[0] == _lib.EVAL_SUCCESS and s[0] == 1 and rg[0] == 0 and popped[0] == 0           # empty list
        assert o[1] == _lib.EVAL_SUCCESS and rg[1] == 1 and popped[1] == 2                          # final sub-goal
        assert o[2] == _lib.EVAL_SUCCESS and rg[2] == 1 and popped[2] == 0                          # goal within 7 m
        assert not fr[:3].any() and fr.sum() <= 0.01 * n      # (tests/test_eval_scripted.py: fragile decisions are rare on these rows)
        seen |= [(o == _lib.EVAL_LOSE).any(), (o == _lib.EVAL_TRUNCATED).any(), (cl > 0).any()]
        assert (s[o == _lib.EVAL_TRUNCATED] == cap).all()
        rec = ev.evaluate_scripted_policy(env, n, scenarios=scn, v0=v0, max_steps=cap, **_kw(pol)).host_records()
        ok = ~fr
        print(f"endings apf={apf} {pol}: success {(o == 1).sum()} lose {(o == 2).sum()} truncated {(o == 4).sum()} "
              f"collided {(cl > 0).sum()} fragile episodes {fr.sum()}")
        assert (rec["outcome"][ok] == o[ok]).all() and (rec["steps"][ok] == s[ok]).all()
        assert (rec["reach_goal"][ok] == rg[ok]).all() and (rec["subgoals"][ok] == popped[ok]).all()
        assert (rec["collisions"][ok] == cl[ok]).all()
    assert seen.all()                                   # lose, truncation and a collision each occurred
    env.close()


# ---- 5. replay through the C oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", [POLICIES[0], POLICIES[2]], ids=[IDS[0], IDS[2]])
@pytest.mark.parametrize("apf", [0, 1])
def test_oracle_replay_of_recorded_actions(apf, pol):
    """The recorded actions of 256 episodes fed to the C oracle step by step from the same resets (APF: the same velocities).
    Outcome and step count exactly; positions and return within the bars of the existing replay tests (non-APF 1e-9 and 1e-9,
    tests/test_eval_gpu.py; APF 1e-8 and 1e-9 x steps, tests/test_eval_sac_gpu.py).  At every step the reference's decision on the
    oracle's state is the recorded action unless it is fragile (at most 0.1 % of the steps), and a step that collided had every
    candidate's next point blocked."""
    env = _env(64, apf)
    scn = _scenarios()
    n, T = 256, 600
    v0 = _v0(n, 71)
    res = ev.evaluate_scripted_policy(env, n, scenarios=scn, v0=v0, max_steps=T, trajectory_steps=T, **_kw(pol))
    rec = res.host_records()
    pos = res.positions.cpu().numpy()
    act = res.actions.cpu().numpy()
    sg, sub, ns = (x.cpu().numpy() for x in scn)
    rows = np.arange(n) % len(sg)
    ref = _ref_policy(pol, apf)
    steers = spr.candidate_steers(pol[0], ref.C)
    batch = _oracle_batch(apf, sg, sub, ns, rows, v0)
    assert np.abs(pos[:, 0] - np.stack([batch.view["px"], batch.view["py"], batch.view["pz"]], 1)).max() == 0.0
    steps = rec["steps"].astype(np.int64)
    assert (steps > 0).all()
    ret = np.zeros(n)
    outcome = np.zeros(n, np.int64)
    ended = np.zeros(n, bool)
    max_p, decisions, fragile, collided = 0.0, 0, 0, 0
    for t in range(int(steps.max())):
        alive = t < steps
        d = ref.decide_batch(batch)
        if pol[0] == "index":
            assert (act[alive, t] >= 0).all()
            a0 = np.where(alive, steers[act[:, t].clip(0)], 0.0)
            same = act[:, t] == d.k
        else:
            assert np.isfinite(act[alive, t]).all()
            a0 = np.where(alive, np.nan_to_num(act[:, t]).astype(np.float64), 0.0)
            same = act[:, t].view(np.uint32) == ref.action(d).view(np.uint32)
        assert (same | d.fragile)[alive].all(), t
        decisions += int(alive.sum())
        fragile += int((alive & d.fragile).sum())
        p0 = np.stack([batch.view["px"], batch.view["py"], batch.view["pz"]], 1).copy()
        left = batch.view["n_sub"].copy()
        r, _, info, _ = batch.step(a0, want_obs=False)
        ret[alive] += r[alive]
        p = np.stack([batch.view["px"], batch.view["py"], batch.view["pz"]], 1)
        hit = alive & (p0 == p).all(1) & (left > 0)
        assert d.all_blocked_t1[hit].all(), t           # a collision only where every candidate's next point was blocked
        collided += int(hit.sum())
        max_p = max(max_p, np.abs(p[alive] - pos[alive, t + 1]).max())
        done_now = alive & ~ended & (batch.view["done"] == 1)
        outcome[done_now] = np.where(info[done_now] == 2, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS)
        ended |= done_now
        assert not (ended & (t + 1 < steps)).any(), "the oracle ended an episode before the kernel did"
    outcome[~ended] = _lib.EVAL_TRUNCATED
    err = np.abs(ret - rec["ret"])
    print(f"oracle replay apf={apf} {pol}: max |position error| {max_p:.3e}, max |return error| {err.max():.3e}, "
          f"{fragile} fragile of {decisions} decisions, {collided} collisions, outcomes {np.bincount(outcome, minlength=5)}")
    assert (outcome == rec["outcome"]).all()
    assert (ended == (rec["outcome"] != _lib.EVAL_TRUNCATED)).all()
    if apf:
        assert max_p <= 1e-8 and (err <= 1e-9 * steps).all()
    else:
        assert max_p <= 1e-9 and err.max() <= 1e-9
    assert fragile <= 1e-3 * decisions
    assert collided == rec["collisions"].sum()
    assert (rec["outcome"] == _lib.EVAL_SUCCESS).any()
    assert (steps[rec["outcome"] == _lib.EVAL_TRUNCATED] == T).all()
    env.close()


# ---- 6. placement, repeatability, invalid rows --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", [POLICIES[0], POLICIES[2]], ids=[IDS[0], IDS[2]])
@pytest.mark.parametrize("apf", [0, 1])
def test_placement_invariance_and_repeatability(apf, pol):
    U = 4
    env = _env(64, apf, U)
    n = 3000 + 37                                  # neither a multiple of 64 nor of U
    outs = []
    for mw in (1, 3, 0, 0):                        # (1 -> 3 -> automatic: every call has more resident lanes than the one before)
        res = ev.evaluate_scripted_policy(env, n, seed=9, max_steps=300, max_workgroups=mw, trajectory_steps=8, **_kw(pol))
        outs.append(res.records.cpu().numpy().tobytes() + res.positions.cpu().numpy().tobytes() + res.actions.cpu().numpy().tobytes())
    assert outs[0] == outs[1] == outs[2] == outs[3]
    rec = np.frombuffer(outs[0][:n * 64], dtype=ev.RECORD_DTYPE)
    assert (rec["steps"] > 0).all() and (rec["slot"] == np.arange(n) % U).all()
    other = ev.evaluate_scripted_policy(env, n, seed=10, max_steps=300, **_kw(pol)).host_records()
    assert other.tobytes() != rec.tobytes()        # the seed draws the headings
    env.close()


@pytest.mark.parametrize("apf", [0, 1])
def test_invalid_rows_are_recorded_not_flown(apf):
    env = _env(64, apf)
    sg, sub, ns = (x.clone() for x in _scenarios())
    ns[5] = -3
    ns[6] = env.K + 1
    for pol in (POLICIES[0], POLICIES[2]):
        rec = ev.evaluate_scripted_policy(env, 16, scenarios=(sg, sub, ns), v0=_v0(16, 1), **_kw(pol)).host_records()
        assert (rec["outcome"][[5, 6]] == _lib.EVAL_INVALID).all() and (rec["steps"][[5, 6]] == 0).all()
        assert ((rec["outcome"] != _lib.EVAL_INVALID).sum() == 14)
    env.close()


# ---- 7. the env is left alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("apf", [0, 1])
def test_refusals_leave_the_env_unchanged(apf):
    U = 4
    env = _env(16, apf, U)
    env.reset(seed=4)
    act = torch.zeros(env.N, dtype=torch.float32, device=DEV)
    for _ in range(3):                             # (an APF env: the sub-goal lists have moved by now)
        env.step(act, skip_done=True)
    before, tick = _state_bytes(env), env.lib.uavenv_tick(env._h)
    rec = torch.zeros((64, 64), dtype=torch.uint8, device=DEV)
    acts = torch.zeros(env.N, dtype=torch.int32, device=DEV)
    lib = env.lib

    def policy(kind=_lib.ACT_INDEX_I32, candidates=0, lookahead=4):
        p = _lib.UavScriptedPolicy()
        p.action_kind, p.candidates, p.lookahead = kind, candidates, lookahead
        return p

    def call(p=None, h=None, **kw):
        a = _lib.UavEvalArgs()
        a.n, a.records = 64, rec.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        p = policy() if p is None else p
        return lib.uavenv_eval_episodes_scripted(env._h if h is None else h, C.byref(p), C.byref(a), env._stream())

    def act_call(p, out=None, h=None):
        return lib.uavenv_scripted_act(env._h if h is None else h, C.byref(p), acts.data_ptr() if out is None else out, env._stream())

    steer = policy(_lib.ACT_STEER_F32, 9)
    assert call() == 0 and call(steer) == 0 and call(eps=0.5) == 0 and act_call(policy()) == 0 and act_call(steer) == 0
    torch.cuda.synchronize()
    assert _state_bytes(env) == before and env.lib.uavenv_tick(env._h) == tick
    bad = [policy(_lib.ACT_STEER_F64, 9), policy(3), policy(-1), policy(candidates=3), policy(candidates=9),
           policy(_lib.ACT_STEER_F32, 0), policy(_lib.ACT_STEER_F32, 1), policy(_lib.ACT_STEER_F32, 4), policy(_lib.ACT_STEER_F32, 8),
           policy(_lib.ACT_STEER_F32, 19), policy(_lib.ACT_STEER_F32, -3), policy(lookahead=-1), policy(lookahead=17),
           policy(_lib.ACT_STEER_F32, 9, 17), policy(_lib.ACT_STEER_F32, 9, -1)]
    for p in bad:
        assert call(p) == _lib.EINVAL and act_call(p) == _lib.EINVAL
    assert lib.uavenv_eval_episodes_scripted(env._h, None, C.byref(_lib.UavEvalArgs()), env._stream()) == _lib.EINVAL
    assert lib.uavenv_scripted_act(env._h, None, acts.data_ptr(), env._stream()) == _lib.EINVAL
    assert act_call(policy(), out=acts.data_ptr() + 2) == _lib.EINVAL
    assert lib.uavenv_scripted_act(env._h, C.byref(policy()), None, env._stream()) == _lib.EINVAL
    assert call(steer, eps=0.5) == _lib.EINVAL and call(steer, eps=1.0) == _lib.EINVAL          # eps > 0 needs the index kind
    # everything the shared checks refuse
    assert call(n=0) == _lib.EINVAL and call(n=-5) == _lib.EINVAL and call(first=-1) == _lib.EINVAL
    assert call(traj_steps=5) == _lib.EINVAL and call(traj_steps=-1) == _lib.EINVAL
    tp = torch.zeros((64, 6, 3), dtype=torch.float64, device=DEV)
    ta = torch.zeros((64, 5), dtype=torch.float32, device=DEV)
    assert call(traj_steps=5, traj_pos=tp.data_ptr()) == _lib.EINVAL                               # only one of the two
    assert call(traj_steps=5, traj_act=ta.data_ptr()) == _lib.EINVAL
    assert call(traj_steps=5, traj_pos=tp.data_ptr() + 4, traj_act=ta.data_ptr()) == _lib.EINVAL   # misaligned arrays
    assert call(steer, traj_steps=5, traj_pos=tp.data_ptr(), traj_act=ta.data_ptr() + 2) == _lib.EINVAL
    assert call(traj_steps=5, traj_pos=tp.data_ptr(), traj_act=ta.data_ptr() + 1) == 0             # (int8 indices need no alignment)
    assert call(steer, traj_steps=5, traj_pos=tp.data_ptr(), traj_act=ta.data_ptr()) == 0
    assert call(records=rec.data_ptr() + 8) == _lib.EINVAL and call(records=None) == _lib.EINVAL
    v0 = torch.zeros((64, 2), dtype=torch.float64, device=DEV)
    assert call(v0=v0.data_ptr() + 4) == _lib.EINVAL
    sg = torch.zeros((4, 6), dtype=torch.float64, device=DEV)
    sub = torch.zeros((4, env.K, 3), dtype=torch.float64, device=DEV)
    ns = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert call(start_goal=sg.data_ptr(), m=4) == _lib.EINVAL                                      # only some of the three
    assert call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), m=4) == _lib.EINVAL
    assert call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), nsub=ns.data_ptr(), m=0) == _lib.EINVAL
    assert call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), nsub=ns.data_ptr() + 2, m=4) == _lib.EINVAL
    assert call(max_steps=-1) == _lib.EINVAL and call(max_workgroups=-1) == _lib.EINVAL
    assert call(n=2 ** 31 - 100) == _lib.EINVAL                                                    # n + lanes leaves the index range
    torch.cuda.synchronize()
    assert _state_bytes(env) == before and env.lib.uavenv_tick(env._h) == tick
    # no world: an env that never saw uavenv_set_buildings; no scenarios: an env without a bank
    h = C.c_void_p()
    _lib.check(lib.uavenv_create(C.byref(env.cfg), C.byref(h)), "uavenv_create")
    assert call(h=h) == _lib.EINVAL and act_call(policy(), h=h) == _lib.EINVAL
    lib.uavenv_destroy(h)
    env.close()
    from dqn_based_uav_3d_path_planer_amd.env import VecPathPlanEnv
    nob = VecPathPlanEnv(16, load_city26()["buildings"], obs_dtype="packed", uav_per_env=U, apf_enabled=apf)
    a = _lib.UavEvalArgs(); a.n, a.records = 64, rec.data_ptr()
    assert nob.lib.uavenv_eval_episodes_scripted(nob._h, C.byref(policy()), C.byref(a), nob._stream()) == _lib.EINVAL
    nob.close()
    # the index kind on an env with more than 32 actions
    many = VecPathPlanEnv(16, load_city26()["buildings"], obs_dtype="packed", n_actions=33)
    many.load_scenarios(*(load_city26()[k] for k in ("start_goal", "sub_goals", "n_sub")))
    out33 = torch.zeros(many.N, dtype=torch.int32, device=DEV)
    assert many.lib.uavenv_eval_episodes_scripted(many._h, C.byref(policy()), C.byref(a), many._stream()) == _lib.EINVAL
    assert many.lib.uavenv_scripted_act(many._h, C.byref(policy()), out33.data_ptr(), many._stream()) == _lib.EINVAL
    assert many.lib.uavenv_eval_episodes_scripted(many._h, C.byref(steer), C.byref(a), many._stream()) == 0    # the steer kind flies
    torch.cuda.synchronize()
    many.close()


def test_training_is_the_same_with_a_scripted_evaluation_in_between():
    from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
    from dqn_based_uav_3d_path_planer_amd.loop import HotLoop
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing

    def run(with_eval):
        env = make_city26_env(4096, obs_dtype="packed")
        ring = DeviceReplayRing(env, 1 << 16, discrete=True)
        ring.reset(seed=1000)
        torch.manual_seed(42)
        L = FusedDQNLearner(DQN_PARAM, "dqn", device=DEV)
        loop = HotLoop(ring, L, 1024, seed=7, eps=0.1)
        loop.run(12)
        if with_eval:
            for pol in POLICIES:
                assert ev.evaluate_scripted_policy(env, 2048, seed=5, max_steps=200, **_kw(pol)).summary()["episodes"] == 2048
            ev.scripted_act(env, torch.zeros(env.N, dtype=torch.int32, device=DEV))
        loop.run(12)
        torch.cuda.synchronize()
        out = (L.flat.cpu().numpy().tobytes(), ring.obs.cpu().numpy().tobytes(), ring.action.cpu().numpy().tobytes(),
               ring.reward.cpu().numpy().tobytes(), _state_bytes(env), env.lib.uavenv_tick(env._h))
        env.close()
        return out

    assert run(False) == run(True)


def test_the_apf_workspace_is_shared_with_the_net_entries():
    """The scripted entry flies APF episodes on the env-owned workspace of the slots / SAC entries: whichever grows it, a later call
    of the others still gives its own bytes."""
    from test_eval_sac_gpu import _sac
    env = _env(64, 1, 1)
    torch.manual_seed(3)
    L = FusedDQNLearner(DQN_PARAM, "dqn", device=DEV)
    S = _sac("init", 5)
    kw = dict(seed=3, max_steps=150)
    dqn = lambda: ev.evaluate_policy(env, [L], 512, max_workgroups=1, **kw).host_records().tobytes()          # noqa: E731
    sac = lambda: ev.evaluate_sac_policy(env, S, 512, max_workgroups=1, **kw).host_records().tobytes()        # noqa: E731
    scr = lambda n, mw: ev.evaluate_scripted_policy(env, n, max_workgroups=mw, **kw).host_records().tobytes()  # noqa: E731
    s_small = scr(512, 1)                          # the workspace is allocated by the scripted entry: 256 lanes
    d0, a0 = dqn(), sac()
    s_big = scr(4096, 0)                           # grown by the scripted entry
    assert dqn() == d0 and sac() == a0
    assert scr(512, 1) == s_small and scr(4096, 3) == s_big and s_big[:512 * 64] == s_small
    env.close()


def test_scripted_transitions_fill_a_replay_ring():
    """scripted_act's output goes straight into the step launch that writes the ring: the stored actions are its indices."""
    from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
    env = make_city26_env(256, obs_dtype="packed")
    ring = DeviceReplayRing(env, 8 * env.N, discrete=True)
    ring.reset(seed=2)
    for _ in range(4):
        frame = ring.head
        ev.scripted_act(env, ring.current_action(), action="index", lookahead=4)
        a = ring.current_action().clone()
        ring.step_env(auto_reset=True)
        assert torch.equal(ring.action[frame], a) and int(a.min()) >= 0 and int(a.max()) <= 2
    torch.cuda.synchronize()
    assert ring.filled == 4 and torch.isfinite(ring.reward[:4]).all()
    env.close()


# ---- 8. the plugin -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trainer,apf", [("DQN", 0), ("DuelingDQN", 1), ("SAC", 0), ("SAC", 1)])
def test_plugin_evaluate_baseline(trainer, apf, tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver
    monkeypatch.chdir(tmp_path)                    # (the config's paths are relative to the working directory)
    xml = driver.make_config_dir(str(tmp_path), trainer, num_envs=64, num_uav=4)
    if apf:
        uav_xml = tmp_path / "config" / "UAV.xml"
        uav_xml.write_text(re.sub(r"<APF_Enabled>0</APF_Enabled>", "<APF_Enabled>1</APF_Enabled>", uav_xml.read_text()))
    torch.manual_seed(0)
    env = driver.simulator(xml).env
    assert env.backend.cfg.apf_enabled == apf
    before = _state_bytes(env.backend)
    calls = []
    real = ev.evaluate_scripted_policy

    def counted(*a, **kw):
        res = real(*a, **kw)
        calls.append((a, kw, res))
        return res

    monkeypatch.setattr(ev, "evaluate_scripted_policy", counted)
    summ = env.evaluate_baseline(n_episodes=256, seed=1, max_steps=300, lookahead=4)
    monkeypatch.setattr(ev, "evaluate_scripted_policy", real)
    assert len(calls) == 1 and len(summ) == 4      # ONE launch for the four slots
    a, kw, res = calls[0]
    assert a[1] == 256 * 4 and kw["lookahead"] == 4
    assert kw["action"] == ("steer" if trainer == "SAC" else "index") and kw.get("candidates") == (9 if trainer == "SAC" else None)
    rec = res.host_records()
    # the missions and headings evaluate_policy(seed = 1) flies
    scn = ev.held_out_scenarios(env.backend, 256, seed=0x7E57_0000 + 1)
    scn_u, v0 = ev.slot_scenarios(scn, 4, float(env.backend.cfg.max_v), 1)
    learners = [u.Trainer.learner for u in env.Agents]
    if trainer == "SAC":
        pol = ev.evaluate_sac_policy(env.backend, learners, 256 * 4, scenarios=scn_u, v0=v0, seed=1, max_steps=300).host_records()
    else:
        pol = ev.evaluate_policy(env.backend, learners, 256 * 4, scenarios=scn_u, v0=v0, seed=1, max_steps=300).host_records()
    assert np.array_equal(rec["v0x"], pol["v0x"]) and np.array_equal(rec["v0y"], pol["v0y"])
    assert np.array_equal(rec["v0x"], v0.cpu().numpy()[:, 0]) and np.array_equal(rec["v0y"], v0.cpu().numpy()[:, 1])
    for x, y in zip(kw["scenarios"], scn_u):
        assert torch.equal(x, y)
    for j in range(4):
        assert summ[j] == ev.summarize(rec[j::4]), j
        assert summ[j]["episodes"] == 256 and summ[j]["invalid"] == 0
    assert len({s["mean_energy"] for s in summ}) == 4 and len({s["success"] for s in summ}) == 1
    # the trained policies' own evaluation still returns what it did
    assert env.evaluate_policy(n_episodes=256, seed=1, max_steps=300) == [ev.summarize(pol[j::4]) for j in range(4)]
    with pytest.raises(ValueError):
        env.evaluate_baseline(n_episodes=64, lookahead=17)
    with pytest.raises(ValueError):
        env.evaluate_baseline(n_episodes=0)
    torch.cuda.synchronize()
    assert _state_bytes(env.backend) == before
