"""Every device text of the step transition against the oracle with the termination cascade ON its thresholds (MI355X).

The catalogue of tests/cascade_edges.py (2 399 pre-step states: d_sub, d_goal and dist(sub0, goal) on 7.0, on each other
and on the neighbouring doubles, crossed with the Step limit, every list length, the reset alias and a collision) is
injected with set_state, read back bit for bit, and stepped twice through

  k_step_coop                 env.step below 49 152 agents, uav_per_env 1 and 4; f32, f16 and packed rows
  k_step, 64 threads          one_wave=True; and the default launch of 49 152 + 64 * 3 + 9 agents
  k_step, 256 threads         the catalogue tiled to 131 072 + 64 * 3 + 9 agents
  k_step_coop<POLICY>         uavenv_step_policy on packed rows, with and without the layer-1 image (step_pre split in two
                              around the staging barrier); a net whose fc2 is all bias picks the middle action, steer 0;
                              both instantiations: up to 256 workgroups, and 16 384 + 64 * 3 + 10 agents
  k_step_polh                 the same on the f16 ring
  the APF forms               apf_enabled = 1 with every building at rest (the force is zero, the thresholds stay put):
                              adjust_subgoals_lane in k_step_coop and in k_step, and k_apf_adjust + adjust_subgoals_split

Expected values are oracle/uav_oracle.c's, which tests/test_cascade_edges.py pins to the executed reference on this very
catalogue.  ret_done, agent_done, info, Step, n_sub, reach and the alias flag are exact; position, goal and the sub-goal
list after each step are bit-equal (they are copies and exact moves: a case whose position differed would be a fault of
the catalogue, and fails); reward within REWARD_TOL = 1e-9 (cos_between against the atan2 chain), reward32 within one
f32 ulp, score / total / path length within 1e-8.  No case is skipped or masked out of that comparison.  (The APF
forms are held to the APF-off expectation as well; there alone the second step of six cases per group is left out: an alias
that outlives a time-out without collision is still there at the second step of the APF-off run and gone from the APF-on
one, in the executed reference too, as tests/test_cascade_edges.py pins.)  The policy launches take the cases
whose action is 0 (all of group v1, 6 of 10 in the max_v = 0 groups; the counts and the presence of every family and side
are asserted).

Cases per family (groups v0 + v1 + v0k3): dsub7 683, clause2 412, dgoal7 739, both 180, nothing_left 25, listlen 144,
alias 126, seq 90.

Cases that reject each mutation of the host model (asserted per family in tests/test_cascade_edges.py):

  d_sub <= 7                                           169     d_goal <= dist(sub0, goal)                          202
  d_goal <= 7                                          193     d_sub < nextafter(7, 0)                              30
  d_sub < nextafter(7, inf)                            169     d_goal < nextafter(7, 0)                             21
  d_goal < nextafter(7, inf)                           193     Step > max_step                                     427
  time-out tested after the pop                        240     goal arm before the pop arm                         156
  last pop without its +50                             377     Step not zeroed on a pop                            478
  window reloaded from sub_idx                         212     alias survives a collision                           48
  thresholds at the moved position after a collision   288

The whole-episode entries (eval_step) fly cascade_edges.episode_rows: from V_vector (1, 0) under steer 0 the UAV is at
start + (t, 0, 0) after t steps (asserted from the trajectory, bit for bit), and a threshold straight above the lane is met
at a chosen step with the neighbouring doubles of 7 -- goal within 7, last pop, a pop and on, d_goal against
dist(sub0, goal), time-out at max_step, nothing left.  The records are held to an oracle rollout of the same rows.  DQN
f32 / f16 / slots with the all-bias net, SAC with a zero actor head (mean mode); the scripted policy flies the rows whose
current sub-goal is never behind the UAV (its pursuit steer is then exactly 0): 26 of the 44.

What this module found: with APF on, an agent whose sub_goals[0] was still the position object and whose first step
collided had the STORED list entry (the start point) adjusted, where the reference's list holds the moved-to point;
adjust_subgoals_lane and adjust_subgoals_split now take the window's value (the three APF tests of group v1 failed on
the twelve alias-and-collision cases at the Step limit, and on the reward of the others, until then).

Measured on an MI355X: the module's 46 tests take 2.8 s; the slowest is test_cooperative_kernel[v0-f32] at 0.4 s (it also
builds the catalogue and the oracle's outputs, once for the module), the three large launches take 0.1 to 0.3 s each.  The
whole-episode returns differ from the oracle's by exactly 0 on every entry (heading 0: the reward's cosine terms are exact).

One mutation trial (not committed): with `d_sub <= 7.0` built into the APF instantiations of step_post_b alone, the nine
test_apf_forms_with_buildings_at_rest cases failed (every group, every form) and the other 34 tests of the module passed.
"""
import numpy as np
import pytest
import torch

import cascade_edges as ce
from conftest import load_golden

pytestmark = pytest.mark.gpu

REWARD_TOL = ce.REWARD_TOL             # as tests/test_env_parity_gpu.py
STATE_TOL = 1e-9
FMT = {"f32": torch.float32, "f16": torch.float16, "packed": "packed"}
PARAM = {"w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99", "Update_loop": "3"}
bits_of = ce.bits_of

_CACHE = {}


def _expected():
    """The catalogue and the oracle's two steps of it, APF off and APF on over buildings at rest.  Built once."""
    if not _CACHE:
        from oracle import pyoracle as po
        w = load_golden("world_stock.npz")
        cat = ce.build(w["buildings"])
        world = po.OracleWorld(w["buildings"])
        _CACHE.update(b=w["buildings"], cat=cat, off={g: ce.run_oracle(grp, world) for g, grp in cat.items()},
                      on={g: ce.run_oracle(grp, world, apf=1) for g, grp in cat.items()})
    return _CACHE


@pytest.fixture(scope="module")
def expected():
    yield _expected()
    _CACHE.clear()


def make_env(exp, grp, n, fmt="f32", **kw):
    from dqn_based_uav_3d_path_planer_amd.env import VecPathPlanEnv
    return VecPathPlanEnv(n, exp["b"], max_v=grp.max_v, max_subgoals=grp.K, max_step=ce.MAX_STEP, steering_angle=ce.STEER,
                          obs_dtype=FMT[fmt], **kw)


def inject(env, grp, idx):
    """set_state, and the pre-step state the device reports back: the injected one, bit for bit."""
    env.set_state(0, grp.kin[idx], grp.step0[idx], grp.n_sub[idx], grp.sub[idx], alias=grp.alias[idx])
    st, sub, alias = env.get_state(0, len(idx), want_sub=True)
    assert np.array_equal(bits_of(st), bits_of(grp.state16()[idx])), "pre-step state is not the one the oracle stepped"
    assert np.array_equal(bits_of(sub), bits_of(grp.sub[idx])) and np.array_equal(alias, grp.alias[idx])


def _f32_ulp_ok(got32, want64):
    want32 = want64.astype(np.float32)
    return np.abs(got32.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64)


def _first_bad(grp, idx, bad):
    k = np.nonzero(bad)[0]
    return [(grp.name, int(idx[i]), str(grp.family[idx[i]]), grp.tag[idx[i]]) for i in k[:4]], len(k)


def check_step(env, grp, want, idx, t, *, reward=None, reward32=None, ret_done=None, agent_done=None, info=None, ints_of=None):
    """The outputs of step t (0 or 1) of agents that carry cases idx, and the state after it, against `want`.
    ints_of: a second expectation whose integers and lists must hold as well (the APF-off run under the APF forms)."""
    n = len(idx)
    st, sub, alias = env.get_state(0, n, want_sub=True)
    ws = want["state"][idx, t]
    for name, got, exp in (("ret_done", ret_done, want["ret_done"][idx, t]), ("info", info, want["info"][idx, t]),
                           ("agent_done", agent_done, ws[:, 10])):
        if got is not None:
            bad = got.cpu().numpy() != exp.astype(np.uint8)
            assert not bad.any(), (name, t, _first_bad(grp, idx, bad))
    for name, cols in (("Step", 9), ("done", 10), ("n_sub", 11), ("reach", 15)):
        bad = st[:, cols] != ws[:, cols]
        assert not bad.any(), (name, t, _first_bad(grp, idx, bad))
    assert np.array_equal(alias, want["alias"][idx, t]), ("alias", t)
    bad = (bits_of(st[:, 0:3]) != bits_of(ws[:, 0:3])).any(axis=1)
    assert not bad.any(), ("catalogue fault: the position after the move is not the oracle's", t, _first_bad(grp, idx, bad))
    assert np.array_equal(bits_of(st[:, 6:9]), bits_of(ws[:, 6:9])), ("goal", t)
    bad = (bits_of(sub) != bits_of(want["sub"][idx, t])).any(axis=(1, 2))
    assert not bad.any(), ("sub-goal list", t, _first_bad(grp, idx, bad))
    assert np.abs(st[:, 3:6] - ws[:, 3:6]).max() <= STATE_TOL, t
    assert np.abs(st[:, 12:15] - ws[:, 12:15]).max() <= 1e-8, t
    if reward is not None:
        err = np.abs(reward.cpu().numpy() - want["reward"][idx, t])
        assert err.max() <= REWARD_TOL, ("reward", t, err.max(), _first_bad(grp, idx, err > REWARD_TOL))
    if reward32 is not None:
        ok = _f32_ulp_ok(reward32.cpu().numpy(), want["reward"][idx, t])
        assert ok.all(), ("reward32", t, _first_bad(grp, idx, ~ok))
    if ints_of is not None:
        # (an alias that outlived the first step of the APF-off run -- a time-out without collision -- moves sub0 along at its
        # second step; under APF it is gone by then, in the reference too: those six second steps are not comparable)
        m = np.ones(n, dtype=bool) if t == 0 else ints_of["alias"][idx, 0] == 0
        os_ = ints_of["state"][idx, t]
        assert np.array_equal(st[m][:, ce.INT_COLS], os_[m][:, ce.INT_COLS])
        assert np.array_equal(bits_of(sub[m]), bits_of(ints_of["sub"][idx, t][m]))
        assert np.array_equal(bits_of(st[m, 0:3]), bits_of(os_[m, 0:3]))
        for got, key in ((ret_done, "ret_done"), (info, "info")):
            assert np.array_equal(got.cpu().numpy()[m], ints_of[key][idx, t][m].astype(np.uint8)), key


def run_steps(env, grp, want, idx, ints_of=None, **step_kw):
    """Inject, then both steps through env.step, each held to `want`."""
    inject(env, grp, idx)
    a = torch.tensor(grp.action[idx], dtype=torch.float64, device="cuda")
    out = env.alloc_out()
    for t in range(ce.STEPS):
        env.step(a, out, **step_kw)
        torch.cuda.synchronize()
        assert (out.valid == 1).all()
        check_step(env, grp, want, idx, t, reward=out.reward, reward32=out.reward32, ret_done=out.ret_done,
                   agent_done=out.agent_done, info=out.info, ints_of=ints_of)
    return out


GROUPS = list(ce.GROUPS)


# ------------------------------------------------------------------------------------------------- env.step, APF off
@pytest.mark.parametrize("fmt", ["f32", "f16", "packed"])
@pytest.mark.parametrize("group", GROUPS)
def test_cooperative_kernel(expected, group, fmt):
    """k_step_coop: one agent per case (a ragged last wavefront in every group), every row format."""
    grp = expected["cat"][group]
    assert grp.n % 64 != 0 and grp.n <= 49152
    env = make_env(expected, grp, grp.n, fmt)
    run_steps(env, grp, expected["off"][group], np.arange(grp.n))
    env.close()


@pytest.mark.parametrize("group,fmt", [("v0", "packed"), ("v1", "f32"), ("v0k3", "f16")])
def test_cooperative_kernel_four_uavs_per_env(expected, group, fmt):
    """k_step_coop with uav_per_env = 4 (the team's flags in LDS beside the transition): the catalogue tiled to whole envs."""
    grp = expected["cat"][group]
    n_env = (grp.n + 3) // 4 + 1
    env = make_env(expected, grp, n_env, fmt, uav_per_env=4)
    assert env.N == 4 * n_env
    run_steps(env, grp, expected["off"][group], np.arange(env.N) % grp.n)
    env.close()


@pytest.mark.parametrize("group,fmt", [("v0", "f32"), ("v1", "packed"), ("v1", "f16"), ("v0k3", "f32")])
def test_single_wave_workgroups(expected, group, fmt):
    """k_step at 64 threads per workgroup (one_wave)."""
    grp = expected["cat"][group]
    env = make_env(expected, grp, grp.n, fmt)
    run_steps(env, grp, expected["off"][group], np.arange(grp.n), one_wave=True)
    env.close()


@pytest.mark.parametrize("group,fmt,n", [("v1", "f32", 49152 + 64 * 3 + 9), ("v0", "f32", 131072 + 64 * 3 + 9),
                                         ("v1", "packed", 131072 + 64 * 3 + 9)])
def test_large_launches(expected, group, fmt, n):
    """Above the cooperative kernel's 49 152-agent limit: k_step in single-wavefront workgroups up to 131 072 agents, in
    256-thread workgroups beyond -- the catalogue tiled, plus 64 * 3 + 9 ragged agents."""
    grp = expected["cat"][group]
    env = make_env(expected, grp, n, fmt)
    run_steps(env, grp, expected["off"][group], np.arange(n) % grp.n)
    env.close()


# ------------------------------------------------------------------------------------------------- the APF forms
@pytest.mark.parametrize("form", ["lane-coop", "lane-wave", "split"])
@pytest.mark.parametrize("group", GROUPS)
def test_apf_forms_with_buildings_at_rest(expected, group, form):
    """apf_enabled = 1, every building velocity 0: cal_force skips every building, so no sub-goal moves and the thresholds stay
    where the catalogue put them.  Adjust_subgoal still rebuilds the list, which ends the alias (the oracle with apf_enabled = 1
    has it so).  lane-coop: adjust_subgoals_lane in k_step_coop; lane-wave: the same in k_step; split: k_apf_adjust in front of
    k_step + adjust_subgoals_split.  Integers, positions and lists must equal the APF-off run as well."""
    grp = expected["cat"][group]
    kw = {"lane-coop": dict(apf_lane=True), "lane-wave": dict(apf_lane=True, one_wave=True), "split": dict()}[form]
    env = make_env(expected, grp, grp.n, "f32", apf_enabled=1)
    run_steps(env, grp, expected["on"][group], np.arange(grp.n), ints_of=expected["off"][group], **kw)
    env.close()


def test_apf_oracle_differs_from_the_plain_one_only_in_the_alias(expected):
    """Host arithmetic only: what the APF forms above are held to is the APF-off expectation with the alias ended (but for the
    second step of the six cases per group whose alias outlives the first)."""
    for g, grp in expected["cat"].items():
        on, off = expected["on"][g], expected["off"][g]
        kept = off["alias"][:, 0] == 1
        assert kept.sum() == 6 and not on["alias"].any()
        for key in ("reward", "ret_done", "info", "state", "sub"):
            assert np.array_equal(on[key][:, 0], off[key][:, 0]) and np.array_equal(on[key][~kept], off[key][~kept]), key


# ------------------------------------------------------------------------------------------------- the policy launches
def _straight_learner(mfma=None):
    """fc2 is all bias, and the bias picks the middle action: steer exactly 0, whatever the row holds."""
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    torch.manual_seed(3)
    L = FusedDQNLearner(dict(PARAM, NetWork="Qnet2"), "dqn", device="cuda:0", **({} if mfma is None else dict(mfma=mfma)))
    with torch.no_grad():
        L.q_local.fc2.weight.zero_()
        L.q_local.fc2.bias.copy_(torch.tensor([0.0, 5.0, 0.0], device="cuda:0"))
    return L


def _policy_subset(grp):
    """The cases a policy launch can fly (action 0), with the count of those it cannot; every family and every side of
    every threshold is still there."""
    sel = np.nonzero(grp.action == 0.0)[0]
    left_out = grp.n - len(sel)
    assert left_out == {"v0": 467, "v1": 0, "v0k3": 91}[grp.name], left_out
    assert set(grp.family[sel]) == set(ce.FAMILIES)
    for fam, col in (("dsub7", 0), ("clause2", 1), ("dgoal7", 2)):
        m = grp.family[sel] == fam
        for hit in ((False, True) if grp.name != "v0k3" else (False,)):
            assert set(grp.side[sel][m & (grp.collide[sel] == hit), col]) == {-1, 0, 1}, (fam, hit)
    return sel


def _policy_launch(expected, group, form, n=None):
    """Both steps of the policy subset of a group through uavenv_step_policy, tiled to n agents (default: the subset itself)."""
    from dqn_based_uav_3d_path_planer_amd import _lib
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
    grp, want = expected["cat"][group], expected["off"][group]
    sel = _policy_subset(grp)
    n = len(sel) + (len(sel) & 1) if n is None else n                 # k_step_polh takes an even agent count
    idx = sel[np.arange(n) % len(sel)]
    polh = form == "polh"
    env = make_env(expected, grp, n, "f16" if polh else "packed")
    ring = DeviceReplayRing(env, 4 * n, discrete=True)
    L = _straight_learner("f16" if polh else None)
    if polh:
        ring.extra_flags = _lib.STEP_ONE_WAVE
    image = L.split_image() if form == "coop-image" else None
    inject(env, grp, idx)
    env.observe(ring.obs[ring.head])
    ad = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for t in range(ce.STEPS):
        frame = ring.head
        assert ring.step_policy(L, 0.0, 29, t, auto_reset=False, skip_done=False, image=image, agent_done=ad)
        torch.cuda.synchronize()
        assert (ring.action[frame] == 1).all() and (ring.valid[frame] == 1).all()
        check_step(env, grp, want, idx, t, reward32=ring.reward[frame], ret_done=ring.done[frame], agent_done=ad)
    env.close()


@pytest.mark.parametrize("form", ["coop", "coop-image", "polh"])
@pytest.mark.parametrize("group", GROUPS)
def test_policy_launches(expected, group, form):
    """uavenv_step_policy, eps = 0: k_step_coop<POLICY> on packed rows without and with the layer-1 image, k_step_polh on f16
    rows.  The launch writes the f32 reward, ret_done and agent_done; the rest is read from the state.  (At most 16
    workgroups: the instantiations for up to 256 of them.)"""
    _policy_launch(expected, group, form)


@pytest.mark.parametrize("group,form", [("v1", "coop"), ("v1", "coop-image"), ("v0", "coop-image")])
def test_policy_launches_beyond_256_workgroups(expected, group, form):
    """k_step_coop<POLICY> above 16 384 agents takes its other instantiation (two or three workgroups share a CU): the subset
    tiled to 16 384 + 64 * 3 + 10 agents, a ragged last workgroup."""
    n = 16384 + 64 * 3 + 10
    assert (n + 63) // 64 > 256 and n <= 49152
    _policy_launch(expected, group, form, n)


# ------------------------------------------------------------------------------------------------- whole episodes
SAC_PARAM = {"actor": {"NetWork": "PolicyNetContinuous_SAC", "w": "100", "action_bound": "1", "hiden_dim": "64", "output": "2", "lr": "0.0001"},
             "critic": {"NetWork": "QValueNetContinuous_SAC", "w": "100", "hiden_dim": "64", "action_dim": "2", "lr": "0.001"},
             "SAC_param": {"IS_Continuous": "1", "alpha_lr": "0.0001", "target_entropy": "1", "gamma": "0.99", "tau": "0.05"}}
EP_PARAMS = dict(max_v=1.0, steering_angle=ce.STEER, max_step=ce.MAX_STEP, apf_enabled=0)


def _episodes(exp):
    if "ep" not in exp:
        from oracle import pyoracle as po
        sg, sub, ns, tags, straight = ce.episode_rows(exp["b"])
        want = ce.oracle_episodes(po.OracleWorld(exp["b"]), sg, sub, ns, EP_PARAMS)
        # the oracle alone shows every ending, on either side of each threshold
        t = np.array(tags)
        for T in (1, 6, 41):
            for what in ("goal within", "last pop"):
                m = np.array([x.startswith(what) and x.endswith("step %d" % T) for x in tags])
                assert list(want["outcome"][m]) == [1, 2, 2] and list(want["steps"][m]) == [T, 150, 150], (what, T)
            m = np.array([x.startswith("pop,") and " step %d," % max(T, 2) in x for x in tags])
            # (popped at the threshold, or some steps later by the second clause: the same length, returns 6.66 apart)
            assert (want["steps"][m] == max(T, 2) + 24).all() and (want["ret"][m][0] - want["ret"][m][1:] > 6.0).all()
            m = np.array([x.startswith("d_goal against") and " step %d," % T in x for x in tags])
            assert list(want["steps"][m]) == [T, T, T + 1, T + 1, T + 1] and (want["outcome"][m] == 1).all()
        assert want["steps"][0] == 1 and want["ret"][0] == 150.0 and want["outcome"][1] == 2 and want["steps"][1] == 150
        assert straight.sum() == 26 and len(t) == 44
        exp["ep"] = (sg, sub, ns, tags, straight, want)
    return exp["ep"]


@pytest.mark.parametrize("entry", ["dqn", "dqn-f16", "slots", "sac", "scripted"])
def test_whole_episode_entries(expected, entry):
    """eval_step inside uavenv_eval_episodes, _f16, _slots, _sac and _scripted on the episode rows: outcome, steps, reach,
    sub-goals popped and collisions exact; the return within REWARD_TOL (as tests/test_eval_gpu.py holds it), path
    length and total score within 1e-8; every position of the trajectory bit-equal to start + (t, 0, 0)."""
    from dqn_based_uav_3d_path_planer_amd import _lib, evaluate as ev
    from dqn_based_uav_3d_path_planer_amd.env import VecPathPlanEnv
    sg, sub, ns, tags, straight, want = _episodes(expected)
    rows = np.nonzero(straight)[0] if entry == "scripted" else np.arange(len(sg))
    n, T = len(rows), 152
    env = VecPathPlanEnv(64, expected["b"], max_v=1.0, max_subgoals=ce.EP_K, max_step=ce.MAX_STEP, steering_angle=ce.STEER,
                         obs_dtype=torch.float16 if entry == "dqn-f16" else "packed")
    scn = tuple(torch.tensor(a[rows], device="cuda") for a in (sg, sub, ns))
    kw = dict(scenarios=scn, v0=np.tile([1.0, 0.0], (n, 1)), trajectory_steps=T)
    if entry == "sac":
        from dqn_based_uav_3d_path_planer_amd.sac import FusedSACLearner
        torch.manual_seed(5)
        L = FusedSACLearner(SAC_PARAM, "cuda:0")
        with torch.no_grad():
            L.actor.fc_mu.weight.zero_()
            L.actor.fc_mu.bias.zero_()
        res = ev.evaluate_sac_policy(env, L, n, mode="mean", **kw)
    elif entry == "scripted":
        res = ev.evaluate_scripted_policy(env, n, action="index", **kw)
    else:
        L = _straight_learner("f16" if entry == "dqn-f16" else None)
        res = ev.evaluate_policy(env, [L] if entry == "slots" else L, n, **kw)
    rec = res.host_records()
    torch.cuda.synchronize()
    steps = want["steps"][rows]
    act = res.actions.cpu().numpy()
    pos = res.positions.cpu().numpy()
    for i in range(n):
        k = int(steps[i])
        a = act[i, :k, 0] if entry == "sac" else act[i, :k]
        assert (a == (0.0 if entry == "sac" else 1)).all(), (tags[rows[i]], "the policy did not fly straight")
        moved = k if ns[rows[i]] > 0 else 0                                      # (nothing left: nothing moves)
        exp_pos = np.c_[ce.EP_START[0] + np.arange(1, k + 1.0) * (moved > 0), np.full(k, ce.EP_START[1]), np.full(k, ce.EP_START[2])]
        assert np.array_equal(bits_of(pos[i, 1:k + 1]), bits_of(exp_pos)), tags[rows[i]]
    code = {1: _lib.EVAL_SUCCESS, 2: _lib.EVAL_LOSE}
    bad = rec["outcome"] != np.array([code[int(o)] for o in want["outcome"][rows]])
    assert not bad.any(), [tags[r] for r in rows[bad]]
    bad = rec["steps"] != steps
    assert not bad.any(), [(tags[r], int(s)) for r, s in zip(rows[bad], rec["steps"][bad])]
    assert np.array_equal(rec["reach_goal"], want["reach"][rows]) and np.array_equal(rec["subgoals"], want["popped"][rows])
    assert (rec["collisions"] == 0).all()
    err = np.abs(rec["ret"] - want["ret"][rows])
    print("whole episodes, %s: max |return - oracle| %.3g over up to %d steps" % (entry, err.max(), steps.max()))
    assert err.max() <= REWARD_TOL, (err.max(), [tags[r] for r in rows[err > REWARD_TOL]])
    assert np.abs(rec["path_len"] - want["path_len"][rows]).max() <= 1e-8
    assert np.abs(rec["total_score"] - want["total_score"][rows]).max() <= 1e-8
    env.close()
