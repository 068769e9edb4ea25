"""The termination cascade of update_PathPlan at every threshold -- host only.

Three things are held on the catalogue of tests/cascade_edges.py (2 399 pre-step states in three env configurations, every
one stepped twice), before tests/test_cascade_edges_gpu.py holds the device texts to the oracle on it:

  the oracle against the executed reference   tests/golden/cascade_edges.npz (oracle/gen_golden.py: gen_cascade_edges ran the
      same catalogue through Agents/UAV.py, APF off and APF on over buildings at rest): reward to 1e-12, Step / done / n_sub /
      reach / ret_done / info / alias exactly, positions, goals and sub-goal lists bit for bit.  The oracle needed no
      change: it agrees everywhere (the rewards are bit-equal too).
  the host model against the oracle           cascade_edges.model_step, unmutated: the same bars.
  the catalogue against mutations             each mutation of cascade_edges.MUTATIONS changes an integer output, a list entry
      or a reward by more than REWARD_TOL on the cases counted below, per threshold family; the counts are asserted, so a
      thinned catalogue does not pass silently.

Cases that reject each mutation (all three groups, either step), as asserted by test_catalogue_rejects_the_mutation:

  d_sub <= 7                                           169     d_goal <= dist(sub0, goal)                          202
  d_goal <= 7                                          193     d_sub < nextafter(7, 0)                              30
  d_sub < nextafter(7, inf)                            169     d_goal < nextafter(7, 0)                             21
  d_goal < nextafter(7, inf)                           193     Step > max_step                                     427
  time-out tested after the pop                        240     goal arm before the pop arm                         156
  last pop without its +50                             377     Step not zeroed on a pop                            478
  window reloaded from sub_idx                         212     alias survives a collision                           48
  thresholds at the moved position after a collision   288

(REJECTS has them per family.  A window reloaded from the wrong list index shows only after a second pop: family "seq", and
the cases of the other families whose second step pops again.)

The module takes about 4 s.
"""
import functools

import numpy as np
import pytest

import cascade_edges as ce
from conftest import load_golden


@functools.lru_cache(maxsize=None)
def _setup():
    from oracle import pyoracle as po
    w = load_golden("world_stock.npz")
    assert float(w["len"]) == ce.W and float(w["width"]) == ce.W and float(w["h"]) == ce.HBOX and int(w["max_step"]) == ce.MAX_STEP
    assert float(w["steering_angle"]) == ce.STEER
    cat = ce.build(w["buildings"])
    world = po.OracleWorld(w["buildings"])
    oracle = {g: ce.run_oracle(grp, world) for g, grp in cat.items()}
    return w["buildings"], cat, oracle


@pytest.fixture(scope="module", params=list(ce.GROUPS))
def group(request):
    b, cat, oracle = _setup()
    return b, cat[request.param], oracle[request.param]


def _assert_equal_outputs(got, want, reward_tol, what):
    assert np.abs(got["reward"] - want["reward"]).max() <= reward_tol, what
    for key in ("ret_done", "info", "alias"):
        assert np.array_equal(got[key], want[key]), (what, key)
    assert np.array_equal(got["state"][:, :, ce.INT_COLS], want["state"][:, :, ce.INT_COLS]), what      # Step, done, n_sub, reach
    for cols in (slice(0, 3), slice(6, 9)):                                                             # position, goal
        assert np.array_equal(ce.bits_of(got["state"][:, :, cols]), ce.bits_of(want["state"][:, :, cols])), what
    assert np.array_equal(ce.bits_of(got["sub"]), ce.bits_of(want["sub"])), what
    assert np.abs(got["state"][:, :, 3:6] - want["state"][:, :, 3:6]).max() <= 1e-12, what              # V_vector, V
    assert np.abs(got["state"][:, :, 12:15] - want["state"][:, :, 12:15]).max() <= 1e-9, what           # score, total, path length


def test_golden_is_this_catalogue(group):
    """The committed golden was generated from the catalogue as it is now."""
    _, grp, _ = group
    g = load_golden("cascade_edges.npz")
    for key, a in (("kin", grp.kin), ("step0", grp.step0), ("n_sub", grp.n_sub), ("sub_goals", grp.sub), ("alias0", grp.alias),
                   ("actions", grp.action)):
        got = g[grp.name + "_" + key]
        assert got.shape == a.shape and np.array_equal(got, a), key


def test_oracle_reproduces_the_reference_at_every_threshold(group):
    _, grp, oracle = group
    g = load_golden("cascade_edges.npz")
    want = {k: g["%s_out_%s" % (grp.name, k)] for k in oracle}
    _assert_equal_outputs(oracle, want, 1e-12, "oracle against the executed reference, group " + grp.name)
    assert want["alias"][:, 0].sum() == 0 or grp.alias.any()


def test_apf_oracle_reproduces_the_reference_with_buildings_at_rest(group):
    """The same catalogue with APF_Enabled = 1 and every building velocity 0 (the second half of the golden): the force is zero,
    so rewards, integers and lists are those of the APF-off run (but for six second steps) -- where sub_goals[0] was the position object and the step
    collided, the list keeps the moved-to point -- and Adjust_subgoal ends the alias on every step that gets that far."""
    from oracle import pyoracle as po
    b, grp, oracle = group
    g = load_golden("cascade_edges.npz")
    got = ce.run_oracle(grp, po.OracleWorld(b), apf=1)
    want = {k: g["%s_apf_out_%s" % (grp.name, k)] for k in got}
    _assert_equal_outputs(got, want, 1e-12, "oracle against the executed reference, APF on, group " + grp.name)
    # (an alias that outlives the first step -- a time-out without collision -- is still there at the second step of the APF-off
    # run, and gone from the APF-on one: those second steps differ, in the reference as in the oracle)
    kept = g["%s_out_alias" % grp.name][:, 0] == 1
    assert kept.sum() == {"v0": 6, "v1": 6, "v0k3": 6}[grp.name]
    for key in ("reward", "ret_done", "info", "state", "sub"):
        off = g["%s_out_%s" % (grp.name, key)]
        assert np.array_equal(want[key][:, 0], off[:, 0]) and np.array_equal(want[key][~kept], off[~kept]), key
    assert not want["alias"].any()


def test_distances_of_the_catalogue_are_the_oracles(group):
    """The catalogue places its thresholds with sqrt(dx*dx + dy*dy + dz*dz); the oracle (and the reference) square with pow.
    On every pair of points the cascade compares, the two give the same double."""
    from oracle import pyoracle as po
    _, grp, _ = group
    lib = po.lib()
    P = grp.state16()[:, 0:3]
    P = P + np.c_[np.where(grp.collide | (grp.n_sub == 0), 0.0, grp.max_v), np.zeros(grp.n), np.zeros(grp.n)]
    for i in range(grp.n):
        if grp.n_sub[i] == 0 or grp.alias[i]:
            continue
        p, s0, goal = tuple(P[i]), tuple(grp.sub[i, 0]), tuple(grp.kin[i, 5:8])
        for a, b in ((p, s0), (p, goal), (s0, goal)):
            assert ce.dist(a, b) == lib.orc_distance(*a, *b)
        assert ce.sides(p, s0, goal) == tuple(grp.side[i])


def test_model_equals_the_oracle(group):
    b, grp, oracle = group
    got, arms = ce.run_model(grp, b)
    _assert_equal_outputs(got, oracle, 1e-12, "host model against the oracle, group " + grp.name)
    assert not ce.differs(got, oracle).any()
    for t in range(ce.STEPS):
        assert np.array_equal(arms[:, t], ce.arm_of(oracle, grp.n_sub, t))


# family -> side of its own threshold -> the arms the first step must take there, away from the Step limit and with a
# sub-goal left (side: -1 below, 0 on, +1 above the threshold)
ARMS_BY_SIDE = {
    "dsub7": (0, {-1: {"pop", "last_pop"}, 0: {"plain"}, 1: {"plain"}}),
    "clause2": (1, {-1: {"pop", "last_pop"}, 0: {"plain"}, 1: {"plain"}}),
    "dgoal7": (2, {-1: {"goal"}, 0: {"plain"}, 1: {"plain"}}),
}


def test_every_arm_on_each_side_of_each_threshold():
    """From the oracle's outputs: on each side of each threshold the cascade takes the arms it must and no other, in every
    group, with and without a collision; at the Step limit every side times out; all six arms occur at every n_sub asked for."""
    _, cat, oracle = _setup()
    seen = set()
    for name, grp in cat.items():
        arms = ce.arm_of(oracle[name], grp.n_sub, 0)
        step1 = grp.step0 + 1
        for fam, (col, by_side) in ARMS_BY_SIDE.items():
            sel = grp.family == fam
            for hit in (False, True):
                for side, want in by_side.items():
                    m = sel & (grp.side[:, col] == side) & (step1 < ce.MAX_STEP) & (grp.collide == hit)
                    if name == "v0k3" and hit:
                        assert not m.any()
                        continue
                    assert m.any(), (name, fam, side, hit)
                    got = set(arms[m])
                    last = grp.n_sub[m] == 1
                    want_here = {a for a in want if a != "last_pop" or last.any()} - ({"pop"} if last.all() else set())
                    assert got == want_here, (name, fam, side, hit, got)
                    # the other two comparisons sit on the side that leaves this one to decide
                    for other in range(3):
                        assert other == col or (grp.side[m][:, other] >= 0).all(), (name, fam, other)
            if name != "v0k3":
                for step0 in (ce.MAX_STEP - 1, ce.MAX_STEP):
                    for side in (-1, 0, 1):
                        m = sel & (grp.side[:, col] == side) & (grp.step0 == step0)
                        assert m.any() and set(arms[m]) == {"timeout"}, (name, fam, side, step0)
                m = sel & (grp.step0 == ce.MAX_STEP - 2)
                assert m.any() and "timeout" not in set(arms[m]) and len(set(arms[m])) >= 2
        seen |= set(arms)
        o = oracle[name]
        for t in range(ce.STEPS):                  # nothing left: max_step - Step is paid, and nothing else moves
            m = ce.arm_of(o, grp.n_sub, t) == "nothing_left"
            pre = grp.state16() if t == 0 else o["state"][:, 0]
            assert np.array_equal(o["reward"][m, t], ce.MAX_STEP - pre[m, 9])
            assert np.array_equal(ce.bits_of(o["state"][m, t, 0:10]), ce.bits_of(pre[m, 0:10]))
        K = grp.K
        pops = np.isin(arms, ("pop", "last_pop"))
        for n in sorted({1, 2, 3, K - 1, K}):
            assert (pops & (grp.n_sub == n)).any(), (name, n)
        assert (grp.n_sub == 0).any() and ((grp.n_sub == 0) & (grp.step0 == 0)).any() and ((grp.n_sub == 0) & (grp.step0 == ce.MAX_STEP)).any()
        for n in (1, 2, 3):
            a = (grp.alias == 1) & (grp.n_sub == n)
            assert (a & ~grp.collide & (step1 < ce.MAX_STEP)).any() and np.isin(arms[a & (step1 < ce.MAX_STEP)], ("pop", "last_pop")).all()
            if name != "v0k3":
                assert (a & grp.collide).any()
        # two pops in a row: Step is back at 0 after each, and the second pop brings up list entry 2
        two = (grp.family == "seq") & (arms == "pop") & (ce.arm_of(o, grp.n_sub, 1) == "pop")
        assert two.sum() >= 2 and (o["state"][two][:, :, 9] == 0).all()
        assert np.array_equal(ce.bits_of(o["sub"][two, 1, 0]), ce.bits_of(grp.sub[two, 2]))
        one = (grp.family == "seq") & (arms == "pop") & (ce.arm_of(o, grp.n_sub, 1) == "plain")
        assert one.sum() >= 2 and (o["state"][one, 0, 9] == 0).all() and (o["state"][one, 1, 9] == 1).all()
    assert seen == set(ce.ARMS)
    print("cases per family:", {f: sum(int((g.family == f).sum()) for g in cat.values()) for f in ce.FAMILIES},
          "per group:", {n: g.n for n, g in cat.items()})


# mutation -> {family: cases that reject it}, summed over the three groups
REJECTS = {
    'd_sub <= 7': {'dsub7': 129, 'seq': 30, 'dgoal7': 10},
    'd_goal <= dist(sub0, goal)': {'clause2': 136, 'dgoal7': 66},
    'd_goal <= 7': {'dgoal7': 193},
    'd_sub < nextafter(7, 0)': {'dsub7': 30},
    'd_sub < nextafter(7, inf)': {'dsub7': 129, 'seq': 30, 'dgoal7': 10},
    'd_goal < nextafter(7, 0)': {'dgoal7': 21},
    'd_goal < nextafter(7, inf)': {'dgoal7': 193},
    'Step > max_step': {'dsub7': 115, 'clause2': 64, 'dgoal7': 134, 'both': 36, 'listlen': 36, 'alias': 42},
    'time-out tested after the pop': {'dsub7': 34, 'clause2': 56, 'both': 72, 'listlen': 36, 'alias': 42},
    'goal arm before the pop arm': {'both': 108, 'alias': 42, 'dgoal7': 6},
    'last pop without its +50': {'dsub7': 76, 'clause2': 124, 'both': 72, 'listlen': 48, 'alias': 54, 'dgoal7': 3},
    'Step not zeroed on a pop': {'dsub7': 67, 'clause2': 106, 'both': 72, 'listlen': 84, 'alias': 56, 'seq': 90, 'dgoal7': 3},
    'window reloaded from sub_idx': {'dsub7': 24, 'clause2': 36, 'both': 36, 'listlen': 60, 'alias': 26, 'seq': 30},
    'alias survives a collision': {'alias': 48},
    'thresholds at the moved position after a collision': {'dsub7': 50, 'clause2': 66, 'dgoal7': 51, 'both': 45, 'listlen': 40,
                                                           'alias': 36},
}
# the threshold families each mutation touches: every one of them must hold a case that rejects it
TOUCHES = {
    'd_sub <= 7': ('dsub7',), 'd_goal <= dist(sub0, goal)': ('clause2',), 'd_goal <= 7': ('dgoal7',),
    'd_sub < nextafter(7, 0)': ('dsub7',), 'd_sub < nextafter(7, inf)': ('dsub7',), 'd_goal < nextafter(7, 0)': ('dgoal7',),
    'd_goal < nextafter(7, inf)': ('dgoal7',), 'Step > max_step': ('dsub7', 'clause2', 'dgoal7'),
    'time-out tested after the pop': ('dsub7', 'clause2'), 'goal arm before the pop arm': ('both',),
    'last pop without its +50': ('dsub7', 'clause2'), 'Step not zeroed on a pop': ('dsub7', 'clause2', 'seq'),
    'window reloaded from sub_idx': ('seq',), 'alias survives a collision': ('alias',),
    'thresholds at the moved position after a collision': ('dsub7', 'clause2', 'dgoal7'),
}


@pytest.mark.parametrize("name", ce.MUTATIONS)
def test_catalogue_rejects_the_mutation(name):
    b, cat, oracle = _setup()
    counts = {}
    for gname, grp in cat.items():
        got, _ = ce.run_model(grp, b, mut=name)
        bad = ce.differs(got, oracle[gname])
        for fam in ce.FAMILIES:
            c = int((bad & (grp.family == fam)).sum())
            if c:
                counts[fam] = counts.get(fam, 0) + c
    print("mutation %r: %d cases rejected" % (name, sum(counts.values())), counts)
    assert all(counts.get(fam, 0) > 0 for fam in TOUCHES[name])
    assert counts == REJECTS[name]
