"""Directed pre-step states for the termination cascade of update_PathPlan (Agents/UAV.py:456-513).

Shared by tests/test_cascade_edges.py (host), tests/test_cascade_edges_gpu.py (device) and oracle/gen_golden.py
(gen_cascade_edges, which runs the same catalogue through the executed reference).  No GPU here.

The cascade decides time-out, sub-goal pop, final pop, goal reached or plain step on three comparisons of distances
(d_sub < 7, d_goal < dist(sub0, goal), d_goal < 7) and one of integers (Step >= max_step).  A uniform draw never puts a
distance ON its threshold or on a neighbouring double; the catalogue built here is made of nothing else, on the stock
world (tests/golden/world_stock.npz):

  every move is exact   group "v0" / "v0k3": max_v = 0, the move adds +-0 (headings in the first quadrant, so the scaled
                        velocity is +0); group "v1": max_v = 1, heading exactly 0 and action exactly 0, the move is +1 in x
                        on coordinates with few mantissa bits.  A case can therefore only disagree in the cascade.
  thresholds            by exactly representable offsets (Pythagorean quadruples of 7; mirror images about the goal) and by
                        bisection in one coordinate until two adjacent doubles give distances on either side; each with the
                        next double further in and further out.  With pz = 0 an altitude-only offset of nextafter(7, .) IS the
                        neighbouring double of 7.
  crossed with          Step before the move in {0, 17, max_step - 2, max_step - 1, max_step}; n_sub in {0, 1, 2, 3, K - 1, K}
                        (K = 8, and K = 3 in group "v0k3", where the list is full); the alias of the first step after a reset;
                        a collision on that step (out of the box, into a disc, or standing in one), which restores the position
                        so that every threshold is placed at the OLD position.
  two steps             every case is stepped twice: after a pop Step restarts from 0 and the window moves up by one; family
                        "seq" pops twice in a row, which is where a window reloaded from the wrong list index shows.

uavenv_set_state always gives the agent a private list (scn = -1); an agent whose list still lives in a bank row comes
only from a reset, at the bank's start point with a drawn heading, where no threshold can be placed exactly.  So the ABI
cannot place that case; tests/test_stencil_edges_gpu.py and tests/test_team_protocol_gpu.py step such agents.

model_step is a short f64 restatement of the transition with named mutations (MUTATIONS); tests/test_cascade_edges.py
shows that the catalogue rejects each of them.
"""
import math

import numpy as np

W, HBOX = 500.0, 100.0
MAX_STEP = 150
STEER = 30.0 / 180.0 * math.pi
REWARD_TOL = 1e-9                      # as tests/test_env_parity_gpu.py
GROUPS = {"v0": dict(max_v=0.0, K=8), "v1": dict(max_v=1.0, K=8), "v0k3": dict(max_v=0.0, K=3)}
FAMILIES = ("dsub7", "clause2", "dgoal7", "both", "nothing_left", "listlen", "alias", "seq")
ARMS = ("nothing_left", "timeout", "pop", "last_pop", "goal", "plain")
_INF = math.inf
nextafter = math.nextafter


def dist(a, b):
    """Eu_Loc_distance as the device and the oracle evaluate it: sqrt(dx*dx + dy*dy + dz*dz), left to right."""
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def threat(buildings, x, y, z):
    """Threaten_rate (Envs/PathPlan_City.py:215-223 + Obstacles/building.py:20-26)."""
    if x < 0 or x > W or y < 0 or y > W or z < 0 or z > HBOX:
        return True
    for cx, cy, _, R, H in buildings:
        if not z > H and math.sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy) + 0.0) < R:
            return True
    return False


def bisect(f, lo, hi):
    """f(lo) and not f(hi) -> adjacent doubles (lo, hi) with f(lo) and not f(hi)."""
    assert f(lo) and not f(hi)
    while True:
        mid = lo + (hi - lo) / 2
        if not min(lo, hi) < mid < max(lo, hi):
            break
        if f(mid):
            lo = mid
        else:
            hi = mid
    assert nextafter(lo, hi) == hi
    return lo, hi


def _four(lo, hi):
    """The two doubles of a flip and the next one on either side, inside first."""
    return nextafter(lo, lo - (hi - lo) * 4), lo, hi, nextafter(hi, hi + (hi - lo) * 4)


def _with(p, axis, v):
    q = list(p)
    q[axis] = v
    return tuple(q)


def _add(p, q, s=1.0):
    return (p[0] + s * q[0], p[1] + s * q[1], p[2] + s * q[2])


def _far_list(k0, n):
    """Recognisable far-away list entries (every one different, none near an agent)."""
    return [(100.0 + 10.0 * k, 440.0 - k, 5.0 + k) for k in range(k0, k0 + n)]


# offsets of length exactly 7 (Pythagorean quadruples), the first three axis-aligned (the third: altitude only)
SEVENS = ((7.0, 0.0, 0.0), (0.0, -7.0, 0.0), (0.0, 0.0, 7.0), (2.0, 3.0, 6.0), (-6.0, 2.0, 3.0), (3.0, -6.0, -2.0))
# oblique offsets of length about 7: only bisection finds their flip
OBLIQUE = ((4.1, -3.3, 4.6), (-1.7, 6.3, 2.2), (5.9, 3.7, 0.0))


def _axis_of(q):
    return max(range(3), key=lambda k: abs(q[k]))


def place_dsub7(P):
    """-> [(sub0, goal, tag)]: d_sub across 7 (below pops), the second clause false (d_goal = 40 > dist(sub0, goal) = 33)."""
    out = []
    for q in SEVENS + OBLIQUE:
        ax = _axis_of(q)
        goal = _add(P, q, 40.0 / 7.0)
        s_in, s_out = _add(P, q, 0.5), _add(P, q, 1.5)
        lo, hi = bisect(lambda v: dist(P, _with(s_in, ax, v)) < 7.0, s_in[ax], s_out[ax])
        base = _add(P, q)
        for v in _four(lo, hi):
            out.append((_with(base, ax, v), goal, "q=%s" % (q,)))
        if q in SEVENS:
            assert dist(P, base) == 7.0
            out.append((base, goal, "exact q=%s" % (q,)))
    if P[2] == 0.0:      # altitude only, from the ground: the offset IS the distance, so these are the neighbours of 7 themselves
        for z in (nextafter(7.0, 0.0), 7.0, nextafter(7.0, _INF), -nextafter(7.0, 0.0), -7.0, -nextafter(7.0, _INF)):
            s0 = (P[0], P[1], z)
            assert dist(P, s0) == abs(z)
            out.append((s0, (P[0], P[1], 40.0 if z > 0 else -40.0), "altitude %r" % z))
    return out


# (a, b, c), mirror axis: goal = P + (a, b, c), sub0 = P mirrored about the goal along that axis -> d_goal == dist(sub0, goal)
MIRRORS = (((5.0, 12.0, 0.0), 0), ((12.0, 5.0, 0.0), 1), ((3.0, 4.0, 12.0), 2), ((8.0, 9.0, 12.0), 0),
           ((5.3, 11.7, 2.9), 0), ((2.9, -6.1, 7.7), 2))


def place_clause2(P):
    """-> [(sub0, goal, tag)]: d_goal across dist(sub0, goal) (below pops) with d_sub >= 7 and d_goal >= 7."""
    out = []
    for (q, ax) in MIRRORS:
        goal = _add(P, q)
        mirror = _with(P, ax, P[ax] + 2.0 * q[ax])
        dg = dist(P, goal)
        assert dg >= 7.0 and dist(P, mirror) >= 7.0
        exact = all(float(v).is_integer() for v in q)
        if exact:
            assert dist(mirror, goal) == dg
            out.append((mirror, goal, "mirror q=%s" % (q,)))
        sgn = 1.0 if q[ax] > 0 else -1.0
        # further from the goal along the axis: dist(sub0, goal) grows, the clause becomes true
        lo, hi = bisect(lambda v: dg < dist(_with(mirror, ax, v), goal), mirror[ax] + sgn, mirror[ax] - sgn)
        for v in _four(lo, hi):
            out.append((_with(mirror, ax, v), goal, "q=%s" % (q,)))
    return out


def place_dgoal7(P):
    """-> [(sub0, goal, tag)]: d_goal across 7 (below reaches the goal) with d_sub = 8 and dist(sub0, goal) about 1, and
    at d_goal = 7 exactly also sub0 = P + 2 q (d_goal == dist(sub0, goal) == 7: neither clause holds)."""
    out = []
    for q in SEVENS + OBLIQUE:
        ax = _axis_of(q)
        s0 = _add(P, q, 8.0 / 7.0)
        g_in, g_out = _add(P, q, 0.5), _add(P, q, 1.5)
        lo, hi = bisect(lambda v: dist(P, _with(g_in, ax, v)) < 7.0, g_in[ax], g_out[ax])
        base = _add(P, q)
        for v in _four(lo, hi):
            g = _with(base, ax, v)
            if not (dist(P, s0) >= 7.0 and not dist(P, g) < dist(s0, g)):
                continue
            out.append((s0, g, "q=%s" % (q,)))
        if q in SEVENS:
            out.append((s0, base, "exact q=%s" % (q,)))
            twice = _add(P, q, 2.0)
            assert dist(P, base) == 7.0 and dist(twice, base) == 7.0 and dist(P, twice) == 14.0
            out.append((twice, base, "exact, sub0 at 2 q=%s" % (q,)))
    if P[2] == 0.0:
        for z in (nextafter(7.0, 0.0), 7.0, nextafter(7.0, _INF)):
            out.append(((P[0], P[1], 8.0), (P[0], P[1], z), "altitude %r" % z))
    return out


PLACE = {"dsub7": place_dsub7, "clause2": place_clause2, "dgoal7": place_dgoal7}


def sides(P, s0, goal):
    """The sign of (left - right) of the three comparisons at the position the cascade evaluates them at."""
    sg = lambda a, b: (a > b) - (a < b)      # noqa: E731
    dg = dist(P, goal)
    return sg(dist(P, s0), 7.0), sg(dg, dist(s0, goal)), sg(dg, 7.0)


class Group:
    """The cases of one env configuration, as arrays.  Built once; never modified."""

    def __init__(self, name, rows):
        self.name, self.n = name, len(rows)
        self.max_v, self.K = GROUPS[name]["max_v"], GROUPS[name]["K"]
        K, n = self.K, self.n
        self.kin = np.array([r["pos"] + r["v"] + r["goal"] for r in rows], dtype=np.float64).reshape(n, 8)
        self.step0 = np.array([r["step"] for r in rows], dtype=np.int32)
        self.n_sub = np.array([len(r["subs"]) for r in rows], dtype=np.int32)
        self.sub = np.zeros((n, K, 3))
        for i, r in enumerate(rows):
            assert len(r["subs"]) <= K
            if r["subs"]:
                self.sub[i, :len(r["subs"])] = r["subs"]
        self.alias = np.array([r["alias"] for r in rows], dtype=np.int32)
        self.action = np.array([r["action"] for r in rows], dtype=np.float64)
        self.family = np.array([r["family"] for r in rows])
        self.side = np.array([r["side"] for r in rows], dtype=np.int8).reshape(n, 3)      # d_sub:7, d_goal:dist(sub0, goal), d_goal:7
        self.collide = np.array([r["collide"] for r in rows], dtype=bool)
        self.tag = [r["tag"] for r in rows]
        for a in (self.kin[:, 0:3], self.kin[:, 5:8], self.sub):
            assert not (np.signbit(a) & (a == 0.0)).any()                  # no -0.0: positions are asserted bit for bit
        self.params = dict(max_v=self.max_v, steering_angle=STEER, max_step=MAX_STEP, apf_enabled=0)

    def state16(self):
        """The [n, 16] pre-step state the device must report after set_state (Calc_V rescales the injected velocity)."""
        st = np.zeros((self.n, 16))
        vx, vy = self.kin[:, 3].copy(), self.kin[:, 4].copy()
        V = np.sqrt(vx * vx + vy * vy + 0.0)
        over = V > self.max_v
        k = np.where(over, self.max_v / np.where(over, V, 1.0), 1.0)
        vx, vy, V = np.where(over, vx * k, vx), np.where(over, vy * k, vy), np.where(over, self.max_v, V)
        st[:, 0:3], st[:, 3], st[:, 4], st[:, 5], st[:, 6:9] = self.kin[:, 0:3], vx, vy, V, self.kin[:, 5:8]
        st[:, 9], st[:, 11] = self.step0, self.n_sub
        return st


def _free_anchor(b, P, span):
    for dx in range(-span, span + 1):
        assert not threat(b, P[0] + dx, P[1], P[2]), (P, dx)


def build(buildings):
    """-> {group name: Group} on the world `buildings` (the stock world)."""
    b = [tuple(float(x) for x in r) for r in np.asarray(buildings, dtype=np.float64).reshape(-1, 5)]
    rows = {g: [] for g in GROUPS}
    count = [0]
    V0_ACTIONS = (0.0, 0.0, 0.0, -1.0, 0.0, 0.5, 0.0, 1.0, 0.0, -0.37)

    def emit(group, family, P, subs, goal, step, *, alias=0, collide=None, tag=""):
        """P: where the cascade evaluates (the position after the move, or the restored one after a collision).
        collide: None, or how the probe comes to hit: "stand" (P itself is blocked; v0) or "move" (P + (1, 0, 0) is; v1)."""
        c = count[0]
        count[0] += 1
        if GROUPS[group]["max_v"] == 0.0:
            pos = P
            h = 0.1 + 0.08 * (c % 10)                                      # strictly inside the first quadrant
            v = (math.cos(h), math.sin(h))
            action = V0_ACTIONS[c % len(V0_ACTIONS)]
            assert threat(b, *P) == (collide == "stand") and collide in (None, "stand")
        else:
            v, action = (1.0, 0.0), 0.0
            if collide == "move":
                pos = P
                assert not threat(b, *P) and threat(b, P[0] + 1.0, P[1], P[2])
            else:
                assert collide is None and not threat(b, *P)
                pos = (P[0] - 1.0, P[1], P[2])
                assert pos[0] + 1.0 == P[0]
        subs = [tuple(float(x) for x in s) for s in subs]
        if alias:
            assert subs and subs[0] == pos
            sd = (0, 0, 0)
        else:
            sd = sides(P, subs[0], goal) if subs else (0, 0, 0)
        rows[group].append(dict(pos=tuple(pos), v=v, goal=tuple(float(x) for x in goal), subs=subs, step=int(step), alias=int(alias),
                                action=action, family=family, side=sd, collide=collide is not None, tag=tag))

    A0, A1, AX = (60.0, 300.0, 0.0), (400.0, 420.0, 20.0), (0.0, 300.0, 0.0)       # free anchors: ground, altitude, on the face x = 0
    EDGE, DISC = (499.5, 420.0, 0.0), (383.0, 241.0, 0.0)                           # +1 in x: out of the box / into cylinder 17
    OUT, IN = (-3.0, 420.0, 0.0), (400.0, 241.0, 0.0)                               # standing outside the box / in cylinder 17
    for P in (A0, A1):
        _free_anchor(b, P, 3)
    assert not threat(b, *AX)
    STEPS = (MAX_STEP - 2, MAX_STEP - 1, MAX_STEP)

    for fam in ("dsub7", "clause2", "dgoal7"):
        # the plain crossings: both exact groups, ground and altitude, lists of 1, 2 and 3
        for P, group, nsub, step in ((A0, "v0", 1, 17), (A0, "v0", 3, 0), (A1, "v0", 2, 5), (AX, "v0", 2, 3),
                                     (A0, "v1", 2, 17), (A1, "v1", 1, 0), (A0, "v0k3", 3, 9)):
            for s0, goal, tag in PLACE[fam](P):
                emit(group, fam, P, [s0] + _far_list(1, nsub - 1), goal, step, tag=tag)
        # the Step limit crossed with every outcome
        for step in STEPS:
            for P, group, nsub in ((A0, "v0", 2), (A1, "v1", 1)):
                for s0, goal, tag in PLACE[fam](P)[::2]:
                    emit(group, fam, P, [s0] + _far_list(1, nsub - 1), goal, step, tag="Step %d, %s" % (step, tag))
        # a collision on the step: the thresholds sit at the old position
        for P, group, how, nsub in ((EDGE, "v1", "move", 1), (DISC, "v1", "move", 3), (OUT, "v0", "stand", 2), (IN, "v0", "stand", 1)):
            for s0, goal, tag in PLACE[fam](P):
                emit(group, fam, P, [s0] + _far_list(1, nsub - 1), goal, 5, collide=how, tag="collision, " + tag)
        for P, group, how in ((EDGE, "v1", "move"), (OUT, "v0", "stand")):
            for s0, goal, tag in PLACE[fam](P)[::3]:
                emit(group, fam, P, [s0, (200.0, 450.0, 3.0)], goal, MAX_STEP - 1, collide=how, tag="collision at the Step limit, " + tag)

    # ---- both the pop condition and d_goal < 7 hold: the pop arm comes first
    for group, P, how in (("v0", A0, None), ("v1", A0, None), ("v1", EDGE, "move"), ("v0k3", A1, None)):
        for nsub in (1, 2, 3):
            for step in (0, 17) + STEPS:
                for s0, goal in ((_add(P, (3.0, 0.0, 0.0)), _add(P, (4.0, 0.0, 0.0))), (_add(P, (0.0, 12.0, 0.0)), _add(P, (0.0, 5.0, 0.0))),
                                 (_add(P, (7.0, 0.0, 0.0)), _add(P, (3.0, 0.0, 0.0)))):
                    emit(group, "both", P, [s0] + _far_list(1, nsub - 1), goal, step, collide=how, tag="n_sub %d Step %d" % (nsub, step))

    # ---- nothing left: n_sub = 0 pays max_step - Step and nothing moves
    for group, P in (("v0", A0), ("v1", A0), ("v1", A1), ("v0k3", A1), ("v0", OUT)):
        for step in (0, 17) + STEPS:
            emit(group, "nothing_left", P if group != "v1" else _add(P, (1.0, 0.0, 0.0)), [], _add(P, (30.0, 40.0, 0.0)), step,
                 collide="stand" if P is OUT else None, tag="Step %d" % step)

    # ---- list length: every n_sub with a pop
    for group, P in (("v0", A0), ("v1", A1), ("v0k3", A0), ("v1", DISC)):
        K = GROUPS[group]["K"]
        for nsub in sorted({1, 2, 3, K - 1, K}):
            for step in (0, 17, MAX_STEP - 2, MAX_STEP - 1):
                for off in ((3.0, 0.0, 0.0), (0.0, -2.0, 6.0)):
                    emit(group, "listlen", P, [_add(P, off)] + _far_list(1, nsub - 1), _add(P, (90.0, 0.0, 0.0)), step,
                         collide="move" if P is DISC else None, tag="n_sub %d of K %d, Step %d" % (nsub, K, step))

    # ---- the alias of the first step after a reset: sub_goals[0] IS the position, the pop is immediate; with a collision the
    # alias ends, sub0 keeps the moved-to point and the position is restored
    for group, P, how in (("v0", A0, None), ("v1", A0, None), ("v0k3", A1, None), ("v1", EDGE, "move"), ("v1", DISC, "move"),
                          ("v0", OUT, "stand"), ("v0", IN, "stand")):
        for nsub in (1, 2, 3):
            for step in (0, MAX_STEP - 2, MAX_STEP - 1):
                pos = P if (how is not None or GROUPS[group]["max_v"] == 0.0) else (P[0] - 1.0, P[1], P[2])
                for goal in (_add(P, (90.0, 0.0, 0.0)), _add(P, (3.0, 4.0, 0.0))):
                    emit(group, "alias", P, [pos] + _far_list(1, nsub - 1), goal, step, alias=1, collide=how,
                         tag="n_sub %d Step %d" % (nsub, step))

    # ---- two pops in a row, and a pop then a plain step: the window moves up by one, Step restarts from 0
    for group, P in (("v0", A0), ("v1", A0), ("v0k3", A1), ("v1", A1)):
        K = GROUPS[group]["K"]
        P2 = P if GROUPS[group]["max_v"] == 0.0 else _add(P, (1.0, 0.0, 0.0))      # where the second step evaluates
        for nsub in sorted({3, 4, K} if K > 3 else {3}):
            for step in (0, 17, MAX_STEP - 2):
                for second in ("pop", "plain", "at7"):
                    off = {"pop": (0.0, 3.0, 4.0), "plain": (30.0, 40.0, 0.0), "at7": (7.0, 0.0, 0.0)}[second]      # (towards the goal)
                    lst = [_add(P, (2.0, 0.0, 0.0)), _add(P2, off)] + [(310.0 + 7.0 * k, 470.0 - k, 1.0 + k) for k in range(nsub - 2)]
                    emit(group, "seq", P, lst, _add(P, (120.0, 0.0, 0.0)), step, tag="then %s, n_sub %d Step %d" % (second, nsub, step))
    return {g: Group(g, r) for g, r in rows.items()}


# ------------------------------------------------------------------------------------------------ whole episodes
EP_START = (20.0, 480.0, 0.0)      # a lane that is free for 152 m along +x on the ground of the stock world
EP_K = 8


def episode_rows(buildings):
    """Scenario rows for the whole-episode entries (max_v = 1, initial V_vector (1, 0), steer 0): the UAV is at
    EP_START + (t, 0, 0) after t steps, so a threshold placed straight above the lane at x = 20 + T is met at step T with
    dx = 0 -- the altitude offset IS the distance, and its neighbouring doubles are those of 7.
    -> (start_goal [m, 6], sub [m, EP_K, 3], n_sub [m], tags, straight [m]): straight marks the rows on which sub-goal pursuit
    steers 0 all the way (the current sub-goal is never behind the UAV), which the scripted policy can fly."""
    b = [tuple(float(x) for x in r) for r in np.asarray(buildings, dtype=np.float64).reshape(-1, 5)]
    x0, y0, z0 = EP_START
    for t in range(153):
        assert not threat(b, x0 + t, y0, z0)
    rows = []

    def row(goal, subs, tag, straight):
        rows.append((goal, subs, tag, straight))

    below, above = nextafter(7.0, 0.0), nextafter(7.0, _INF)
    row((300.0, 300.0, 0.0), [], "nothing left", True)
    row((x0 + 420.0, y0, 0.0), [(x0 + 400.0, y0, 0.0)], "time-out at max_step", True)
    for T in (1.0, 6.0, 41.0):
        X = x0 + T
        for dz in (below, 7.0, above):
            row((X, y0, dz), [(X, y0, dz + 1.0)], "goal within %r at step %d" % (dz, T), dz < 7.0)
            row((X, y0, 40.0), [(X, y0, dz)], "last pop, d_sub %r at step %d" % (dz, T), dz < 7.0)
            # (a list of three starts with the start node, which the alias pops at step 1: the next threshold is met from step 2 on)
            Tm = max(T, 2.0)
            Xm = x0 + Tm
            row((Xm + 30.0, y0, 40.0), [EP_START, (Xm, y0, dz), (Xm + 30.0, y0, 3.0)], "pop, d_sub %r at step %d, then on" % (dz, Tm), dz < 7.0)
        # d_goal against dist(sub0, goal): the mirror image (equal at step T: the pop comes one step later) and its neighbours
        goal, mirror = (X + 5.0, y0 + 12.0, 0.0), (X + 10.0, y0, 0.0)
        assert dist((X, y0, 0.0), goal) == 13.0 == dist(mirror, goal)
        lo, hi = bisect(lambda v: 13.0 < dist((v, y0, 0.0), goal), mirror[0] + 1.0, mirror[0] - 1.0)
        for v in _four(lo, hi) + (mirror[0],):
            row(goal, [(v, y0, 0.0)], "d_goal against dist(sub0, goal) at step %d, sub0 x %r" % (T, v), True)
    m = len(rows)
    sg, sub, ns = np.zeros((m, 6)), np.zeros((m, EP_K, 3)), np.zeros(m, dtype=np.int32)
    for i, (goal, subs, _, _) in enumerate(rows):
        sg[i, 0:3], sg[i, 3:6], ns[i] = EP_START, goal, len(subs)
        if subs:
            sub[i, :len(subs)] = subs
    return sg, sub, ns, [r[2] for r in rows], np.array([r[3] for r in rows], dtype=bool)


def oracle_episodes(world, sg, sub, ns, params, cap=400):
    """Whole episodes under steer 0 from V_vector (1, 0) by the C oracle -> dict of per-row outcome (1 success, 2 lose), steps,
    ret (the rewards summed in step order), path_len, total_score, reach, popped."""
    import ctypes as C
    from oracle import pyoracle as po
    m = len(sg)
    batch = po.OracleBatch(world, params, m)
    for i in range(m):
        u = batch.arr[i]
        u.px, u.py, u.pz = (float(x) for x in sg[i, :3])
        u.gx, u.gy, u.gz = (float(x) for x in sg[i, 3:])
        u.vx, u.vy, u.vz = 1.0, 0.0, 0.0
        u.V = batch.lib.orc_calc_v(C.byref(u))
        u.step = u.done = u.reach_goal = u.error = 0
        u.score = u.total_score = u.path_len = 0.0
        u.n_sub = int(ns[i])
        u.sub0_alias = 1 if int(ns[i]) >= 2 else 0
        if ns[i] > 0:
            C.memmove(C.addressof(u.sub), np.ascontiguousarray(sub[i, :ns[i]]).ctypes.data, int(ns[i]) * 24)
    v = batch.view
    steps, outcome, ret = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m)
    rec = {k: np.zeros(m) for k in ("path_len", "total_score", "reach", "popped")}
    for _ in range(cap):
        live = outcome == 0
        if not live.any():
            break
        r, _, info, _ = batch.step(np.zeros(m), want_obs=False)
        steps[live] += 1
        ret[live] += r[live]
        dn = live & (v["done"] == 1)
        outcome[dn] = np.where(info[dn] == 2, 2, 1)
        rec["path_len"][dn], rec["total_score"][dn], rec["reach"][dn] = v["path_len"][dn], v["total_score"][dn], v["reach_goal"][dn]
        rec["popped"][dn] = ns[dn] - v["n_sub"][dn]
    assert (outcome != 0).all()
    return dict(rec, outcome=outcome, steps=steps, ret=ret)


# ------------------------------------------------------------------------------------------------ the host model
MUTATIONS = ("d_sub <= 7", "d_goal <= dist(sub0, goal)", "d_goal <= 7", "d_sub < nextafter(7, 0)", "d_sub < nextafter(7, inf)",
             "d_goal < nextafter(7, 0)", "d_goal < nextafter(7, inf)", "Step > max_step", "time-out tested after the pop",
             "goal arm before the pop arm", "last pop without its +50", "Step not zeroed on a pop",
             "window reloaded from sub_idx", "alias survives a collision", "thresholds at the moved position after a collision")


def _angle(x1, y1, x2, y2):
    a = math.atan2(y2 - y1, x2 - x1) * (180.0 / math.pi)
    return math.fmod(a + 360.0, 360.0) / 180.0 * math.pi


class Agent:
    """One agent in the device's form: a private list, the index of the first remaining entry, and a window of two."""

    def __init__(self, grp, i, st16):
        st = st16[i]
        self.p, self.v, self.V, self.goal = list(st[0:3]), [st[3], st[4]], st[5], tuple(st[6:9])
        self.step, self.done, self.reach, self.alias = int(st[9]), 0, 0, int(grp.alias[i])
        self.n_total, self.sub_idx = int(grp.n_sub[i]), 0
        self.lst = [tuple(r) for r in grp.sub[i]]
        self.s0 = self.lst[0] if self.n_total >= 1 else (0.0, 0.0, 0.0)
        self.s1 = self.lst[1] if self.n_total >= 2 else (0.0, 0.0, 0.0)
        self.score = self.total = self.path = 0.0

    def n_sub(self):
        return self.n_total - self.sub_idx

    def sub_list(self, K):
        """What uavenv_get_state reports: the window's first entry, then the list."""
        out = np.zeros((K, 3))
        for k in range(self.n_sub()):
            out[k] = self.s0 if k == 0 else self.lst[self.sub_idx + k]
        return out


def model_step(g, a0, max_v, buildings, mut=None):
    """update_PathPlan on Agent g (APF off) -> (reward, ret_done, info, arm).  mut: one of MUTATIONS, or None."""
    m = lambda name: mut == name      # noqa: E731
    if g.sub_idx >= g.n_total:                                                 # :400-406
        g.done = 1
        r = float(MAX_STEP - g.step)
        g.score += r
        return r, 1, 1, "nothing_left"
    r = 0.0
    g.step += 1
    old = tuple(g.p)
    seta_old = _angle(0.0, 0.0, g.v[0], g.v[1])
    dis_old, g_old = dist(g.p, g.s0), dist(g.p, g.goal)
    seta_new = seta_old + a0 * STEER
    g.v = [max_v * math.cos(seta_new), max_v * math.sin(seta_new)]
    g.V = math.sqrt(g.v[0] * g.v[0] + g.v[1] * g.v[1] + 0.0)
    g.p[0] += g.v[0]
    g.p[1] += g.v[1]
    if g.alias:
        g.s0 = tuple(g.p)
    tri_goal = _angle(g.p[0], g.p[1], g.s0[0], g.s0[1])
    tri_v = _angle(0.0, 0.0, g.v[0], g.v[1])
    moved = tuple(g.p)
    hit = threat(buildings, *g.p)
    if hit:
        r -= 0.3
        g.p = list(old)
        if m("alias survives a collision"):
            if g.alias:
                g.s0 = tuple(g.p)
        else:
            g.alias = 0
        tri_v = _angle(g.p[0], g.p[1], g.s0[0], g.s0[1])
    dis_new, g_new = dist(g.p, g.s0), dist(g.p, g.goal)
    r -= 0.13 * abs(a0)
    r += 0.2 * math.cos(abs(tri_goal - tri_v))
    r += 0.4 * (dis_old - dis_new)
    r += 0.4 * (g_old - g_new)
    r -= 0.1
    r -= 0.01 * abs(g.p[2] - g.s0[2])
    g.path += g.V

    at = moved if (hit and m("thresholds at the moved position after a collision")) else g.p
    d_sub, d_goal = dist(at, g.s0), dist(at, g.goal)
    seven_sub = nextafter(7.0, 0.0) if m("d_sub < nextafter(7, 0)") else nextafter(7.0, _INF) if m("d_sub < nextafter(7, inf)") else 7.0
    seven_goal = nextafter(7.0, 0.0) if m("d_goal < nextafter(7, 0)") else nextafter(7.0, _INF) if m("d_goal < nextafter(7, inf)") else 7.0
    near = d_sub <= seven_sub if m("d_sub <= 7") else d_sub < seven_sub
    d_sg = dist(g.s0, g.goal)
    closer = d_goal <= d_sg if m("d_goal <= dist(sub0, goal)") else d_goal < d_sg
    at_goal = d_goal <= seven_goal if m("d_goal <= 7") else d_goal < seven_goal
    late = g.step > MAX_STEP if m("Step > max_step") else g.step >= MAX_STEP
    pop = near or closer
    if m("time-out tested after the pop"):
        arm = "pop" if pop else "timeout" if late else "goal" if at_goal else "plain"
    elif m("goal arm before the pop arm"):
        arm = "timeout" if late else "goal" if at_goal else "pop" if pop else "plain"
    else:
        arm = "timeout" if late else "pop" if pop else "goal" if at_goal else "plain"
    if arm == "timeout":                                                       # :456-465
        g.done = 1
        r += 50.0 - d_sub
        g.score += r
        g.total += r
        return r, 1, 2, arm
    if arm == "pop":                                                           # :466-495
        r += 50.0 - d_sub
        g.sub_idx += 1
        g.alias = 0
        if g.sub_idx >= g.n_total:
            if not m("last pop without its +50"):
                r += 50.0
            g.done = 1
            r += float(MAX_STEP - g.step)
            g.score += r
            g.reach = 1
            g.total += r
            return r, 1, 1, "last_pop"
        if not m("Step not zeroed on a pop"):
            g.step = 0
        g.score = 0.0
        g.s0 = g.s1
        if g.sub_idx + 1 < g.n_total:
            g.s1 = g.lst[g.sub_idx if m("window reloaded from sub_idx") else g.sub_idx + 1]
        r += 0.2 * math.cos(abs(_angle(g.p[0], g.p[1], g.s0[0], g.s0[1]) - _angle(0.0, 0.0, g.v[0], g.v[1])))
        r += float(MAX_STEP - g.step)
        g.score += r
        g.total += r
        return r, 1, 1, arm
    if arm == "goal":                                                          # :496-509
        g.done = 1
        r += 50.0
        r += float(MAX_STEP - g.step)
        g.score += r
        g.reach = 1
        g.total += r
        return r, 1, 1, arm
    g.score += r
    g.total += r
    return r, 0, 0, arm


STEPS = 2           # every case is stepped twice, with the same action


def empty_outputs(n, K):
    return dict(reward=np.zeros((n, STEPS)), ret_done=np.zeros((n, STEPS), dtype=np.int32), info=np.zeros((n, STEPS), dtype=np.int32),
                state=np.zeros((n, STEPS, 16)), sub=np.zeros((n, STEPS, K, 3)), alias=np.zeros((n, STEPS), dtype=np.int32))


def run_model(grp, buildings, mut=None):
    """-> the outputs of both steps of every case of the group by model_step, and the arm each step took."""
    b = [tuple(float(x) for x in r) for r in np.asarray(buildings, dtype=np.float64).reshape(-1, 5)]
    out = empty_outputs(grp.n, grp.K)
    arms = np.empty((grp.n, STEPS), dtype=object)
    st16 = grp.state16()
    for i in range(grp.n):
        g = Agent(grp, i, st16)
        for t in range(STEPS):
            r, d, info, arms[i, t] = model_step(g, float(grp.action[i]), grp.max_v, b, mut)
            out["reward"][i, t], out["ret_done"][i, t], out["info"][i, t], out["alias"][i, t] = r, d, info, g.alias
            out["state"][i, t] = g.p + g.v + [g.V] + list(g.goal) + [g.step, g.done, g.n_sub(), g.score, g.total, g.path, g.reach]
            out["sub"][i, t] = g.sub_list(grp.K)
    return out, arms


def run_oracle(grp, world, apf=0):
    """-> the outputs of both steps by oracle/uav_oracle.c (orc_update_pathplan), in the layout of run_model."""
    from oracle import pyoracle as po
    batch = po.OracleBatch(world, dict(grp.params, apf_enabled=apf), grp.n)
    batch.set_from_state16(grp.state16(), grp.sub, grp.alias)
    out = empty_outputs(grp.n, grp.K)
    v = batch.view
    for t in range(STEPS):
        r, d, info, _ = batch.step(grp.action, want_obs=False)
        assert not v["error"].any()
        out["reward"][:, t], out["ret_done"][:, t], out["info"][:, t], out["alias"][:, t] = r, d, info, v["sub0_alias"]
        for k, name in enumerate(("px", "py", "pz", "vx", "vy", "V", "gx", "gy", "gz", "step", "done", "n_sub", "score", "total_score",
                                  "path_len", "reach_goal")):
            out["state"][:, t, k] = v[name]
        sub = v["sub"][:, :grp.K].copy()
        sub[np.arange(grp.K)[None, :] >= v["n_sub"][:, None]] = 0.0
        out["sub"][:, t] = sub
    return out


def arm_of(out, pre_n_sub, t=0):
    """The arm each case took at step t, from outputs alone (info, ret_done, done, reach, the change of n_sub)."""
    st = out["state"][:, t]
    n_before = pre_n_sub if t == 0 else out["state"][:, t - 1, 11]
    arms = np.empty(len(st), dtype=object)
    for i in range(len(st)):
        info, done, reach, popped = out["info"][i, t], st[i, 10], st[i, 15], n_before[i] - st[i, 11]
        if n_before[i] == 0:
            arms[i] = "nothing_left"
        elif info == 2:
            arms[i] = "timeout"
        elif info == 0:
            arms[i] = "plain"
        elif popped:
            arms[i] = "last_pop" if done else "pop"
        else:
            arms[i] = "goal"
            assert done and reach
    return arms


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


INT_COLS = [9, 10, 11, 15]          # Step, done, n_sub, reach_goal of the 16-column state


def differs(a, b, tol=REWARD_TOL):
    """Per case: an integer output differs, or a reward by more than tol (either step)."""
    bad = (a["ret_done"] != b["ret_done"]) | (a["info"] != b["info"]) | (np.abs(a["reward"] - b["reward"]) > tol)
    bad |= (a["state"][:, :, INT_COLS] != b["state"][:, :, INT_COLS]).any(axis=2) | (a["alias"] != b["alias"])
    bad |= (bits_of(a["sub"]) != bits_of(b["sub"])).any(axis=(2, 3))
    return bad.any(axis=1)
