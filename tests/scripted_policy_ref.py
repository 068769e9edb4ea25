"""The scripted baseline policy (include/uavenv.h: uavenv_scripted_act, uavenv_eval_episodes_scripted) in numpy float64 -- the
independent reference of tests/test_eval_scripted.py and tests/test_eval_scripted_gpu.py, written from the rule and not from the
kernel.  It works on the state of the C oracle's agents (oracle/pyoracle.py: OracleUav, OracleBatch) and probes through
OracleWorld.threaten_rate_many.

The rule, for candidate steers k = 0 .. C - 1 (index kind: -1 + 2k / (A - 1); steer kind: the f32 value of -1 + 2k / (C - 1)):
  no sub-goal left -> candidate C // 2;
  err = calculate_angle(sub0 - pos) - calculate_angle(0, V_vector), wrapped (> pi: - 2 pi; <= -pi: + 2 pi);
  s* = clamp(err / Steering_angle, -1, 1); cost_k = |steer_k - s*|;
  candidate k is blocked where Threaten_rate(pos + t V_k) = 1 for some t = 1 .. H, V_k = the V_vector update_PathPlan sets for
  steer_k (UAV.py:411-417, Calc_V's clamp included);
  the unblocked candidate of least cost, the lower k on equal cost; all blocked: the least cost among the candidates whose t = 1
  probe is free (so that a step collides only when every candidate's next point is blocked); none of those: the least cost overall.

Every decision comes with a margin: the least of the gap between the two smallest costs, |err -+ pi| before wrapping and, over all
C x H probe points, the distances to the box faces (x and y against 0 and `width`) and |distance to a building's axis - R| for every
building.  A decision whose margin is below FRAGILE may legitimately differ between two correct implementations (sincos / atan2 in
the last place); the tests accept either side's action there and nothing else.
"""
import math

import numpy as np

FRAGILE = 1e-6
INDEX, STEER = "index", "steer"


def calculate_angle(dx, dy):
    """BaseClass/CalMod.py:89-102 calculate_angle(p1, p2) with (dx, dy) = p2 - p1, in radians."""
    a = np.arctan2(dy, dx) * (180.0 / math.pi)
    return ((a + 360.0) % 360.0) / 180.0 * math.pi


def candidate_steers(kind, C):
    k = np.arange(C, dtype=np.float64)
    s = -1.0 + 2.0 * k / float(C - 1)
    return s if kind == INDEX else s.astype(np.float32).astype(np.float64)


class Decision:
    """k [n] int, steer [n] f64, margin [n] f64, all_blocked_t1 [n] bool (every candidate's t = 1 probe is 1; False with H = 0),
    blocked [n, C] bool."""

    def __init__(self, k, steer, margin, all_blocked_t1, blocked):
        self.k, self.steer, self.margin, self.all_blocked_t1, self.blocked = k, steer, margin, all_blocked_t1, blocked

    @property
    def fragile(self):
        return self.margin < FRAGILE


def decide(world, buildings, width, max_v, steering_angle, pos, sub0, v, n_sub, kind, C, H):
    """The rule for n agents.  world: OracleWorld; buildings: [nb, 5] (cx, cy, cz, R, H); pos [n, 3]; sub0 [n, 2+]; v [n, 2] the
    current V_vector; n_sub [n]."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    sub0 = np.asarray(sub0, np.float64).reshape(len(pos), -1)
    v = np.asarray(v, np.float64).reshape(-1, 2)
    n_sub = np.asarray(n_sub).reshape(-1)
    n = len(pos)
    steers = candidate_steers(kind, C)
    head = calculate_angle(v[:, 0], v[:, 1])
    beta = calculate_angle(sub0[:, 0] - pos[:, 0], sub0[:, 1] - pos[:, 1])
    raw = beta - head
    err = np.where(raw > math.pi, raw - 2.0 * math.pi, raw)
    err = np.where(err <= -math.pi, err + 2.0 * math.pi, err)
    want = np.clip(err / steering_angle, -1.0, 1.0)
    cost = np.abs(steers[None, :] - want[:, None])                  # [n, C]
    margin = np.minimum(np.abs(raw - math.pi), np.abs(raw + math.pi))
    two = np.sort(cost, axis=1)[:, :2]
    margin = np.minimum(margin, two[:, 1] - two[:, 0])
    blocked = np.zeros((n, C), bool)
    hit_t1 = np.zeros((n, C), bool)
    all_t1 = np.zeros(n, bool)
    if H > 0:
        seta = head[:, None] + steers[None, :] * steering_angle
        vx, vy = max_v * np.cos(seta), max_v * np.sin(seta)
        V = np.sqrt(vx * vx + vy * vy + 0.0)
        over = V > max_v
        scale = np.where(over, max_v / np.where(over, V, 1.0), 1.0)
        vx, vy = np.where(over, vx * scale, vx), np.where(over, vy * scale, vy)
        t = np.arange(1, H + 1, dtype=np.float64)
        x = pos[:, 0, None, None] + t[None, None, :] * vx[:, :, None]          # [n, C, H]
        y = pos[:, 1, None, None] + t[None, None, :] * vy[:, :, None]
        z = np.broadcast_to(pos[:, 2, None, None], x.shape)
        hit = world.threaten_rate_many(np.stack([x, y, z], -1).reshape(-1, 3)).reshape(n, C, H) == 1
        blocked = hit.any(2)
        hit_t1 = hit[:, :, 0]
        all_t1 = hit_t1.all(1)
        face = np.minimum(np.minimum(np.abs(x), np.abs(x - width)), np.minimum(np.abs(y), np.abs(y - width)))
        b = np.asarray(buildings, np.float64).reshape(-1, 5)
        rim = np.full(x.shape, np.inf)
        for cx, cy, _, R, _ in b:
            rim = np.minimum(rim, np.abs(np.sqrt((x - cx) ** 2 + (y - cy) ** 2) - R))
        margin = np.minimum(margin, np.minimum(face, rim).reshape(n, -1).min(1))
    free_cost = np.where(blocked, np.inf, cost)
    next_cost = np.where(hit_t1, np.inf, cost)
    k = np.where(~blocked.all(1), np.argmin(free_cost, 1),                      # (argmin: the first of equal costs)
                 np.where(~all_t1, np.argmin(next_cost, 1), np.argmin(cost, 1)))
    empty = n_sub == 0
    k = np.where(empty, C // 2, k).astype(np.int64)
    margin = np.where(empty, np.inf, margin)
    return Decision(k, steers[k], margin, all_t1 & ~empty, blocked)


class Policy:
    """The rule bound to a world and the UAV parameters: decide_uav(OracleUav), decide_batch(OracleBatch), decide_state(state16, sub)."""

    def __init__(self, world, buildings, width, max_v, steering_angle, kind, C, H):
        assert kind in (INDEX, STEER)
        self.world, self.buildings, self.width = world, np.asarray(buildings, np.float64).reshape(-1, 5), float(width)
        self.max_v, self.steering_angle, self.kind, self.C, self.H = float(max_v), float(steering_angle), kind, int(C), int(H)

    def _decide(self, pos, sub0, v, n_sub):
        return decide(self.world, self.buildings, self.width, self.max_v, self.steering_angle, pos, sub0, v, n_sub, self.kind,
                      self.C, self.H)

    def decide_uav(self, uav):
        u = uav.u
        sub0 = [u.sub[0][0], u.sub[0][1]] if u.n_sub > 0 else [0.0, 0.0]
        return self._decide([[u.px, u.py, u.pz]], [sub0], [[u.vx, u.vy]], [u.n_sub])

    def decide_batch(self, batch):
        v = batch.view
        return self._decide(np.stack([v["px"], v["py"], v["pz"]], 1), v["sub"][:, 0, :2], np.stack([v["vx"], v["vy"]], 1), v["n_sub"])

    def decide_state(self, st, sub):
        """st: [n, 16] of uavenv_get_state, sub: its [n, K, 3] lists (row 0 = the current sub-goal)."""
        return self._decide(st[:, :3], sub[:, 0, :2], st[:, 3:5], st[:, 11].astype(np.int64))

    def action(self, d):
        """What the device writes for decision d: int32 indices or f32 steers."""
        return d.k.astype(np.int32) if self.kind == INDEX else d.steer.astype(np.float32)


def city_policy(c, kind, C, H, velocities=None):
    """Policy on the packaged city (data.load_city26()) -> (policy, world)."""
    from oracle import pyoracle as po
    world = po.OracleWorld(c["buildings"], c["len"], c["width"], c["h"], velocities=velocities)
    return Policy(world, c["buildings"], float(c["width"]), float(c["max_v"]), float(c["steering_angle"]), kind, C, H), world
