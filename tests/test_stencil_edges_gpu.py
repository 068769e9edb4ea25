"""The four device texts of the observation stencils against the oracle at every geometric edge (MI355X).

  obs_bits                                   k_observe                       one lane per agent
  obs_bits_queued                            k_step (64 and 256 threads), k_step_polh       per-wave LDS queue
  obs_cand_queued + box + below              k_step_coop (and its policy form)               three candidate phases
  the reset path of k_step_coop / k_step     the stencil sits on the reset candidate, not on the moved agent

all on the catalogue of tests/stencil_edges.py: adjacent doubles across rims (which on a stencil corner's diagonal are the
reject and accept radii), roofs, box faces, cell edges, cylinders tangent to a stencil's reach -- on a 29-cylinder world
(32-bit masks, cell 20) and a 40-cylinder world (64-bit masks, cell 13, inexact reciprocal).  The expected flags are 80
calls of the oracle's Threaten_rate per position; tests/test_stencil_edges.py shows on the host that this catalogue
rejects one-ulp and 1e-9 mutations of the tables and guards.

Every env has max_v = 0: the move adds +-0, so a stepped agent's stencil sits exactly on the injected position (asserted
from get_state, bit for bit).  Headings start in the first quadrant and steer actions are in [0, 1]; goal and both
sub-goals are one point some 280 m away, so nothing pops and no agent ends (asserted).  The pre-step state the device
reports is asserted equal to the one the oracle transition was computed from, once per world, in the fixture.

Flags (columns 11..85 and 90..94), info and ret_done are exact; the reward, which carries the collision probe's -0.3 for
agents inside a disc or outside the box, is held to the parity suite's REWARD_TOL.

Measured on an MI355X: the module takes about 13 s for its 25 tests, 8.6 s of it on the host, building the two
catalogues with their oracle flags and oracle transition once (109 536 positions for the 29-cylinder world, 125 670 for
the 40-cylinder one); no other test takes more than 0.2 s.  With a queue drain that skips one slot built in for a trial,
the lattice queue test failed and the crowd one did not: under the crowd another item usually sets the same flag.
"""
import math

import numpy as np
import pytest
import torch

import stencil_edges as se

pytestmark = pytest.mark.gpu

REWARD_TOL = 1e-9                      # as tests/test_env_parity_gpu.py
STEER = 30.0 / 180.0 * math.pi
MAX_STEP = 150
K = 8
PARAMS = dict(max_v=0.0, steering_angle=STEER, max_step=MAX_STEP, apf_enabled=0)
FMT = {"f32": torch.float32, "f16": torch.float16, "packed": "packed"}


def make_env(n, b, cell, fmt="f32", **kw):
    from dqn_based_uav_3d_path_planer_amd.env import VecPathPlanEnv
    return VecPathPlanEnv(n, b, cell_size=cell, max_v=0.0, max_subgoals=K, max_step=MAX_STEP, steering_angle=STEER,
                          obs_dtype=FMT[fmt], **kw)


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def flags_of(env, obs):
    """The 80 flags of observation rows as this env stores them -> [n, 80] uint8 (they are 0.0 / 1.0 in every format)."""
    rows = env.unpack(obs).float().cpu().numpy()
    f = rows[:, se.FLAG_COLS]
    assert np.isin(f, (0.0, 1.0)).all()
    return f.astype(np.uint8)


class Case:
    """Positions in one world with everything a step test injects and expects.  Built once; never modified."""

    def __init__(self, b, cell, pos, seed=1, step=0, steer=None):
        from oracle import pyoracle as po
        rng = np.random.default_rng(seed)
        n = len(pos)
        self.b, self.cell, self.pos, self.n = b, cell, np.ascontiguousarray(pos), n
        self.world = po.OracleWorld(b)
        self.want = se.oracle_flags(self.world, pos)
        h = rng.uniform(0.1, 0.9, n)                                          # strictly inside the first quadrant
        goal = np.c_[np.where(pos[:, 0] < 250.0, pos[:, 0] + 200.0, pos[:, 0] - 200.0),
                     np.where(pos[:, 1] < 250.0, pos[:, 1] + 200.0, pos[:, 1] - 200.0), np.full(n, 20.0)]
        self.kin = np.c_[pos, np.cos(h), np.sin(h), goal]
        self.sub = np.zeros((n, K, 3))
        self.sub[:, 0] = self.sub[:, 1] = goal
        self.step0 = np.full(n, step, dtype=np.int32)
        self.n_sub = np.full(n, 2, dtype=np.int32)
        self.alias = np.zeros(n, dtype=np.int32)
        self.actions = rng.uniform(0.0, 1.0, n) if steer is None else np.asarray(steer, dtype=np.float64)
        # the state the device must report before the step (max_v = 0: Calc_V scales the injected heading vector to +0)
        st = np.zeros((n, 16))
        st[:, 0:3], st[:, 6:9], st[:, 9], st[:, 11] = pos, goal, step, 2
        self.state0 = st
        batch = po.OracleBatch(self.world, PARAMS, n)
        batch.set_from_state16(st, self.sub, self.alias)
        self.reward, self.ret_done, self.info, obs_o = batch.step(self.actions, want_obs=True)
        self.agent_done = batch.view["done"].copy()
        v = batch.view
        self.pos_after = np.c_[v["px"], v["py"], v["pz"]]
        self.obs_flags = obs_o[:, se.FLAG_COLS].astype(np.uint8)

    def inject(self, env, idx):
        env.set_state(0, self.kin[idx], self.step0[idx], self.n_sub[idx], self.sub[idx], alias=self.alias[idx])
        st, sub, alias = env.get_state(0, len(idx), want_sub=True)
        assert np.array_equal(bits_of(st), bits_of(self.state0[idx])), "pre-step state is not the one the oracle stepped"
        assert np.array_equal(bits_of(sub), bits_of(self.sub[idx])) and not alias.any()

    def step(self, env, idx, out=None, **kw):
        """Inject, step once, and hold every output to the oracle's.  -> the StepOut."""
        self.inject(env, idx)
        a = torch.tensor(self.actions[idx], dtype=torch.float64, device="cuda")
        out = env.step(a, out, **kw)
        torch.cuda.synchronize()
        st1 = env.get_state(0, len(idx))
        assert np.array_equal(bits_of(st1[:, 0:3]), bits_of(self.pos[idx])), "a stepped agent left its injected position"
        assert np.abs(out.reward.cpu().numpy() - self.reward[idx]).max() <= REWARD_TOL
        assert np.array_equal(out.info.cpu().numpy(), self.info[idx].astype(np.uint8))
        assert np.array_equal(out.ret_done.cpu().numpy(), self.ret_done[idx].astype(np.uint8))
        assert not out.agent_done.cpu().numpy().any()
        self.check_flags(flags_of(env, out.obs), idx)
        return out

    def check_flags(self, got, idx, what=""):
        bad = np.nonzero((got != self.want[idx]).any(axis=1))[0]
        assert len(bad) == 0, (what, len(bad), [(self.pos[idx][k].tolist(), np.nonzero(got[k] != self.want[idx][k])[0].tolist())
                                                for k in bad[:4]])


_CASES = {}


def _world_case(name):
    if name not in _CASES:
        wide, cell = {"u32": (False, 20.0), "u64": (True, 13.0)}[name]
        b = se.edge_world(cell, wide)
        pos, kinds = se.edge_positions(b, cell)
        c = Case(b, cell, pos)
        c.kinds = kinds
        # the oracle itself: no agent ends, nothing moves, and its observation carries the same 80 flags
        assert not c.agent_done.any() and not c.ret_done.any()
        assert np.array_equal(bits_of(c.pos_after), bits_of(pos))
        assert np.array_equal(c.obs_flags, c.want)
        assert (c.info == 0).all() and (c.reward < -0.3).any() and (c.reward > -0.3).any()
        print(f"catalogue {name}: {len(b)} cylinders, cell {cell}, {len(pos)} positions")
        _CASES[name] = c
    return _CASES[name]


@pytest.fixture(scope="module")
def cases():
    yield _world_case
    _CASES.clear()


# ------------------------------------------------------------------------------------------------- k_observe: obs_bits
@pytest.mark.parametrize("name,fmt", [("u32", "f32"), ("u32", "f16"), ("u32", "packed"), ("u64", "f32"), ("u64", "f16"),
                                      ("u64", "packed")])
def test_observe_lane_per_agent(cases, name, fmt):
    c = cases(name)
    idx = np.arange(c.n)
    env = make_env(c.n, c.b, c.cell, fmt)
    c.inject(env, idx)
    obs = env.observe()
    c.check_flags(flags_of(env, obs), idx, "k_observe")
    env.close()


# ------------------------------------------------------------------------------------------------- k_step: obs_bits_queued
@pytest.mark.parametrize("name,fmt", [("u32", "f32"), ("u32", "packed"), ("u64", "f16"), ("u64", "f32")])
def test_step_single_wave_workgroups(cases, name, fmt):
    """k_step at 64 threads per workgroup (one_wave): the catalogue in chunks of at most 131 072 agents.  (f32 rows leave
    through the compact LDS tile at this size, f16 and packed rows row by row.)"""
    c = cases(name)
    for lo in range(0, c.n, 131072):
        idx = np.arange(lo, min(c.n, lo + 131072))
        env = make_env(len(idx), c.b, c.cell, fmt)
        c.step(env, idx, one_wave=True)
        env.close()


@pytest.mark.parametrize("name,fmt", [("u32", "f16"), ("u64", "f32"), ("u32", "packed")])
def test_step_256_thread_workgroups(cases, name, fmt):
    """k_step at 256 threads per workgroup: the catalogue tiled to 131 072 + 64 * 3 + 5 agents (a ragged last wavefront in a
    ragged last workgroup), canary rows behind the observation buffer."""
    c = cases(name)
    n = 131072 + 64 * 3 + 5
    idx = np.arange(n) % c.n
    env = make_env(n, c.b, c.cell, fmt)
    canary = -7
    guard = torch.full((n + 64, env.obs_width), canary, device="cuda", dtype=env.obs_dtype)
    out = env.alloc_out()
    out.obs = guard[:n]
    c.step(env, idx, out)
    assert torch.all(guard[n:] == canary)                              # nothing written past agent N - 1
    env.close()


# ------------------------------------------------------------------------------------------------- k_step_coop: obs_cand_queued
def _coop_chunks(n):
    """Chunks of at most 49 152 agents whose last ones are ragged: 65, 63 and 1 agents."""
    tail = [65, 63, 1]
    edges, lo = [], 0
    body = n - sum(tail)
    while lo < body:
        hi = min(body, lo + 49152)
        edges.append((lo, hi))
        lo = hi
    for t in tail:
        edges.append((lo, lo + t))
        lo += t
    assert lo == n
    return edges


@pytest.mark.parametrize("name,fmt", [("u32", "f32"), ("u64", "packed"), ("u64", "f16")])
def test_step_cooperative_and_agreement_with_single_wave(cases, name, fmt):
    """k_step_coop on the whole catalogue; then the same chunk through one_wave on the same env: the two kernels must agree
    bit for bit on every output, not only on the flags."""
    c = cases(name)
    for lo, hi in _coop_chunks(c.n):
        idx = np.arange(lo, hi)
        env = make_env(len(idx), c.b, c.cell, fmt)
        oa = c.step(env, idx)                                          # N <= 49 152: the cooperative kernel
        sa = env.get_state(0, len(idx))
        ob = c.step(env, idx, one_wave=True)
        sb = env.get_state(0, len(idx))
        for field in ("reward", "reward32", "ret_done", "agent_done", "info", "valid", "obs"):
            assert torch.equal(getattr(oa, field), getattr(ob, field)), (lo, field)
        assert np.array_equal(bits_of(sa), bits_of(sb))
        env.close()


# ------------------------------------------------------------------------------------------------- the policy instantiations
def _policy_launch(c, idx, fmt, learner_args, seed):
    """One uavenv_step_policy launch from the injected catalogue: the flags of the next frame's rows, and `done`."""
    from oracle import pyoracle as po
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
    n = len(idx)
    env = make_env(n, c.b, c.cell, fmt)
    ring = DeviceReplayRing(env, 2 * n, discrete=True)
    c.inject(env, idx)
    frame = ring.head
    env.observe(ring.obs[frame])
    torch.manual_seed(seed)
    cfg = {"w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99", "Update_loop": "3"}
    L = FusedDQNLearner(dict(cfg, NetWork=learner_args[0]), learner_args[1], device="cuda:0", **learner_args[2])
    assert ring.step_policy(L, 0.0, 23, 0, auto_reset=False)          # the launch took the in-kernel policy
    torch.cuda.synchronize()
    a = ring.action[frame].cpu().numpy()
    assert a.min() >= 0 and a.max() <= 2
    st1 = env.get_state(0, n)
    assert np.array_equal(bits_of(st1[:, 0:3]), bits_of(c.pos[idx]))      # the move is still zero
    batch = po.OracleBatch(c.world, PARAMS, n)
    batch.set_from_state16(c.state0[idx], c.sub[idx], c.alias[idx])
    r_o, d_o, i_o, _ = batch.step(-1.0 + a.astype(np.float64), want_obs=False)
    assert not batch.view["done"].any()
    assert np.array_equal(ring.done[frame].cpu().numpy(), d_o.astype(np.uint8))
    c.check_flags(flags_of(env, ring.obs[ring.head]), idx, "policy launch")
    env.close()


def test_policy_form_of_the_cooperative_kernel_on_packed_rows(cases):
    """k_step_coop<.., PACKED, POLICY>: the fc1 image sits in LDS beside the three stencil queues."""
    c = cases("u64")
    idx = np.arange(0, c.n, 3)[:40000]
    _policy_launch(c, idx, "packed", ("Qnet2", "dqn", {}), seed=4)


def test_policy_wavefronts_beside_the_queue_on_f16_rows(cases):
    """k_step_polh: the f16 policy team's tiles share the workgroup's LDS with the agent wavefront's queue.  (The launch
    takes an even agent count in (49 152, 65 536] and a world that leaves the team its 27 KB: the 32-bit-mask world.)"""
    c = cases("u32")
    idx = np.arange(0, c.n, 2)[:52000]
    assert len(idx) == 52000
    _policy_launch(c, idx, "f16", ("VAnet2", "dueling", dict(mfma="f16")), seed=3)


# ------------------------------------------------------------------------------------------------- the reset path
@pytest.mark.parametrize("name,one_wave", [("u32", False), ("u64", False), ("u64", True)])
def test_reset_path_places_the_stencil_on_the_reset_candidate(cases, name, one_wave):
    """Every agent one step from the Step limit, one auto-reset step: each restarts on a bank row whose start point is a
    catalogue position, and the returned observation must be the one AT that start point (k_step_coop reads it from the
    reset candidate in LDS, k_step from the reset agent)."""
    c = cases(name)
    rng = np.random.default_rng(17)
    t = c.kinds["tangent"]
    rows = np.unique(np.r_[np.arange(t.start, t.stop), rng.choice(c.n, 4000, replace=False)])
    start = c.pos[rows]
    key = {bits_of(p).tobytes(): k for k, p in enumerate(start)}       # (equal positions have equal flags)
    M = len(rows)
    far = np.c_[np.where(start[:, 0] < 250.0, start[:, 0] + 80.0, start[:, 0] - 80.0), start[:, 1], start[:, 2]]
    goal = np.c_[np.where(start[:, 0] < 250.0, start[:, 0] + 200.0, start[:, 0] - 200.0), start[:, 1], start[:, 2]]
    sub = np.zeros((M, K, 3))
    sub[:, 0], sub[:, 1], sub[:, 2] = start, far, goal
    N = 8 * M
    assert N <= 49152
    env = make_env(N, c.b, c.cell, "f32")
    env.load_scenarios(np.c_[start, goal], sub, np.full(M, 3, dtype=np.int32))
    idx = rng.integers(0, c.n, N)
    env.set_state(0, c.kin[idx], np.full(N, MAX_STEP - 1, dtype=np.int32), c.n_sub[idx], c.sub[idx], alias=c.alias[idx])
    out = env.step(torch.tensor(c.actions[idx], device="cuda"), auto_reset=True, one_wave=one_wave)
    torch.cuda.synchronize()
    assert (out.agent_done.cpu().numpy() == 1).all() and (out.info.cpu().numpy() == 2).all()      # out of steps: lose
    st1 = env.get_state(0, N)
    assert (st1[:, 9] == 0).all() and (st1[:, 10] == 0).all()                                 # restarted in this launch
    drawn = np.array([key.get(bits_of(p).tobytes(), -1) for p in st1[:, 0:3]])
    assert (drawn >= 0).all(), "an agent restarted somewhere that is no bank start"
    assert len(np.unique(drawn)) >= 0.95 * len(key)                    # a uniform draw of 8 M from M covers 1 - exp(-8)
    got = flags_of(env, out.obs)
    want = c.want[rows][drawn]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), st1[bad[:4], 0:3].tolist())
    env.close()


# ------------------------------------------------------------------------------------------------- the queue's drain branch
@pytest.mark.parametrize("kind", ["crowd", "lattice"])
def test_full_queues_drain_and_lose_nothing(kind):
    """3 * 64 + 17 agents whose every wholly crowded wavefront hands at least 4 x 512 (agent, cylinder, stencil) triples to
    the exact test (the host's geometric count; the device's guards can only add to it), each of k_step_coop's three
    candidate phases a third of that -- so every 512-entry queue drains on `count > 512 - 192` several times.  Wavefront 1
    has its odd lanes in an empty far cell: lanes without a candidate amid lanes that push.
      crowd    64 small cylinders in a 6 m patch, the agents among them (every flag under several discs at once);
      lattice  41 discs ON the points of the 5 m and 10 m stencils: every queue item owns a flag that no other item sets
               (asserted), so one lost, doubled or misplaced item is one wrong flag."""
    if kind == "crowd":
        b, lattice = se.queue_world(), se.queue_positions()
    else:
        b, lattice = se.lattice_world(), se.lattice_positions()
    far = np.asarray(se.QUEUE_FAR)
    n = 3 * 64 + 17
    pos = np.empty((n, 3))
    pos[0:64] = lattice
    pos[64:128] = lattice
    pos[65:128:2] = far
    pos[128:192] = lattice[::-1]
    pos[192:] = lattice[:17]
    is_far = np.zeros(n, dtype=bool)
    is_far[65:128:2] = True
    tri = se.full_triples(b, pos)
    for w0 in (0, 128):                                               # the two wholly crowded wavefronts
        assert tri[w0:w0 + 64].sum() >= 4 * 512
        for ph in range(3):                                           # every cylinder is a candidate of every crowd agent,
            cyl = np.arange(ph, len(b), 3)                             # in index order: phase ph takes every third from ph
            assert se.full_triples(b, pos[w0:w0 + 64], cyl).sum() >= 4 * 512 / 3
    assert tri[64:128].sum() >= 512 and tri[is_far].sum() == 0
    c = Case(b, 20.0, pos, seed=2)
    assert not c.agent_done.any() and np.array_equal(c.obs_flags, c.want)
    assert not c.want[is_far].any() and c.want[~is_far, :75].any(axis=1).all()
    if kind == "lattice":      # 50 triples of the two wide stencils, 50 flags, all set: each triple sets exactly one of them
        assert (tri[~is_far] == 51).all() and c.want[~is_far, 25:75].all()      # (the 51st: the centre disc in the 1 m stencil)
    idx = np.arange(n)
    for fmt in ("f32", "packed"):
        env = make_env(n, b, 20.0, fmt)
        c.inject(env, idx)
        c.check_flags(flags_of(env, env.observe()), idx, "k_observe")
        for one_wave in (True, False):
            out = c.step(env, idx, one_wave=one_wave)
            assert not flags_of(env, out.obs)[is_far].any()
        env.close()


# ------------------------------------------------------------------------------------------------- the single-point probe
@pytest.mark.parametrize("name", ["u32", "u64"])
def test_single_point_probe_on_the_edge_worlds(cases, name):
    """probe() through the 2 m halo grid on all 80 probe points of every eighth catalogue position: equal to the all-pairs
    loop and to the oracle (the known-answer file of the single-point probe only knows the stock world)."""
    c = cases(name)
    idx = np.arange(0, c.n, 8)
    pts = torch.tensor(se.probe_points(c.pos[idx]).reshape(-1, 3), device="cuda")
    env = make_env(4, c.b, c.cell)
    got = env.threaten_rate(pts)
    assert torch.equal(got, env.threaten_rate(pts, allpairs=True))
    assert np.array_equal(got.cpu().numpy().reshape(-1, 80), c.want[idx])
    env.close()
