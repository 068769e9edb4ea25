"""Inputs shared by tests/test_rrt_ref.py (CPU) and tests/test_rrt_forms_gpu.py (GPU): three worlds and, per world, M planner
rows with explicit starts, goals and uniform streams, chosen so that the CPU oracle's trees cover every launch form of
csrc/rrt.hip (trees above tier A's 320 nodes, trees in the second trip of the 256-node scans, rows that give up, paths
longer and shorter than K = 24).  test_rrt_ref.py asserts that coverage from the oracle alone, so a changed seed cannot
quietly lose it.  Everything here is a pure function of the constants below and the oracle (no GPU, no file but
tests/golden/world_stock.npz)."""
import functools

import numpy as np

from conftest import load_golden

M = 192                       # rows per world
STREAM = 6000                 # uniforms per row: 4 draws per iteration at most
MAX_ITER = 1500               # the node cap (2 048) cannot bind
TIER_A, SCAN, NODE_CAP = 320, 256, 2048     # csrc/rrt.hip: kTierANodes, the four-round scans' trip, kTierBNodes
K_SHORT, K_LONG = 24, 64
# world -> (cylinders, seed of np.random.default_rng: buildings first, then the rows); 0 cylinders: the stock world
WORLDS = {"stock": (0, 26), "c33": (33, 110), "c64": (64, 64)}

# the node cap: a harder world (48 cylinders, radius U(8, 22)) and rows whose tree reaches 2 048 nodes under 10 000 iterations
CAP_WORLD = (48, 275)
CAP_MAX_ITER, CAP_STREAM = 10000, 40000
CAP_ROW_SEEDS = (20, 43, 44)
# ... and rows of the same world that find a path from a tree of more than 1 280 nodes (two fit K = 24, one does not): the
# path walk through `parent` of a tree that deep is where a node list laid out for the wrong tier overlaps itself
# (320 nodes x 32 bytes = 1 280 doubles)
DEEP_ROW_SEEDS = (153, 578, 409)
DEEP_NODES = 1280


def cylinders(rng, nb, r_lo=5.0, r_hi=20.0):
    """x, y ~ U(0, 500), z = 0 (as the env tests), radius U(r_lo, r_hi), height U(10, 90)."""
    return np.c_[rng.uniform(0, 500, nb), rng.uniform(0, 500, nb), np.zeros(nb), rng.uniform(r_lo, r_hi, nb),
                 rng.uniform(10, 90, nb)]


def free_pair(rng, world):
    """A start in [10,210] x [1,10] and a goal in [330,490] x [420,490] (Agents/UAV.py:353-358), redrawn until the oracle's
    threaten_rate is 0 at both."""
    while True:
        s = np.array([rng.uniform(10, 210), rng.uniform(1, 10), 0.0])
        g = np.array([rng.uniform(330, 490), rng.uniform(420, 490), 0.0])
        if world.threaten_rate(*s) == 0 and world.threaten_rate(*g) == 0:
            return s, g


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(buildings [nb,5], start_goal [M,6], uniforms [M,STREAM])"""
    from oracle import pyoracle as po
    nb, seed = WORLDS[name]
    rng = np.random.default_rng(seed)
    b = load_golden("world_stock.npz")["buildings"] if nb == 0 else cylinders(rng, nb)
    world = po.OracleWorld(b)
    sg = np.array([np.r_[free_pair(rng, world)] for _ in range(M)])
    u = rng.random((M, STREAM))
    for a in (b, sg, u):
        a.setflags(write=False)
    return dict(buildings=b, start_goal=sg, uniforms=u)


def _plan(world, sg, u, max_iter, max_nodes):
    from oracle import pyoracle as po
    return po.rrt_get_path(world, po.OracleRng(0).replay(u), sg[:3], sg[3:], max_iter=max_iter, cap=NODE_CAP + 2,
                           max_nodes=max_nodes, want_nodes=True)


@functools.lru_cache(maxsize=None)
def oracle_plans(name):
    """The CPU oracle on inputs(name) -> (paths: list of [n,3], iters [M], nodes [M]); computed once per process."""
    from oracle import pyoracle as po
    d = inputs(name)
    world = po.OracleWorld(d["buildings"])
    out = [_plan(world, d["start_goal"][k], d["uniforms"][k], MAX_ITER, NODE_CAP) for k in range(M)]
    return [p for p, _, _ in out], np.array([i for _, i, _ in out]), np.array([n for _, _, n in out])


def cap_world():
    return cylinders(np.random.default_rng(CAP_WORLD[1]), CAP_WORLD[0], 8.0, 22.0)


def cap_row(world, seed):
    """Row of the node-cap test from its own seed -> (start_goal [6], uniforms [CAP_STREAM])"""
    rng = np.random.default_rng(seed)
    s, g = free_pair(rng, world)
    return np.r_[s, g], rng.random(CAP_STREAM)


@functools.lru_cache(maxsize=None)
def cap_rows():
    """CAP_ROW_SEEDS then DEEP_ROW_SEEDS -> dict(buildings, start_goal [R,6], uniforms [R,CAP_STREAM])"""
    from oracle import pyoracle as po
    b = cap_world()
    world = po.OracleWorld(b)
    rows = [cap_row(world, s) for s in CAP_ROW_SEEDS + DEEP_ROW_SEEDS]
    return dict(buildings=b, start_goal=np.array([sg for sg, _ in rows]), uniforms=np.array([u for _, u in rows]))


@functools.lru_cache(maxsize=None)
def cap_inputs():
    """cap_rows() and the capped oracle's results on them (max_nodes = 2 048): + iters [R], nodes [R], paths"""
    from oracle import pyoracle as po
    d = cap_rows()
    world = po.OracleWorld(d["buildings"])
    out = [_plan(world, sg, u, CAP_MAX_ITER, NODE_CAP) for sg, u in zip(d["start_goal"], d["uniforms"])]
    return dict(d, paths=[p for p, _, _ in out], iters=np.array([i for _, i, _ in out]), nodes=np.array([n for _, _, n in out]))


# ---- the device side (GPU tests and their child processes) -------------------------------------------------------------------
CANARY = -31337.25            # no coordinate of any world
PREFILL = -7                  # out_nsub / out_iters before the launch
TAIL = 64                     # canary rows behind row m - 1


def make_env(buildings, K):
    from dqn_based_uav_3d_path_planer_amd.env import VecPathPlanEnv
    return VecPathPlanEnv(4, buildings, max_subgoals=K)


def device_plan(env, m, *, start_goal=None, uniforms=None, seed=0, max_iter=MAX_ITER):
    """uavenv_rrt_plan through the C ABI into pre-filled outputs of m + TAIL rows
    -> dict(start_goal [m+TAIL,6], sub [m+TAIL,K,3], n_sub [m+TAIL], iters [m+TAIL]) as numpy arrays."""
    import torch
    from dqn_based_uav_3d_path_planer_amd import _lib
    dev = env.device
    sg_in = None if start_goal is None else torch.as_tensor(np.array(start_goal), dtype=torch.float64, device=dev)
    u = None if uniforms is None else torch.as_tensor(np.array(uniforms), dtype=torch.float64, device=dev)
    rows = m + TAIL
    sg = torch.full((rows, 6), CANARY, dtype=torch.float64, device=dev)
    sub = torch.full((rows, env.K, 3), CANARY, dtype=torch.float64, device=dev)
    ns = torch.full((rows,), PREFILL, dtype=torch.int32, device=dev)
    it = torch.full((rows,), PREFILL, dtype=torch.int32, device=dev)
    _lib.check(env.lib.uavenv_rrt_plan(env._h, int(m), None if sg_in is None else sg_in.data_ptr(),
                                       None if u is None else u.data_ptr(), 0 if u is None else u.shape[1], int(seed),
                                       int(max_iter), 30.0, 5.0, sg.data_ptr(), sub.data_ptr(), ns.data_ptr(), it.data_ptr(),
                                       env._stream()), "uavenv_rrt_plan")
    torch.cuda.synchronize(dev)
    return dict(start_goal=sg.cpu().numpy(), sub=sub.cpu().numpy(), n_sub=ns.cpu().numpy(), iters=it.cpu().numpy())
