"""The CPU oracle's capped planner (oracle/uav_oracle.c: orc_rrt_get_path_n), the independent side of tests/test_rrt_forms_gpu.py:
  * without a cap it is orc_rrt_get_path, which test_oracle_golden.py pins to the executed reference, on the 44 golden resets;
  * with the GPU planner's cap of 2 048 nodes a tree that reaches the cap ends with [goal] at the iteration it stopped at;
  * the inputs of tests/rrt_forms_inputs.py cover what the GPU tests rely on (asserted here from the oracle alone)."""
import numpy as np
import pytest

import rrt_forms_inputs as ri
from conftest import load_golden
from oracle import pyoracle as po


def test_uncapped_form_is_the_plain_planner_on_the_golden_resets(world_npz):
    g = load_golden("resets.npz")
    world = po.OracleWorld(world_npz["buildings"])
    for k, seed in enumerate(g["seeds"]):
        plans = []
        for kw in ({}, dict(want_nodes=True), dict(max_nodes=10002, want_nodes=True)):
            r = po.OracleRng(int(seed))
            r.uniform(0, 2 * np.pi)                                               # the heading draw of UAV.reset
            s = [r.uniform(10, 210), r.uniform(1, 10), 0.0]
            t = [r.uniform(330, 490), r.uniform(420, 490), 0.0]
            plans.append(po.rrt_get_path(world, r, s, t, **kw) + (r.random(),))    # (the stream ends at the same draw)
        (p0, i0, u0), (p1, i1, n1, u1), (p2, i2, n2, u2) = plans
        assert np.array_equal(p0, g["sub_goals"][k][: g["n_sub"][k]]) and len(p0) == g["n_sub"][k], seed
        assert np.array_equal(p0, p1) and np.array_equal(p0, p2) and i0 == i1 == i2 and u0 == u1 == u2 and n1 == n2, seed
        assert len(p0) - 1 <= n1 <= i0 + 1, seed                # every path node but the goal is a tree node; a node per iteration at most


def test_a_tree_that_reaches_the_node_cap_gives_up_where_it_stopped():
    d = ri.cap_inputs()
    nc = len(ri.CAP_ROW_SEEDS)
    assert nc >= 2 and len(ri.DEEP_ROW_SEEDS) >= 2 and np.all(4 * d["iters"] <= ri.CAP_STREAM)
    for k in range(nc):                                         # the cap ended the loop: iterations were left
        assert d["nodes"][k] == ri.NODE_CAP and d["iters"][k] < ri.CAP_MAX_ITER
        assert np.array_equal(d["paths"][k], d["start_goal"][k][None, 3:])          # [goal]
    n = np.array([len(p) for p in d["paths"][nc:]])
    assert np.all((d["nodes"][nc:] > ri.DEEP_NODES) & (d["nodes"][nc:] < ri.NODE_CAP)) and np.all(n >= 2)
    assert (n <= ri.K_SHORT).sum() >= 1 and (n > ri.K_SHORT).sum() >= 1


@pytest.mark.parametrize("name", list(ri.WORLDS))
def test_inputs_cover_every_form_of_the_planner(name):
    d = ri.inputs(name)
    paths, iters, nodes = ri.oracle_plans(name)
    world = po.OracleWorld(d["buildings"])
    assert len(d["buildings"]) == (ri.WORLDS[name][0] or 26) and d["start_goal"].shape == (ri.M, 6)
    assert world.threaten_rate_many(d["start_goal"].reshape(-1, 3)).sum() == 0
    assert iters.max() <= ri.MAX_ITER and nodes.max() < ri.NODE_CAP and 4 * ri.MAX_ITER <= ri.STREAM
    assert np.all(nodes <= iters + 1)
    n = np.array([len(p) for p in paths])
    print(name, "trees above tier A:", int((nodes > ri.TIER_A).sum()), "in the scans' second trip only:",
          int(((nodes > ri.SCAN) & (nodes <= ri.TIER_A)).sum()), "give up:", int((n == 1).sum()), "longer than 24:",
          int((n > ri.K_SHORT).sum()), "fit 24:", int(((n >= 2) & (n <= ri.K_SHORT)).sum()), "longest:", int(n.max()))
    if len(d["buildings"]) > 32:                               # the uint64_t mask worlds
        assert (nodes > ri.TIER_A).sum() >= 8
    assert (n > ri.K_SHORT).sum() >= 20 and ((n >= 2) & (n <= ri.K_SHORT)).sum() >= 20
    assert n.max() <= ri.K_LONG                                # every path fits the K = 64 env
    assert np.all(iters[n == 1] == ri.MAX_ITER)                # giving up is running out of iterations here


def test_inputs_cover_the_second_scan_trip_and_giving_up():
    second = giveup = 0
    for name in ri.WORLDS:
        paths, iters, nodes = ri.oracle_plans(name)
        second += int(((nodes > ri.SCAN) & (nodes <= ri.TIER_A)).sum())
        giveup += sum(len(p) == 1 for p in paths)
    assert second >= 3 and giveup >= 2
