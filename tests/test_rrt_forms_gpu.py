"""Every launch form and mask width of the sub-goal planner (csrc/rrt.hip, k_rrt_plan) against the CPU oracle's capped planner
(oracle/uav_oracle.c: orc_rrt_get_path_n, pinned to the executed reference by tests/test_rrt_ref.py and test_oracle_golden.py).
Inputs: tests/rrt_forms_inputs.py (the stock world with uint32_t masks, 33 and 64 random cylinders with uint64_t masks; 192
explicit rows each; tests/test_rrt_ref.py asserts on the CPU that they reach tier B, the second trip of the 256-node scans,
giving up, and paths on both sides of K = 24).  All calls go through the C ABI into outputs pre-filled with a canary (-7 for
n_sub and iters) and 64 canary rows behind the last one.

  (a) test_default_launch_matches_the_oracle: tier A then tier B, K = 64 and K = 24, all three worlds.
  (b) test_every_launch_form_gives_the_same_bits: UAVENV_RRT_TIER_A=2048 / =16 / UAVENV_RRT_BACKGROUND=64 against no knob, each in a
      fresh child (the knobs are read once per process), explicit streams (the 64-cylinder rows, the rows of (c)) and Philox
      mode: bit for bit the same outputs.
  (c) test_node_cap: rows whose tree reaches 2 048 nodes end with [goal] at the capped oracle's iteration; rows that find
      their path from a tree of more than 1 280 nodes.

Forks.  The device's f64 square root is faithfully, not correctly, rounded, and every steered node sits one step from its
parent to within an ulp, so `int(d / 5)` and `d < step` can be decided by the last bit in any row: a row that differs from
the oracle is counted against a cap (3 % of a world's rows, the share test_rrt_gpu.py allows), never excused by a near-tie
rule, and must still be a valid plan.  Measured on an MI355X (rows of 192 that differ from the oracle; rows whose oracle tree
is above 320 nodes, agreeing / all), the same for K = 64 and K = 24:
    stock  0 differ,  2 /  2
    c33    0 differ, 15 / 15
    c64    0 differ, 17 / 17
and in (c) all six rows agree (iterations 4469, 4374, 4372 at the cap; 3764, 4265, 4387 for the deep trees).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import rrt_forms_inputs as ri

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9               # f64; pow(x, 2) vs x * x and OCML vs glibc arithmetic differ in the last ulp (as tests/test_rrt_gpu.py)
MAX_FORK_SHARE = 0.03
STEP, OBSTACLE_STEP = 30.0, 5.0


def _hop_is_free(world, a, b):
    """RRT.obstacle_free's sample points (RRT.py:48-56) under the oracle's threaten_rate.  The number of points is
    int(d / 5) + 1 with d one sqrt away from a multiple of 5 for every steered hop, so where d / 5 is within 1e-9 of an
    integer the device may have tested either count: the hop is free if one of the two sets is."""
    d = float(np.sqrt(((a - b) ** 2).sum()))
    q = d / OBSTACLE_STEP
    counts = {int(q)}
    if abs(q - round(q)) <= 1e-9:
        counts |= {int(round(q)) - 1, int(round(q))}
    for steps in counts:
        if steps < 0:
            continue
        pts = np.array([a + (b - a) * i / (steps + 1) for i in range(steps + 1)])
        if world.threaten_rate_many(pts).sum() == 0:
            return True
    return False


def _check_call(out, m, K, sg_in, max_iter):
    """What holds for every row of every call, whatever the tree: each row written once and inside its own
    slot, nothing behind row m - 1."""
    sg, sub, ns, it = out["start_goal"], out["sub"], out["n_sub"], out["iters"]
    assert np.all(sg[m:] == ri.CANARY) and np.all(sub[m:] == ri.CANARY) and np.all(ns[m:] == ri.PREFILL) and np.all(it[m:] == ri.PREFILL)
    assert np.all(ns[:m] != ri.PREFILL) and np.all(it[:m] != ri.PREFILL)
    if sg_in is not None:
        assert np.array_equal(sg[:m], sg_in)
    assert np.all((it[:m] >= 1) & (it[:m] <= max_iter))
    flat = sub.reshape(len(sub), -1)
    for k in range(m):
        if ns[k] < 0:
            assert -ns[k] > K and np.all(flat[k] == ri.CANARY), k                  # does not fit: the row is left alone
        else:
            assert 1 <= ns[k] <= K and not np.any(flat[k, : 3 * ns[k]] == ri.CANARY), k
            assert np.all(flat[k, 3 * ns[k]:] == 0.0) and not np.any(np.signbit(flat[k, 3 * ns[k]:])), k      # exact zero fill
            assert np.array_equal(sub[k, ns[k] - 1], sg[k, 3:]), k                  # ends at the goal


def _valid_plan(world, out, k, max_iter):
    """A row that differs from the oracle must still be a plan: start .. goal in hops of at most one step, every planned
    hop obstacle-checked (the last one, node -> goal, is not checked by the reference either: RRT.py:92-94)."""
    ns, it = int(out["n_sub"][k]), int(out["iters"][k])
    if not 1 <= it <= max_iter:
        return False
    if ns < 0:
        return True                                  # too long for this K: only its length is reported
    p = out["sub"][k, :ns]
    if ns == 1:
        return it == max_iter and np.array_equal(p[0], out["start_goal"][k, 3:])       # gave up: [goal]
    if not (np.array_equal(p[0], out["start_goal"][k, :3]) and np.array_equal(p[-1], out["start_goal"][k, 3:])):
        return False
    if np.linalg.norm(np.diff(p, axis=0), axis=1).max() > STEP + 1e-9:
        return False
    return all(_hop_is_free(world, p[i], p[i + 1]) for i in range(ns - 2))


def _compare_with_oracle(name, out, K):
    """-> (rows that differ from the oracle, rows above tier A that agree, rows above tier A)"""
    paths, o_it, o_nodes = ri.oracle_plans(name)
    ns, it, sub = out["n_sub"], out["iters"], out["sub"]
    differ = []
    for k in range(ri.M):
        n = len(paths[k])
        same = it[k] == o_it[k] and ns[k] == (n if n <= K else -n)
        if same and n <= K:
            same = np.abs(sub[k, :n] - paths[k]).max() <= TOL
        if not same:
            differ.append(k)
    long_rows = np.nonzero(o_nodes > ri.TIER_A)[0]
    return differ, [k for k in long_rows if k not in differ], long_rows


@pytest.mark.parametrize("K", [ri.K_LONG, ri.K_SHORT])
@pytest.mark.parametrize("name", list(ri.WORLDS))
def test_default_launch_matches_the_oracle(name, K):
    """(a)"""
    from oracle import pyoracle as po
    d = ri.inputs(name)
    paths, o_it, o_nodes = ri.oracle_plans(name)
    env = ri.make_env(d["buildings"], K)
    try:
        out = ri.device_plan(env, ri.M, start_goal=d["start_goal"], uniforms=d["uniforms"])
    finally:
        env.close()
    _check_call(out, ri.M, K, d["start_goal"], ri.MAX_ITER)
    differ, long_same, long_rows = _compare_with_oracle(name, out, K)
    print(f"{name} K={K}: {len(differ)} of {ri.M} rows differ from the oracle: "
          + ", ".join(f"row {k} (oracle n={len(paths[k])} it={o_it[k]} nodes={o_nodes[k]}; device n={out['n_sub'][k]} it={out['iters'][k]})"
                      for k in differ) + f"; rows above tier A: {len(long_same)} of {len(long_rows)} agree")
    # rows that agree carry the oracle's edges: giving up is [goal] with n = 1, a path longer than K is -needed
    for k in range(ri.M):
        if k in differ:
            continue
        n = len(paths[k])
        if n == 1:
            assert out["n_sub"][k] == 1 and np.array_equal(out["sub"][k, 0], d["start_goal"][k, 3:]) and out["iters"][k] == ri.MAX_ITER
        if n > K:
            assert out["n_sub"][k] == -n
    world = po.OracleWorld(d["buildings"])
    for k in differ:
        assert _valid_plan(world, out, k, ri.MAX_ITER), f"row {k} differs from the oracle and is not a valid plan"
    assert len(differ) <= MAX_FORK_SHARE * ri.M, f"{len(differ)} of {ri.M} rows differ from the oracle: {differ}"
    if len(d["buildings"]) > 32:
        assert len(long_same) >= 8, f"only {len(long_same)} of the {len(long_rows)} rows above tier A agree with the oracle"


# --- (b) the launch forms: the knobs are read once per process, so each runs in a fresh child, one at a time, under its own time
# limit; a child that fails ends the test
FORMS = {"single_tier": {"UAVENV_RRT_TIER_A": "2048"}, "tier_a_16": {"UAVENV_RRT_TIER_A": "16"},
         "background": {"UAVENV_RRT_BACKGROUND": "64"}}
PHILOX_M, PHILOX_SEED, PHILOX_MAX_ITER = 512, 23, 10000
FIELDS = ("start_goal", "n_sub", "iters", "sub")
CHILD = r"""
import os, sys
root, dest = sys.argv[1:3]
sys.path[:0] = [root, os.path.join(root, "tests")]
import numpy as np
import rrt_forms_inputs as ri
res = {}
d = ri.inputs("c64")
for K in (ri.K_LONG, ri.K_SHORT):
    env = ri.make_env(d["buildings"], K)
    for key, v in ri.device_plan(env, ri.M, start_goal=d["start_goal"], uniforms=d["uniforms"]).items():
        res[f"explicit{K}/{key}"] = v
    env.close()
d = ri.cap_rows()
env = ri.make_env(d["buildings"], ri.K_SHORT)
for key, v in ri.device_plan(env, len(d["start_goal"]), start_goal=d["start_goal"], uniforms=d["uniforms"], max_iter=ri.CAP_MAX_ITER).items():
    res[f"cap/{key}"] = v
env.close()
m, seed, max_iter = (int(x) for x in sys.argv[3:6])
for name in ("stock", "c64"):
    env = ri.make_env(ri.inputs(name)["buildings"], ri.K_SHORT)
    for key, v in ri.device_plan(env, m, seed=seed, max_iter=max_iter).items():
        res[f"philox_{name}/{key}"] = v
    env.close()
np.savez(dest, **res)
"""


def _run_form(knobs, dest):
    """The calls of CHILD in a fresh process under `knobs` -> {call: outputs}; every row of every call written once, in place."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("UAVENV_")}
    env.update(knobs)
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, ROOT, str(dest), str(PHILOX_M), str(PHILOX_SEED),
                    str(PHILOX_MAX_ITER)], env=env, check=True, timeout=150)
    with np.load(dest) as z:
        got = {k: z[k] for k in z.files}
    c64, cap = ri.inputs("c64")["start_goal"], ri.cap_rows()["start_goal"]
    calls = [(f"explicit{ri.K_LONG}", ri.M, ri.K_LONG, c64, ri.MAX_ITER), (f"explicit{ri.K_SHORT}", ri.M, ri.K_SHORT, c64, ri.MAX_ITER),
             ("cap", len(cap), ri.K_SHORT, cap, ri.CAP_MAX_ITER),
             ("philox_stock", PHILOX_M, ri.K_SHORT, None, PHILOX_MAX_ITER), ("philox_c64", PHILOX_M, ri.K_SHORT, None, PHILOX_MAX_ITER)]
    outs = {}
    for call, m, K, sg_in, max_iter in calls:
        outs[call] = {k: got[f"{call}/{k}"] for k in FIELDS}
        _check_call(outs[call], m, K, sg_in, max_iter)
    return outs


@pytest.fixture(scope="module")
def default_form(tmp_path_factory):
    return _run_form({}, tmp_path_factory.mktemp("rrt_forms") / "default.npz")


def test_default_form_in_a_child_is_the_launch_held_to_the_oracle(default_form):
    """(b) The reference side of the comparison below is what (a) and (c) check, and its Philox calls draw what they should."""
    differ, long_same, _ = _compare_with_oracle("c64", default_form[f"explicit{ri.K_LONG}"], ri.K_LONG)
    assert len(differ) <= MAX_FORK_SHARE * ri.M and len(long_same) >= 8
    d = ri.cap_inputs()
    nc = len(ri.CAP_ROW_SEEDS)
    assert np.array_equal(default_form["cap"]["iters"][:nc], d["iters"][:nc]) and np.all(default_form["cap"]["n_sub"][:nc] == 1)
    for name in ("stock", "c64"):
        ns, sg = default_form[f"philox_{name}"]["n_sub"][:PHILOX_M], default_form[f"philox_{name}"]["start_goal"][:PHILOX_M]
        assert np.all((sg[:, 0] >= 10) & (sg[:, 0] <= 210) & (sg[:, 1] >= 1) & (sg[:, 1] <= 10) & (sg[:, 2] == 0))
        assert np.all((sg[:, 3] >= 330) & (sg[:, 3] <= 490) & (sg[:, 4] >= 420) & (sg[:, 4] <= 490) & (sg[:, 5] == 0))
        assert ((ns >= 2) & (ns <= ri.K_SHORT)).mean() > 0.5                # (a sanity bound: most rows get a path that fits in four attempts)


@pytest.mark.parametrize("form", list(FORMS))
def test_every_launch_form_gives_the_same_bits(form, default_form, tmp_path):
    """(b) No tolerance and no cap: the single tier, a 16-node tier A (nearly every row goes through `flagged` to tier B) and the
    LDS-free background form write what the default launch writes (sub: the whole array, zero fill and untouched rows included)."""
    outs = _run_form(FORMS[form], tmp_path / f"{form}.npz")
    for call, ref in default_form.items():
        for k in FIELDS:
            assert np.array_equal(outs[call][k], ref[k]), (form, call, k)


def _cap_agrees(out, d, k):
    n = len(d["paths"][k])
    if out["iters"][k] != d["iters"][k] or out["n_sub"][k] != (n if n <= ri.K_SHORT else -n):
        return False
    return n > ri.K_SHORT or np.abs(out["sub"][k, :n] - d["paths"][k]).max() <= TOL


def test_node_cap():
    """(c) A tree that reaches 2 048 nodes: tier A defers it, tier B stops at the cap -> [goal], n = 1, the capped oracle's
    iteration count (the reference, without a cap, would go on).  The rows behind them find a path from a tree of 1 762 to
    1 985 nodes -- the path walk of a nearly full node list -- and are held to the oracle the same way."""
    d = ri.cap_inputs()
    m, nc = len(d["iters"]), len(ri.CAP_ROW_SEEDS)
    assert nc >= 2 and np.all(d["nodes"][:nc] == ri.NODE_CAP)
    env = ri.make_env(d["buildings"], ri.K_SHORT)
    try:
        out = ri.device_plan(env, m, start_goal=d["start_goal"], uniforms=d["uniforms"], max_iter=ri.CAP_MAX_ITER)
    finally:
        env.close()
    print("node cap: device iters", out["iters"][:m], "oracle iters", d["iters"], "device n_sub", out["n_sub"][:m],
          "oracle path lengths", [len(p) for p in d["paths"]])
    _check_call(out, m, ri.K_SHORT, d["start_goal"], ri.CAP_MAX_ITER)
    assert np.all(out["n_sub"][:nc] == 1)
    assert np.array_equal(out["sub"][:nc, 0], d["start_goal"][:nc, 3:])
    assert np.array_equal(out["iters"][:nc], d["iters"][:nc])
    for k in range(nc, m):
        assert _cap_agrees(out, d, k), k
