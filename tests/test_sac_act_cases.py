"""The host side of tests/test_sac_act_kernels_gpu.py, without a GPU: the case table against the launch rule of
uavenv_sac_act_multi (oracle.sac_grad_ref.act_launch_map), and the mutants of (e) on made-up observation rows -- every mutant
that applies to a case is told from the original by more than the two bars, the unmutated side by nothing."""
import numpy as np

import test_sac_act_kernels_gpu as T
from oracle.sac_grad_ref import HID, PA, W, act_bar, act_launch_map


def test_the_case_table_is_what_the_launch_rule_gives():
    T.check_case_table()
    assert len(T.CASES) == 9 and sorted({c[0] for c in T.CASES}) == [1, 2, 3, 4, 5, 8]
    for n in range(1, 9):                                  # the thresholds of the second trip: 32 768 agents for one slot, 8 192 for four
        gx = 512 // n
        assert act_launch_map(n, 64 * gx)["trips"] == 1 and act_launch_map(n, 64 * gx + 1)["trips"] == 2
    assert 64 * (512 // 1) == 32768 and 64 * (512 // 4) == 8192


def made_up(rng, rows=4096):
    """Rows with the packed layout's shape (11 + 4 floats, 80 flags, 5 zero columns) and eight small random actors."""
    X = np.zeros((rows, W), dtype=np.float32)
    X[:, :11] = rng.normal(0, 1, (rows, 11))
    X[:, 11:86] = rng.random((rows, 75)) < 0.2
    X[:, 86:90] = rng.normal(0, 1, (rows, 4))
    X[:, 90:95] = rng.random((rows, 5)) < 0.5
    k = 1.0 / np.sqrt(W)
    flats = [rng.uniform(-k, k, PA).astype(np.float32) for _ in range(8)]
    for f in flats:
        f[HID * W + HID:] *= np.sqrt(W / HID)
    return X, flats


def test_the_mutants_are_told_apart_on_made_up_rows():
    rng = np.random.default_rng(3)
    X, flats = made_up(rng)
    for n, count, trips, _, _, s0 in T.CASES:
        inp = T.Inputs(n, count, s0, rows=X, flats=flats)
        res = inp.mutants()
        assert ("rows one trip back" in res) == (trips > 1) and ("next slot's actor" in res) == (n >= 2)
        assert ("clamp one short" in res) == (count >= 2) and "draws swapped" in res
        assert all(v > 1.0 for v in res.values()), (n, count, res)
        for j in range(n):                                 # the unmutated head, rebuilt the way the mutants are, is the original
            d = T.rehead(inp.hd[j], np.arange(count), inp.eps[j])
            assert np.array_equal(d["act"], inp.hd[j]["act"])
            assert np.array_equal(act_bar(d, T.TAU_TD, T.U), act_bar(inp.hd[j], T.TAU_TD, T.U))
