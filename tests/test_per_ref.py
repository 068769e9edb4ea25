"""oracle/per_oracle.py's restatement of the UavPer contract (include/uavenv.h) on the CPU: against the executed reference
(tests/golden/per.npz), against the tree restatement (PerOracle), against rational arithmetic -- and the resolving power of
the assertions tests/test_per_frame_kernels_gpu.py applies to the device (tests/per_frame_fixtures.py): each of them has to
reject an oracle with one plausible kernel bug in it."""
from fractions import Fraction

import numpy as np
import pytest

import per_frame_fixtures as fx
from conftest import load_golden
from oracle.per_oracle import (PerOracle, batch_update_seq, decided, exact_sums, in_order, is_weights, leaf_rotation, ring_fill,
                               sample_by_cumsum)


def test_is_weights_reproduces_the_reference_weights():
    g = load_golden("per.npz")
    for ci in range(4):
        pre = f"c{ci}_"
        cap = int(g[pre + "capacity"])
        for r in range(3):
            p = g[pre + "prio"][g[pre + f"r{r}_tree_idx"] - (cap - 1)]
            w = is_weights(p, int(g[pre + "n_entries"]), float(g[pre + "total"]), float(g[pre + f"r{r}_beta"]))
            assert np.allclose(w, g[pre + f"r{r}_weights"], rtol=1e-12, atol=0) and w.max() == 1.0


def test_is_weights_rules():
    p = np.array([0.5, 0.0, 0.25, 2.0])
    w = is_weights(p, 10, 7.9, 0.4)
    assert w[1] == 0.0 and w[2] == 1.0 and np.array_equal(w, is_weights(p, 10, 7.0, 0.4))             # int(total)
    assert np.array_equal(is_weights(p, 10, 0.3, 0.4, normalise=False), is_weights(p, 10, 1.0, 0.4, normalise=False))
    assert w[0] == pytest.approx((10 * 0.5 / 7) ** -0.4 / (10 * 0.25 / 7) ** -0.4, rel=1e-15)
    assert np.array_equal(is_weights(p, 10, 7.9, 0.0), [1.0, 0.0, 1.0, 1.0])
    z = is_weights(np.zeros(5), 10, 7.9, 0.4)
    assert np.array_equal(z, np.zeros(5))                                                              # no 0 / 0


def test_batch_update_seq_reproduces_the_reference_priorities():
    g = load_golden("per.npz")
    for ci in range(4):
        pre = f"c{ci}_"
        cap, n_push = int(g[pre + "capacity"]), int(g[pre + "n_push"])
        # push (:143): no clip, empty leaves are written.  ReplayTree.push raises with Python's pow, batch_update with numpy's --
        # an ulp apart on a few operands, hence the bar the device's pow is held to; the batch_update below is bit for bit
        pushed = batch_update_seq(np.zeros(cap), np.arange(n_push) % cap, g[pre + "errors"], 0.01, 0.6, 0.0)
        assert np.allclose(pushed, g[pre + "prio_after_push"], rtol=fx.POW_RTOL, atol=0) and (pushed > 0).sum() == min(n_push, cap)
        got = batch_update_seq(g[pre + "prio_after_push"], g[pre + "upd_data"], g[pre + "upd_err"], 0.01, 0.6, 1.0)
        assert np.array_equal(got, g[pre + "prio"])


def test_batch_update_seq_rules():
    prio = np.array([0.5, 0.0, 0.25, 0.0])
    got = batch_update_seq(prio, [0, 0, 0, -1, 4, 1, 2], [0.1, 0.2, -0.3, 9.0, 9.0, 0.5, 5.0], 0.01, 0.6, 1.0)
    assert got[0] == pytest.approx(0.31 ** 0.6, rel=4e-16) and got[0] != pytest.approx(0.21 ** 0.6, rel=0.01)   # last of the run, |error|
    assert got[1] == 0.0 and got[3] == 0.0              # an empty leaf stays empty under a clip; slots -1 and 4 are nobody's
    assert got[2] == 1.0                                # clipped
    push = batch_update_seq(prio, [1, 2], [0.0, 5.0], 0.01, 0.6, 0.0)
    assert push[1] == pytest.approx(0.01 ** 0.6, rel=4e-16) and push[2] == pytest.approx(5.01 ** 0.6, rel=4e-16)   # empty leaves written
    assert prio[1] == 0.0                                                                                         # the input is not touched


def test_ring_fill_agrees_with_the_tree_on_a_rot0_tree():
    cap, n = 64, 16
    assert leaf_rotation(cap) == 0
    o = PerOracle(cap)
    rng = np.random.default_rng(2)
    for e in rng.uniform(0.0, 3.0, cap):
        o.push(e)
    flat = o.priorities()
    for t in range(9):                                  # wraps the 4-frame ring twice
        first, retire = fx.frame_ranges(cap // n, n, t)
        assert o.ptr == first
        for _ in range(n):
            o.push(0.0)                                 # ReplayTree.push(error 0) per transition of the frame
        for s in range(retire, retire + n):
            o._set_leaf(s + cap - 1, 0.0)
        flat = ring_fill(flat, first, n, (0.0 + 0.01) ** 0.6, None, 1, retire)
        assert np.array_equal(flat, o.priorities())


def test_ring_fill_rules():
    prio = np.arange(1.0, 13.0)
    plane = np.array([1, 0, 0, 0, 0, 9, 0, 0, 255, 0, 0, 0], dtype=np.uint8)
    got = ring_fill(prio, 3, 3, 0.5, plane, 4, 9)
    assert np.array_equal(got, [1, 2, 3, 0.5, 0.0, 0.5, 7, 8, 9, 0, 0, 0])
    assert np.array_equal(ring_fill(prio, 3, 3, 0.5, plane[1:], 4, 9)[3:6], [0.0, 0.5, 0.0])        # another slot's column
    assert np.array_equal(ring_fill(prio, 9, 3, 0.5, None, 1, 0), [0, 0, 0, 4, 5, 6, 7, 8, 9, 0.5, 0.5, 0.5])
    assert np.array_equal(ring_fill(prio, 3, 0, 0.5, plane, 4, 9), prio) and prio[3] == 4.0


@pytest.mark.parametrize("cap", [1, 5, 333, 1024, 1025, 4200])
def test_exact_sums_are_the_rational_sums_rounded_once(cap):
    prio = fx.initial_prio(cap)
    for rot in (0, leaf_rotation(cap)):
        ex = exact_sums(prio, rot)
        x = [Fraction(v) for v in in_order(prio, rot)]
        n_chunks = (cap + 1023) // 1024
        assert len(ex["chunk"]) == n_chunks and len(ex["group"]) == 64 * n_chunks and len(ex["prefix"]) == n_chunks + 1
        for b in range(n_chunks):
            assert ex["chunk"][b] == float(sum(x[b * 1024:(b + 1) * 1024]))
            assert ex["prefix"][b] == float(sum(x[:b * 1024]))
        assert ex["prefix"][-1] == float(sum(x))
        for k in range(0, 64 * n_chunks, 7):
            assert ex["group"][k] == float(sum(x[k * 16:(k + 1) * 16]))
    assert in_order(np.arange(5.0), 3).tolist() == [3, 4, 0, 1, 2]


def test_decided_is_the_distance_to_the_nearest_leaf_edge():
    prio = np.array([1.0, 0.0, 2.0, 0.5])
    d = decided(prio, 0, [0.5, 1.0, 1.0 + 1e-9, 2.9999, 3.0 - 1e-13, 3.2, 3.5, 1e-13], 1e-12)
    assert d.tolist() == [True, False, True, True, False, True, False, False]
    assert decided(prio, 2, [2.0 + 1e-9], 1e-12).tolist() == [True] and decided(prio, 2, [2.5], 1e-12).tolist() == [False]


@pytest.mark.parametrize("geom", fx.GEOMS)
def test_the_selection_inputs_leave_no_draw_undecided(geom):
    """What (c) of the device module relies on: with its inputs (the frame-1 fill on the initial priorities, stratified draws)
    no draw lies within the margin of a leaf edge -- the at-most-one allowance is never used up."""
    F, n, U = geom
    cap = F * n
    prio = fx.selection_case(F, n, U)[-1]
    for rotated in (False, True):
        rot = fx.rotation(cap, rotated)
        total = exact_sums(prio, rot)["prefix"][-1]
        rng = np.random.default_rng([41, cap, rot])
        for rep in range(20):
            for batch in (1, 255, 257, 1000):
                draws = fx.stratified_draws(total, batch, rng)
                assert decided(prio, rot, draws, fx.selection_margin(cap, total)).all(), (geom, rot, rep, batch)
                assert (prio[sample_by_cumsum(prio, None, draws, rot=rot)] > 0).all()


def test_set_case_keeps_the_precondition_and_holds_every_edge():
    prio, slots, err = fx.set_case(5000, 700)
    seen = {}
    for i, s in enumerate(slots.tolist()):
        assert s not in seen or seen[s] == i - 1, (i, s)            # equal entries are adjacent
        seen[s] = i
    assert len(set(slots[254:259].tolist())) == 1 and len(set(err[254:259].tolist())) == 5
    assert (slots < 0).sum() == 3 and (slots >= 5000).sum() == 3
    ok = (slots >= 0) & (slots < 5000)
    assert (prio[slots[ok]] == 0.0).sum() > 20 and (err > 1.0).any() and (err == 0.0).any() and (err < 0.0).any()
    for clip in (1.0, 0.0):
        want = batch_update_seq(prio, slots, err, 0.01, 0.6, clip)
        assert fx.check_set(want, prio, slots, err, 0.01, 0.6, clip) == 0.0
        assert fx.rejects(fx.check_set, want, prio, slots, err, 0.01, 0.6, clip, fx.PERTURBED["first of a run wins"])
        empty = slots[ok][prio[slots[ok]] == 0.0]
        assert ((want[empty] == 0.0).all() if clip > 0 else (want[empty] > 0.0).all())


def test_resolving_power_of_the_frame_assertions():
    fx.resolving_power_frames()


def test_resolving_power_of_the_weight_assertions():
    fx.resolving_power_weights()


def test_resolving_power_of_the_state_machine_assertions():
    hits = fx.resolving_power_passes()
    assert len(hits) == 11 and all(h >= 1 for h in hits.values()), hits
