"""Inputs, bars and assertions shared by tests/test_per_ref.py (host) and tests/test_per_frame_kernels_gpu.py (device): the
hand-built valid planes and errors, and every comparison of a result with oracle/per_oracle.py.  The assertions take plain
numpy arrays and the oracle functions as arguments, so the host tests can feed them a PERTURBED oracle and require a rejection
(resolving power) -- the same code then judges what the device returns.  Nothing here touches a device."""
from types import SimpleNamespace

import numpy as np

from oracle import philox as px
from oracle.per_oracle import (CHUNK, batch_update_seq, decided, exact_sums, is_weights, leaf_rotation, ring_fill,
                               sample_by_cumsum)

U53 = 2.0 ** -53
POW_RTOL = 4e-16                 # OCML pow against glibc pow on the same operands: the project's bar (tests/test_per_gpu.py)
EPSILON, ALPHA, CLIP = 0.01, 0.6, 1.0
SENTINEL = -777.25               # behind every device array; never a priority, a sum or a weight

# (frames F, rows per frame n, valid stride U); capacity F * n
GEOMS = [(7, 600, 1), (5, 1023, 1), (4, 1025, 1), (9, 37, 4), (3, 1, 1), (2, 2500, 1), (65, 1000, 1)]

ORACLE = SimpleNamespace(fill=ring_fill, weights=is_weights, update=batch_update_seq)


def rotation(capacity, rotated):
    return leaf_rotation(capacity) if rotated else 0


def initial_prio(capacity, seed=11):
    """uniform ** 3 (six decades of magnitudes: the order of a sum matters), a quarter of the leaves at 0."""
    rng = np.random.default_rng([seed, capacity])
    p = rng.uniform(0.0, 1.0, capacity) ** 3
    p[rng.permutation(capacity)[:capacity // 4]] = 0.0
    return p


def valid_plane(n, U, t, seed=23, p_valid=0.75):
    """One frame's valid plane, n rows of U flags: 0 = invalid, anything else (1, 7, 255) = valid."""
    rng = np.random.default_rng([seed, n, U, t])
    flags = rng.choice(np.array([1, 1, 7, 255], dtype=np.uint8), n * U)
    flags[rng.uniform(0.0, 1.0, n * U) >= p_valid] = 0
    return flags


def fill_value(t):
    """A priority that names its pass: a frame filled at the wrong pass, or left behind, carries the wrong bits."""
    return (EPSILON + 0.125 * t) ** ALPHA


def frame_ranges(F, n, t):
    """-> (first, retire_first): pass t writes frame t % F and retires the frame that became the ring's head."""
    return (t % F) * n, ((t + 1) % F) * n


# ------------------------------------------------------------------------------------------------ assertions
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_frame(got_prio, before, first, count, value, valid, valid_stride, retire_first, orc=ORACLE, what=None):
    """(a): the priorities after a fill/retire equal the oracle's bit for bit -- values are copied, not computed; that covers
    the slots outside the two ranges, which the oracle leaves alone."""
    want = orc.fill(before, first, count, value, valid, valid_stride, retire_first)
    assert same_bits(got_prio, want), (what, np.flatnonzero(np.asarray(got_prio) != want)[:8])
    return want


def prefix_additions(n_chunks):
    """The longest addition chain behind a chunk_prefix entry: k_per_prefix splits the chunks over 256 threads, `per` each --
    at most `per` additions for a thread's own sum, 255 for the running sum over the threads, `per` again along its chunks."""
    per = (n_chunks + 255) // 256
    return 2 * per + 255


def check_sums(prio, rot, chunk_sum, chunk_prefix, group_sum, what=None):
    """(b): the device's sums against the exact sums of the device's own priorities.  Priorities are non-negative, so the sum
    of the operands' magnitudes IS the exact sum.  -> the worst error / bar ratio of each family."""
    ex = exact_sums(prio, rot)
    n_chunks = len(ex["chunk"])
    assert len(chunk_sum) == n_chunks and len(chunk_prefix) == n_chunks + 1 and len(group_sum) == n_chunks * 64, what
    worst = {}
    for name, got, want, bar in (
            ("group_sum", group_sum, ex["group"], 15 * U53 * ex["group"]),
            ("chunk_sum", chunk_sum, ex["chunk"], 11 * U53 * ex["chunk"]),
            ("chunk_prefix", chunk_prefix, ex["prefix"],
             prefix_additions(n_chunks) * U53 * ex["prefix"][-1] + 11 * U53 * ex["prefix"])):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        bad = np.flatnonzero(~(err <= bar))
        assert bad.size == 0, (what, name, bad[:4], err[bad[:4]], bar[bad[:4]])
        nz = bar > 0
        worst[name] = float((err[nz] / bar[nz]).max()) if nz.any() else 0.0
    assert chunk_prefix[0] == 0.0 and not np.signbit(chunk_prefix[0]), what
    return worst


def selection_case(F, n, U):
    """(c): the initial priorities and the fill of frame 1 -- [n, 2 n) starts and ends inside a chunk in every geometry (in
    in-order position too) -- from column 1 % U of its valid plane.  -> (before, first, retire_first, value, column, expected)"""
    before = initial_prio(F * n)
    first, retire = frame_ranges(F, n, 1)
    col = valid_plane(n, U, 1)[1 % U:]
    return before, first, retire, fill_value(1), col, ring_fill(before, first, n, fill_value(1), col, U, retire)


def stratified_draws(total, batch, rng):
    """Explicit draws, one per segment of [0, total)."""
    seg = np.float64(total) / batch
    return seg * (np.arange(batch) + rng.uniform(0.0, 1.0, batch))


def selection_margin(capacity, total):
    return 4.0 * capacity * U53 * total


def decided_draws(prio, rot, draws, total):
    """-> the decided mask; at most ONE draw of a call may be undecided (asserted before any device result is looked at)."""
    dec = decided(prio, rot, draws, selection_margin(len(prio), total))
    assert int((~dec).sum()) <= 1, int((~dec).sum())
    return dec


def check_selection(slots, p, prio, rot, draws, dec, what=None):
    """(c): every decided draw lands on the slot the cumulative-sum restatement names; the returned priority is that slot's."""
    want = sample_by_cumsum(prio, None, draws, rot=rot)
    assert np.array_equal(np.asarray(slots)[dec], want[dec]), (what, int((np.asarray(slots)[dec] != want[dec]).sum()))
    assert np.asarray(slots).min() >= 0 and np.asarray(slots).max() < len(prio), what
    assert same_bits(p, np.asarray(prio)[slots]) and (np.asarray(p) > 0).all(), what


def check_set(got_prio, before, slots, abs_err, epsilon, alpha, clip, orc=ORACLE, what=None):
    """(d): written leaves within POW_RTOL of the sequential restatement, exact zeros exact, every leaf no listed slot names
    bitwise unchanged.  -> worst error / bar ratio."""
    before = np.asarray(before, dtype=np.float64)
    want = orc.update(before, slots, abs_err, epsilon, alpha, clip)
    got = np.asarray(got_prio, dtype=np.float64)
    s = np.asarray(slots)
    touched = np.zeros(len(before), dtype=bool)
    touched[s[(s >= 0) & (s < len(before))]] = True
    assert same_bits(got[~touched], before[~touched]), what
    zero = touched & (want == 0.0)
    assert same_bits(got[zero], want[zero]), what
    live = touched & (want != 0.0)
    err, bar = np.abs(got[live] - want[live]), POW_RTOL * np.abs(want[live])
    assert (err <= bar).all(), (what, float((err / bar).max()), np.flatnonzero(live)[~(err <= bar)][:8])
    return float((err / bar).max()) if live.any() else 0.0


def check_weights(w32, tail, fa, p, slots, n_entries, total, beta, n_agents, orc=ORACLE, what=None):
    """(e): f32 weights within one f32 ulp of the rounded f64 oracle (both f64 sides carry a few 1e-16: the f32 values differ
    only across a rounding boundary), maximum exactly 1, zero priorities exactly 0, the scratch tail = the per-workgroup maxima
    of the UNNORMALISED weights (the one place the divisor int(total) shows: it cancels in the normalised ones), the slot split
    exact.  -> worst error / bar ratios."""
    p, w32 = np.asarray(p, dtype=np.float64), np.asarray(w32)
    assert w32.dtype == np.float32 and np.isfinite(w32).all(), what
    ref = orc.weights(p, n_entries, total, beta)
    raw = orc.weights(p, n_entries, total, beta, normalise=False)
    ref32 = ref.astype(np.float32)
    err = np.abs(w32.astype(np.float64) - ref32.astype(np.float64))
    bar = np.spacing(ref32).astype(np.float64)
    live = p > 0
    assert (err[live] <= bar[live]).all(), (what, float((err[live] / bar[live]).max()))
    assert np.array_equal(w32[~live], np.zeros(int((~live).sum()), dtype=np.float32)) and not np.signbit(w32[~live]).any(), what
    if live.any():
        assert w32.max() == np.float32(1.0) and (w32[live] > 0).all(), (what, float(w32.max()))
    n_wg = (len(p) + 255) // 256
    assert len(tail) == n_wg, what
    pad = np.zeros(n_wg * 256)
    pad[:len(p)] = raw
    want_tail = pad.reshape(n_wg, 256).max(axis=1)
    terr, tbar = np.abs(np.asarray(tail) - want_tail), POW_RTOL * want_tail
    assert (terr <= tbar).all(), (what, np.flatnonzero(~(terr <= tbar))[:4])
    if fa is not None:
        fa = np.asarray(fa).astype(np.int64)
        assert np.array_equal(fa[:, 0] * n_agents + fa[:, 1], np.asarray(slots)), what
        assert (fa[:, 1] >= 0).all() and (fa[:, 1] < n_agents).all(), what
    return dict(weights=float((err[live] / bar[live]).max()) if live.any() else 0.0,
                wg_max=float((terr[tbar > 0] / tbar[tbar > 0]).max()) if (tbar > 0).any() else 0.0)


# ------------------------------------------------------------------------------------------------ (f) the K-pass state machine
def pass_inputs(F, n, U, t, slot, batch, seed=5):
    """What pass t of a run over geometry (F, n, U) feeds the tree of UAV slot `slot`: the frame's valid plane (the whole plane
    and where this slot's column starts), the ranges, the Philox (seed, counter) and the f32 errors."""
    first, retire = frame_ranges(F, n, t)
    rng = np.random.default_rng([seed, F, n, U, t, slot])
    err = rng.uniform(0.0, 2.0, batch).astype(np.float32)
    err[rng.uniform(0.0, 1.0, batch) < 0.1] = 0.0
    err[::17] *= -1.0
    return SimpleNamespace(t=t, first=first, retire=retire, count=n, value=(0.0 + EPSILON) ** ALPHA,
                           plane=valid_plane(n, U, t, p_valid=0.875), offset=slot, stride=U,
                           seed=(0x5EED << 32) | (seed + 7 + slot), counter=(0x3 << 32) | t, err=err,
                           n_entries=min(t + 1, F - 1) * n, head=(t + 1) % F)


def oracle_pass(before, rot, inp, batch, beta, n_agents, orc=ORACLE):
    """The oracle standing in for the device: what a correct pass returns (the record check_pass judges)."""
    after_fill = orc.fill(before, inp.first, inp.count, inp.value, inp.plane[inp.offset:], inp.stride, inp.retire)
    total = exact_sums(after_fill, rot)["prefix"][-1]
    draws = px.per_draws(batch, inp.seed, inp.counter, total)
    slots = sample_by_cumsum(after_fill, None, draws, rot=rot)
    p = after_fill[slots]
    raw = orc.weights(p, inp.n_entries, total, beta, normalise=False)
    n_wg = (batch + 255) // 256
    pad = np.zeros(n_wg * 256)
    pad[:batch] = raw
    fa = np.stack([slots // n_agents, slots % n_agents], 1).astype(np.int32)
    return SimpleNamespace(after_fill=after_fill, total=total, slots=slots, p=p,
                           w32=orc.weights(p, inp.n_entries, total, beta).astype(np.float32),
                           tail=pad.reshape(n_wg, 256).max(axis=1), fa=fa,
                           after_set=orc.update(after_fill, slots, inp.err, EPSILON, ALPHA, CLIP))


def check_pass(rec, before, rot, inp, batch, beta, n_agents, F, orc=ORACLE, what=None):
    """One pass re-derived from the priorities the device held BEFORE it: fill/retire bit for bit, the total within the prefix
    bar, the Philox draws and every decided selection, the weights, batch_update; the head frame is never drawn and at most
    F - 1 frames are live."""
    n = inp.count
    want_fill = check_frame(rec.after_fill, before, inp.first, inp.count, inp.value, inp.plane[inp.offset:], inp.stride,
                            inp.retire, orc, what)
    exact_total = exact_sums(want_fill, rot)["prefix"][-1]
    n_chunks = (len(before) + CHUNK - 1) // CHUNK
    assert abs(rec.total - exact_total) <= (prefix_additions(n_chunks) + 11) * U53 * exact_total, what
    assert exact_total >= 1.0, what                              # (int(total) >= 1: the draws are spread, not all 0)
    draws = px.per_draws(batch, inp.seed, inp.counter, rec.total)
    dec = decided_draws(want_fill, rot, draws, exact_total)
    check_selection(rec.slots, rec.p, want_fill, rot, draws, dec, what)
    assert (np.asarray(rec.slots) // n != inp.head).all(), what
    ratios = check_weights(rec.w32, rec.tail, rec.fa, want_fill[rec.slots], rec.slots, inp.n_entries, rec.total, beta, n_agents,
                           orc, what)
    ratios["set_f32"] = check_set(rec.after_set, want_fill, rec.slots, inp.err, EPSILON, ALPHA, CLIP, orc, what)
    assert int((np.asarray(rec.after_set) > 0).sum()) <= (F - 1) * n, what
    assert (np.asarray(rec.after_set).reshape(F, n)[inp.head] == 0.0).all(), what
    return ratios


# ------------------------------------------------------------------------------------------------ (g) perturbed oracles
def fill_shifted(prio, first, count, value, valid, valid_stride, retire_first):
    """the fill range one slot late (the last frame's wraps into range by starting one early)"""
    first = first + 1 if first + count < len(prio) else first - 1
    return ring_fill(prio, first, count, value, valid, valid_stride, retire_first)


def fill_no_retire(prio, first, count, value, valid, valid_stride, retire_first):
    out = ring_fill(prio, first, count, value, valid, valid_stride, retire_first)
    out[retire_first:retire_first + count] = np.asarray(prio)[retire_first:retire_first + count]
    return out


def fill_stride_ignored(prio, first, count, value, valid, valid_stride, retire_first):
    return ring_fill(prio, first, count, value, valid, 1, retire_first)


def weights_unfloored(p, n_entries, total, beta, normalise=True):
    """`total` where the reference has int(total)"""
    p = np.asarray(p, dtype=np.float64)
    w = np.zeros_like(p)
    w[p > 0] = np.power(n_entries * (p[p > 0] / max(float(total), 1.0)), -beta)
    return w / w.max() if normalise and w.max() > 0 else w


def weights_unnormalised(p, n_entries, total, beta, normalise=True):
    return is_weights(p, n_entries, total, beta, normalise=False)


def update_first_wins(prio, slots, abs_err, epsilon, alpha, clip):
    """the FIRST of a run of equal slots wins"""
    return batch_update_seq(prio, np.asarray(slots)[::-1], np.asarray(abs_err)[::-1], epsilon, alpha, clip)


PERTURBED = {
    "fill range shifted by one slot": SimpleNamespace(fill=fill_shifted, weights=is_weights, update=batch_update_seq),
    "retire skipped": SimpleNamespace(fill=fill_no_retire, weights=is_weights, update=batch_update_seq),
    "valid stride ignored": SimpleNamespace(fill=fill_stride_ignored, weights=is_weights, update=batch_update_seq),
    "total instead of floor(total)": SimpleNamespace(fill=ring_fill, weights=weights_unfloored, update=batch_update_seq),
    "normalisation skipped": SimpleNamespace(fill=ring_fill, weights=weights_unnormalised, update=batch_update_seq),
    "first of a run wins": SimpleNamespace(fill=ring_fill, weights=is_weights, update=update_first_wins),
}
FILL_PERTURBATIONS = ("fill range shifted by one slot", "retire skipped", "valid stride ignored")
WEIGHT_PERTURBATIONS = ("total instead of floor(total)", "normalisation skipped")


def set_case(capacity, n, seed=3):
    """(d): a slot list with equal entries ADJACENT (the precondition of uavenv_per_set) -- runs of one slot across the 256-thread
    workgroup edge (indices 254..258) and elsewhere, runs on EMPTY leaves, slots below 0 and at / past the capacity (single and
    in runs) -- and errors above the clip, zero, negative.  -> (prio, slots int64 [n], err float64 [n])"""
    assert n >= 700 and capacity >= 4 * n
    rng = np.random.default_rng([seed, capacity, n])
    prio = initial_prio(capacity, seed)
    empty = np.flatnonzero(prio == 0.0)
    pool = np.setdiff1d(np.arange(capacity), empty[[5, 9]])   # the two empty leaves placed by hand below appear nowhere else
    slots = np.sort(rng.choice(pool, n, replace=False)).astype(np.int64)
    assert (prio[slots] == 0.0).sum() > 20                    # empty leaves among the ordinary entries too
    for lo, hi in ((254, 259), (10, 13), (509, 515), (n - 3, n)):
        slots[lo:hi] = slots[lo]
    prio[slots[254]] = 0.3                                    # the run over the workgroup edge sits on a filled leaf
    slots[40:44] = empty[5]                                   # a run on an empty leaf
    slots[60] = empty[9]
    slots[[100, 101, 300]] = [-1, -1, -(1 << 40)]
    slots[[600, 400, 401]] = [capacity, capacity + 7, capacity + 7]
    err = rng.uniform(0.0, 0.9, n)
    err[rng.uniform(0.0, 1.0, n) < 0.2] += 1.5                # above the clip
    err[::7] = 0.0
    err[3::11] *= -1.0
    err[254:259] = [0.2, 3.0, -0.4, 0.0, 0.55]                # the run over the workgroup edge: distinct, the last one wins
    return prio, slots, err


def weights_case(batch, max_at, seed=9):
    """(e): batch priorities uniform ** 3 with zeros among them and the SMALLEST positive one -- the largest weight for
    beta > 0 -- at index max_at; slots any int64 below 2^31 * 7."""
    rng = np.random.default_rng([seed, batch])
    p = rng.uniform(0.05, 1.0, batch) ** 3
    if batch > 4:
        p[rng.permutation(batch)[:max(1, batch // 9)]] = 0.0
    p[max_at] = 1e-5
    slots = rng.integers(0, 1 << 31, batch).astype(np.int64)
    return p, slots


# ------------------------------------------------------------------------------------------------ (g) resolving power, host only
def rejects(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def host_run(F, n, U, slot, K, batch, beta0=0.4, beta_inc=0.001):
    """K passes with the oracle in the device's place -> [(before, inp, rec, beta)], the records check_pass accepts."""
    rot = rotation(F * n, True)
    prio, beta, trace = np.zeros(F * n), beta0, []
    for t in range(K):
        beta = min(1.0, beta + beta_inc)
        inp = pass_inputs(F, n, U, t, slot, batch)
        rec = oracle_pass(prio, rot, inp, batch, beta, n)
        trace.append((prio, inp, rec, beta))
        prio = rec.after_set
    return rot, trace


def resolving_power_frames():
    """Each perturbed fill must fail (a)'s comparison at EVERY pass of the walk."""
    for name in FILL_PERTURBATIONS:
        for F, n, U in ((7, 600, 1), (9, 37, 4)):
            if U == 1 and name == "valid stride ignored":
                continue
            prio = initial_prio(F * n)
            for t in range(2 * F + 1):
                first, retire = frame_ranges(F, n, t)
                col = valid_plane(n, U, t)[t % U:]
                got = check_frame(ring_fill(prio, first, n, fill_value(t), col, U, retire), prio, first, n, fill_value(t), col, U,
                                  retire)
                assert rejects(check_frame, got, prio, first, n, fill_value(t), col, U, retire, PERTURBED[name]), (name, F, n, U, t)
                prio = got


def resolving_power_weights():
    """Each perturbed weight formula must fail (e)'s assertions, at every beta > 0 (at beta = 0 every weight is 1 whatever the
    formula: nothing to resolve, and nothing that could go wrong)."""
    for batch, max_at in ((257, 256), (1000, 999)):
        p, slots = weights_case(batch, max_at)
        for total in (487.3, 30.6):
            for beta in (0.4, 1.0):
                raw = is_weights(p, 1500, total, beta, normalise=False)
                n_wg = (batch + 255) // 256
                pad = np.zeros(n_wg * 256)
                pad[:batch] = raw
                tail = pad.reshape(n_wg, 256).max(axis=1)
                w32 = is_weights(p, 1500, total, beta).astype(np.float32)
                check_weights(w32, tail, None, p, slots, 1500, total, beta, 7)
                for name in WEIGHT_PERTURBATIONS:
                    assert rejects(check_weights, w32, tail, None, p, slots, 1500, total, beta, 7, PERTURBED[name]), (name, batch, total, beta)


def resolving_power_passes(K=20):
    """Every perturbation must fail (f)'s assertions somewhere in the K passes -> {name: passes that rejected it}."""
    out = {}
    for F, n, U, slot, batch in ((7, 600, 1, 0, 256), (9, 37, 4, 2, 64)):
        rot, trace = host_run(F, n, U, slot, K, batch)
        for before, inp, rec, beta in trace:
            check_pass(rec, before, rot, inp, batch, beta, n, F)
        for name, orc in PERTURBED.items():
            if U == 1 and name == "valid stride ignored":
                continue
            hits = sum(rejects(check_pass, rec, before, rot, inp, batch, beta, n, F, orc) for before, inp, rec, beta in trace)
            assert hits >= 1, (name, F, n, U)
            out[(name, F, n, U)] = hits
    return out
