"""The prioritised-replay kernels AROUND the sampler (csrc/per.hip), each against oracle/per_oracle.py's plain-numpy restatement
of the contract in include/uavenv.h -- numbers the device had no part in.  k_per_sample itself is pinned by
tests/test_random_streams_gpu.py; here are the kernels that keep the priorities it reads, and the importance weights:

  (a) uavenv_per_fill_frame / _fill_frame_strided / _rebuild_frame (k_per_fill2, k_per_chunk_sum's fused fill and retire): the
      three entry points csrc/loop.hip enqueues per pass, walked twice round the ring -- priorities equal ring_fill bit for bit,
      the three forms leave prio, chunk_sum, chunk_prefix and group_sum bit-identical, sentinels behind all four intact; frames
      that begin and end inside a 1 024-leaf chunk, rot = 0 and the flat tree's rotation, a valid plane read at a stride.
  (b) group_sum, chunk_sum, chunk_prefix against exact_sums (math.fsum / rationals) of the device's OWN priorities.  The bars
      are the addition chains of the code: a group sum is 16 leaves added in order from 0.0 -- 15 roundings; a chunk sum is 4
      leaves per thread (3 roundings) and an 8-level LDS tree -- 11; a prefix entry passes through at most per = ceil(n_chunks /
      256) additions for a thread's own sum, 255 for the running sum over the threads and per more along the thread's chunks.
      Each rounding is at most 2^-53 of a partial sum of non-negative operands, hence of their whole sum:
          group 15 * 2^-53 * group,  chunk 11 * 2^-53 * chunk,  prefix[b] (2 per + 255) * 2^-53 * total + 11 * 2^-53 * prefix[b].
      chunk_prefix[0] == 0 exactly; chunk_prefix[n_chunks] (the total, written by one thread only) for 1, 2, 255, 256, 257 and
      4 098 chunks.
  (c) uavenv_per_sample after a fused rebuild whose frame starts and ends inside chunks: with and without group sums bit for bit,
      and sample_by_cumsum of the ORACLE's priorities on every decided draw (further than 4 capacity 2^-53 total from a leaf
      edge; at most one draw per call may be undecided, asserted before the device is looked at -- on the CPU none is,
      tests/test_per_ref.py).
  (d) uavenv_per_set / _set_f32 / _set_f32_gated against batch_update_seq: runs of one slot over the 256-thread edge, slots
      outside the tree, empty leaves with and without a clip; written leaves within 4e-16 (OCML pow against the host's), zeros
      exact, unlisted leaves bitwise unchanged; a closed gate changes no byte.
  (e) uavenv_per_weights against is_weights for 1 .. 65 793 samples (258 workgroups: the second round of k_per_weights_norm's
      loop over the workgroup maxima): f32 weights within one f32 ulp of the rounded oracle, maximum exactly 1, zero priorities
      exactly 0, the scratch tail = the per-workgroup maxima of the unnormalised weights (4e-16), the slot split exact;
      n_entries <= 0 is refused.
  (f) 20 passes of fill/retire, Philox sampling, weights, batch_update and a beta step, every pass re-derived from the
      priorities the device held before it.
  (g) on the host only: the assertions of (a), (e) and (f) reject an oracle with a shifted fill range, a skipped retire, an
      ignored valid stride, total for int(total), a skipped normalisation, first-of-run for last-of-run.

Worst error / bar per kernel, MEASURED ON THE DEVICE (an MI355X; run this module with -s and it prints them) -- a record of
how much room the bars leave, none of them went into a bar:
  (b) k_per_chunk_sum: group_sum 0.37, chunk_sum 0.22; k_per_prefix: chunk_prefix 0.036
  (d) k_per_set 0.55; k_per_set_f32 0.55 (0.56 in the passes of (f))
  (e) k_per_weights_pow: workgroup maxima 0.56; k_per_weights_norm: f32 weights 0.0 of one ulp (every weight equal to the
      rounded oracle; no case straddled a rounding boundary)
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import per_frame_fixtures as fx
from dqn_based_uav_3d_path_planer_amd import _lib
from oracle.per_oracle import exact_sums

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 8
WORST = {}


def _note(**ratios):
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("worst error / bar so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t, offset=0):
    return None if t is None else t.data_ptr() + offset


class Tree:
    """One UavPer whose four arrays lie in ONE device allocation, each followed by PAD sentinel doubles: a single copy brings the
    whole state, sentinels included, to the host.  The sums start as NaN: an entry a rebuild does not write shows."""

    def __init__(self, capacity, rot, prio=None, group=True):
        self.lib = _lib.load()
        self.cap = int(capacity)
        self.nc = self.lib.uavenv_per_num_chunks(self.cap)
        assert self.nc == (self.cap + 1023) // 1024
        self.sizes = [self.cap, self.nc, self.nc + 1, self.nc * 64]
        self.off = [0]
        for s in self.sizes:
            self.off.append(self.off[-1] + s + PAD)
        host = np.full(self.off[-1], np.nan)
        host[:self.cap] = 0.0 if prio is None else prio
        for o, s in zip(self.off, self.sizes):
            host[o + s:o + s + PAD] = fx.SENTINEL
        self.buf = _dev(host)
        base = self.buf.data_ptr()
        at = [base + 8 * o for o in self.off]
        self.c = _lib.UavPer(at[0], at[1], at[2], self.cap, int(rot), at[3] if group else None)
        self.plain = _lib.UavPer(at[0], at[1], at[2], self.cap, int(rot), None)          # group_sum == NULL
        self.ref = C.byref(self.c)

    def read(self):
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        for o, s in zip(self.off, self.sizes):
            assert fx.same_bits(h[o + s:o + s + PAD], np.full(PAD, fx.SENTINEL)), "a sentinel behind array %d was written" % self.off.index(o)
        part = [h[o:o + s] for o, s in zip(self.off, self.sizes)]
        return SimpleNamespace(prio=part[0], chunk_sum=part[1], chunk_prefix=part[2], group_sum=part[3], all=h)

    def rebuild(self):
        assert self.lib.uavenv_per_rebuild(self.ref, _stream()) == _lib.OK

    def fill_frame(self, first, count, value, valid, retire):
        return self.lib.uavenv_per_fill_frame(self.ref, first, count, value, _ptr(valid), retire, _stream())

    def rebuild_frame(self, first, count, value, valid, retire):
        return self.lib.uavenv_per_rebuild_frame(self.ref, first, count, value, _ptr(valid), retire, _stream())

    def fill_frame_strided(self, first, count, value, valid, offset, stride, retire):
        return self.lib.uavenv_per_fill_frame_strided(self.ref, first, count, value, _ptr(valid, offset), stride, retire, _stream())

    def sample(self, batch, draws=None, seed=0, counter=0, grouped=True):
        slots = torch.full((batch + PAD,), -7, dtype=torch.int64, device=DEV)
        p = torch.full((batch + PAD,), fx.SENTINEL, dtype=torch.float64, device=DEV)
        d = None if draws is None else _dev(np.asarray(draws, dtype=np.float64))
        rc = self.lib.uavenv_per_sample(C.byref(self.c if grouped else self.plain), batch, _ptr(d), seed, counter, slots.data_ptr(),
                                        p.data_ptr(), _stream())
        assert rc == _lib.OK
        torch.cuda.synchronize()
        assert bool((slots[batch:] == -7).all()) and bool((p[batch:] == fx.SENTINEL).all())
        return slots[:batch].clone(), p[:batch].clone()


def _weights(tree, slots_dev, p_host, n_entries, beta, n_agents, with_fa=True):
    """uavenv_per_weights on batch priorities -> (rc, w32, tail, fa, w64) as numpy, sentinels behind every output checked."""
    batch = len(p_host)
    n_wg = (batch + 255) // 256
    pbuf = _dev(np.concatenate([p_host, np.full(n_wg, np.nan), np.full(PAD, fx.SENTINEL)]))
    w32 = torch.full((batch + PAD,), -3.0, dtype=torch.float32, device=DEV)
    fa = torch.full((batch * 2 + PAD,), -9, dtype=torch.int32, device=DEV)
    rc = tree.lib.uavenv_per_weights(tree.ref, slots_dev.data_ptr(), pbuf.data_ptr(), batch, n_entries, beta, n_agents, w32.data_ptr(),
                                     fa.data_ptr() if with_fa else None, _stream())
    torch.cuda.synchronize()
    ph, wh, fh = pbuf.cpu().numpy(), w32.cpu().numpy(), fa.cpu().numpy()
    assert fx.same_bits(ph[batch + n_wg:], np.full(PAD, fx.SENTINEL)), "written behind the scratch tail"
    assert (wh[batch:] == -3.0).all() and (fh[batch * 2:] == -9).all()
    if not with_fa:
        assert (fh == -9).all()
    return rc, wh[:batch], ph[batch:batch + n_wg], fh[:batch * 2].reshape(batch, 2), ph[:batch]


def _rot(tree_lib, cap, rotated):
    rot = tree_lib.uavenv_per_rotation(cap) if rotated else 0
    assert rot == fx.rotation(cap, rotated)
    return rot


# ------------------------------------------------------------------------------------------------ (a) frame bookkeeping
@pytest.mark.parametrize("rotated", [False, True], ids=["rot0", "tree_rot"])
@pytest.mark.parametrize("geom", fx.GEOMS, ids=lambda g: "F%d_n%d_U%d" % g)
def test_the_three_frame_forms_equal_ring_fill_and_each_other(geom, rotated):
    F, n, U = geom
    cap = F * n
    lib = _lib.load()
    rot = _rot(lib, cap, rotated)
    prio = fx.initial_prio(cap)
    trees = [Tree(cap, rot, prio) for _ in range(3)]
    last_leaf = False
    for t in range(2 * F + 1):                                   # twice round the ring: every frame is filled AND retired
        first, retire = fx.frame_ranges(F, n, t)
        last_leaf |= first + n == cap
        value, j = fx.fill_value(t), t % U
        if t % 5 == 4:                                           # valid_dev NULL: every row counts
            plane = col = d_plane = d_col = None
        else:
            plane = fx.valid_plane(n, U, t)
            col = plane[j::U].copy()                             # the forms without a stride take the column packed
            assert len(col) == n
            d_plane, d_col = _dev(plane), _dev(col)
        assert trees[0].fill_frame(first, n, value, d_col, retire) == _lib.OK
        trees[0].rebuild()
        assert trees[1].rebuild_frame(first, n, value, d_col, retire) == _lib.OK
        assert trees[2].fill_frame_strided(first, n, value, d_plane, j, U, retire) == _lib.OK
        trees[2].rebuild()
        got = [tr.read() for tr in trees]
        what = (geom, rot, t)
        prio = fx.check_frame(got[0].prio, prio, first, n, value, None if plane is None else plane[j:], U, retire, what=what)
        for g in got[1:]:
            assert fx.same_bits(g.all, got[0].all), what         # prio, chunk_sum, chunk_prefix, group_sum and the sentinels
        assert not np.isnan(got[0].all).any(), what              # every sum was written
    assert last_leaf


def test_frame_forms_with_nothing_to_do_and_refused_arguments():
    F, n, U = 7, 600, 2
    cap = F * n
    prio = fx.initial_prio(cap)
    tree = Tree(cap, fx.rotation(cap, True), prio)
    tree.rebuild()
    before = tree.read().all
    plane = _dev(fx.valid_plane(n, U, 0))
    assert tree.fill_frame(600, 0, 0.5, plane, 1200) == _lib.OK                      # count = 0
    assert tree.fill_frame_strided(600, 0, 0.5, plane, 0, U, 1200) == _lib.OK
    assert tree.rebuild_frame(600, 0, 0.5, plane, 1200) == _lib.OK                   # (a plain rebuild)
    assert fx.same_bits(tree.read().all, before)
    bad = [(cap - n + 1, n, 0), (0, n, cap - n + 1), (-1, n, 1200), (600, n, -1), (600, -1, 1200), (cap, 1, 0), (0, cap + 1, 0)]
    for first, count, retire in bad:
        assert tree.fill_frame(first, count, 0.5, plane, retire) == _lib.EINVAL, (first, count, retire)
        assert tree.rebuild_frame(first, count, 0.5, plane, retire) == _lib.EINVAL, (first, count, retire)
        assert tree.fill_frame_strided(first, count, 0.5, plane, 0, U, retire) == _lib.EINVAL, (first, count, retire)
    for stride in (0, -1, -(1 << 40)):
        assert tree.fill_frame_strided(600, n, 0.5, plane, 0, stride, 1200) == _lib.EINVAL
    assert fx.same_bits(tree.read().all, before)                                     # a refused call writes nothing
    assert tree.fill_frame_strided(cap - n, n, 0.5, plane, 1, U, 0) == _lib.OK       # the range that ends on the last leaf
    want = fx.check_frame(tree.read().prio, prio, cap - n, n, 0.5, fx.valid_plane(n, U, 0)[1:], U, 0)
    assert want[-1] in (0.0, 0.5) and (want[cap - n:] == 0.5).sum() > n // 2


# ------------------------------------------------------------------------------------------------ (b) sums
@pytest.mark.parametrize("rotated", [False, True], ids=["rot0", "tree_rot"])
@pytest.mark.parametrize("geom", fx.GEOMS, ids=lambda g: "F%d_n%d_U%d" % g)
def test_sums_after_fused_rebuilds_against_exact_sums(geom, rotated):
    F, n, U = geom
    cap = F * n
    rot = _rot(_lib.load(), cap, rotated)
    tree = Tree(cap, rot, fx.initial_prio(cap))
    worst = {}
    for t in range(2 * F + 1):
        first, retire = fx.frame_ranges(F, n, t)
        col = _dev(fx.valid_plane(n, U, t)[t % U::U].copy())
        assert tree.rebuild_frame(first, n, fx.fill_value(t), col, retire) == _lib.OK
        if F <= 9 or t % 8 == 0 or t == 2 * F:
            g = tree.read()
            r = fx.check_sums(g.prio, rot, g.chunk_sum, g.chunk_prefix, g.group_sum, what=(geom, rot, t))
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    _note(**worst)


@pytest.mark.parametrize("cap", [1000, 1025, 255 * 1024 - 7, 256 * 1024, 256 * 1024 + 1, 4097 * 1024 + 5],
                         ids=["1_chunk", "2_chunks", "255_chunks", "256_chunks", "257_chunks", "4098_chunks"])
def test_prefix_and_total_for_every_split_of_the_chunks_over_the_prefix_workgroup(cap):
    """uavenv_per_rebuild on a plain array: 255, 256 chunks -> one chunk per thread of k_per_prefix (one thread idle / none),
    257 -> two per thread and half the threads idle, 4 098 -> 17 per thread, the last thread with a ragged share."""
    lib = _lib.load()
    for rotated in ((False, True) if cap < (1 << 20) else (True,)):
        rot = _rot(lib, cap, rotated)
        prio = fx.initial_prio(cap)
        tree = Tree(cap, rot, prio)
        tree.rebuild()
        g = tree.read()                                          # (asserts the sentinel behind chunk_prefix[n_chunks])
        assert fx.same_bits(g.prio, prio) and not np.isnan(g.all).any()
        r = fx.check_sums(g.prio, rot, g.chunk_sum, g.chunk_prefix, g.group_sum, what=(cap, rot))
        assert (np.diff(g.chunk_prefix) >= 0).all() and g.chunk_prefix[-1] > 0.1 * cap
        _note(**r)


# ------------------------------------------------------------------------------------------------ (c) selection after a fused rebuild
@pytest.mark.parametrize("rotated", [False, True], ids=["rot0", "tree_rot"])
@pytest.mark.parametrize("geom", fx.GEOMS, ids=lambda g: "F%d_n%d_U%d" % g)
def test_selection_after_a_fused_rebuild(geom, rotated):
    F, n, U = geom
    cap = F * n
    rot = _rot(_lib.load(), cap, rotated)
    before, first, retire, value, col, want = fx.selection_case(F, n, U)
    tree = Tree(cap, rot, before)
    assert tree.rebuild_frame(first, n, value, _dev(col[::U].copy()), retire) == _lib.OK
    assert fx.same_bits(tree.read().prio, want)
    total = exact_sums(want, rot)["prefix"][-1]
    rng = np.random.default_rng([41, cap, rot])
    for batch in (1, 255, 257, 1000):
        draws = fx.stratified_draws(total, batch, rng)
        dec = fx.decided_draws(want, rot, draws, total)          # before the device is looked at
        s1, p1 = tree.sample(batch, draws, grouped=True)
        s2, p2 = tree.sample(batch, draws, grouped=False)
        assert torch.equal(s1, s2) and fx.same_bits(p1.cpu().numpy(), p2.cpu().numpy()), (geom, rot, batch)
        fx.check_selection(s1.cpu().numpy(), p1.cpu().numpy(), want, rot, draws, dec, what=(geom, rot, batch))


# ------------------------------------------------------------------------------------------------ (d) batch_update
@pytest.mark.parametrize("clip", [1.0, 0.0], ids=["clip1", "push"])
def test_set_kernels_against_the_sequential_loop(clip):
    cap, n = 5000, 700
    prio, slots, err = fx.set_case(cap, n)
    d_slots = _dev(slots)
    err32 = err.astype(np.float32)
    d_err, d_err32 = _dev(err), _dev(err32)
    args = (fx.EPSILON, fx.ALPHA, clip)
    lib = _lib.load()

    t64 = Tree(cap, 0, prio)
    assert lib.uavenv_per_set(t64.ref, d_slots.data_ptr(), d_err.data_ptr(), n, *args, _stream()) == _lib.OK
    r64 = fx.check_set(t64.read().prio, prio, slots, err, *args, what="f64")

    t32 = Tree(cap, 0, prio)
    assert lib.uavenv_per_set_f32(t32.ref, d_slots.data_ptr(), d_err32.data_ptr(), n, *args, _stream()) == _lib.OK
    got32 = t32.read()
    r32 = fx.check_set(got32.prio, prio, slots, err32.astype(np.float64), *args, what="f32")
    edge = slots[258]                                            # the run over the workgroup edge took its LAST error
    assert abs(got32.prio[edge] - (float(err32[258]) + fx.EPSILON) ** fx.ALPHA) <= 1e-15 and (prio[edge] > 0 or clip == 0.0)

    word = torch.tensor([5, 6], dtype=torch.int32, device=DEV)                      # the gate word holds 5
    shut = Tree(cap, 0, prio)
    before = shut.read().all
    assert lib.uavenv_per_set_f32_gated(shut.ref, d_slots.data_ptr(), d_err32.data_ptr(), n, *args, word.data_ptr(), 6, _stream()) == _lib.OK
    assert fx.same_bits(shut.read().all, before)                                     # closed: not a byte
    for gate in (word.data_ptr(), None):
        tg = Tree(cap, 0, prio)
        assert lib.uavenv_per_set_f32_gated(tg.ref, d_slots.data_ptr(), d_err32.data_ptr(), n, *args, gate, 5, _stream()) == _lib.OK
        assert fx.same_bits(tg.read().all, got32.all)                                # open / no word: the ungated call
    assert lib.uavenv_per_set_f32(shut.ref, d_slots.data_ptr(), d_err32.data_ptr(), 0, *args, _stream()) == _lib.OK    # n = 0
    assert lib.uavenv_per_set(shut.ref, d_slots.data_ptr(), d_err.data_ptr(), 0, *args, _stream()) == _lib.OK
    assert fx.same_bits(shut.read().all, before)
    _note(per_set=r64, per_set_f32=r32)


# ------------------------------------------------------------------------------------------------ (e) importance weights
def _weight_trees():
    big = Tree(2000, fx.rotation(2000, True), fx.initial_prio(2000))                # total ~ 370
    small = Tree(300, 0, fx.initial_prio(300) * 1e-3)                               # total < 1: int(total) = 0 counts as 1
    out = []
    for tr in (big, small):
        tr.rebuild()
        out.append((tr, float(tr.read().chunk_prefix[-1])))
    assert out[0][1] > 100.0 and 0.0 < out[1][1] < 1.0
    return out


@pytest.mark.parametrize("batch,max_at", [(1, 0), (255, 254), (256, 255), (257, 256), (1000, 999), (65793, 65792), (65793, 65536 + 17)],
                         ids=["1", "255", "256", "257", "1000", "65793_last_wg", "65793_wg256"])
def test_weights_against_is_weights(batch, max_at):
    p, slots = fx.weights_case(batch, max_at)
    assert p[max_at] == p[p > 0].min() and ((p == 0).any() or batch <= 4) and max_at // 256 in ((batch - 1) // 256, 256)
    d_slots = _dev(slots)
    worst = {}
    for k, (tree, total) in enumerate(_weight_trees()):
        for i, beta in enumerate((0.0, 0.4, 1.0)):
            n_agents = (1, 7, 1000)[(i + k) % 3]
            rc, w32, tail, fa, _ = _weights(tree, d_slots, p, 1500, beta, n_agents)
            assert rc == _lib.OK
            r = fx.check_weights(w32, tail, fa, p, slots, 1500, total, beta, n_agents, what=(batch, max_at, total, beta))
            if beta > 0:
                assert w32[max_at] == np.float32(1.0) and (w32 == 1.0).sum() == 1
            worst = {kk: max(v, worst.get(kk, 0.0)) for kk, v in r.items()}
    rc, w32, tail, fa, _ = _weights(tree, d_slots, p, 1500, 0.4, 7, with_fa=False)                   # frame_agent_out_dev NULL
    assert rc == _lib.OK
    fx.check_weights(w32, tail, None, p, slots, 1500, total, 0.4, 7)
    _note(weights_f32_ulp=worst["weights"], weights_wg_max=worst["wg_max"])


def test_weights_of_an_all_zero_batch_and_refused_entry_counts():
    (tree, total), _ = _weight_trees()
    for batch in (5, 300):
        p, slots = np.zeros(batch), np.arange(batch, dtype=np.int64)
        rc, w32, tail, fa, _ = _weights(tree, _dev(slots), p, 1500, 0.4, 7)
        assert rc == _lib.OK and np.array_equal(w32, np.zeros(batch, dtype=np.float32)) and np.array_equal(tail, np.zeros(len(tail)))
        fx.check_weights(w32, tail, fa, p, slots, 1500, total, 0.4, 7)
    p, slots = fx.weights_case(300, 299)
    for n_entries in (0, -1):                                    # the header: refused, nothing is written
        rc, w32, tail, fa, w64 = _weights(tree, _dev(slots), p, n_entries, 0.4, 7)
        assert rc == _lib.EINVAL
        assert (w32 == -3.0).all() and (fa == -9).all() and np.isnan(tail).all() and fx.same_bits(w64, p)


# ------------------------------------------------------------------------------------------------ (f) K passes
@pytest.mark.parametrize("F,n,U,batch", [(7, 600, 1, 256), (9, 37, 4, 64)], ids=["shared_tree", "per_slot_trees"])
def test_k_pass_state_machine(F, n, U, batch):
    K, cap = 20, F * n
    lib = _lib.load()
    rot = _rot(lib, cap, True)
    trees = [Tree(cap, rot) for _ in range(U)]                   # one tree per UAV slot, over its column of the valid plane
    prios = [np.zeros(cap) for _ in range(U)]
    beta, worst = 0.4, {}
    for t in range(K):
        beta = min(1.0, beta + 0.001)
        for j, tree in enumerate(trees):
            inp = fx.pass_inputs(F, n, U, t, j, batch)
            d_plane = _dev(inp.plane)
            if U == 1:
                assert tree.rebuild_frame(inp.first, n, inp.value, d_plane, inp.retire) == _lib.OK
            else:
                assert tree.fill_frame_strided(inp.first, n, inp.value, d_plane, j, U, inp.retire) == _lib.OK
                tree.rebuild()
            after_fill = tree.read()
            slots, p = tree.sample(batch, None, seed=inp.seed, counter=inp.counter)
            _, w32, tail, fa, _ = _weights(tree, slots, p.cpu().numpy(), inp.n_entries, beta, n)
            d_err = _dev(inp.err)
            assert lib.uavenv_per_set_f32(tree.ref, slots.data_ptr(), d_err.data_ptr(), batch, fx.EPSILON, fx.ALPHA, fx.CLIP,
                                          _stream()) == _lib.OK
            rec = SimpleNamespace(after_fill=after_fill.prio, total=float(after_fill.chunk_prefix[-1]), slots=slots.cpu().numpy(),
                                  p=p.cpu().numpy(), w32=w32, tail=tail, fa=fa, after_set=tree.read().prio)
            r = fx.check_pass(rec, prios[j], rot, inp, batch, beta, n, F, what=(F, n, U, t, j))
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
            prios[j] = rec.after_set
    assert len({pr.tobytes() for pr in prios}) == U              # the slots' trees went their own ways
    _note(**{"pass_" + k: v for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------ (g) resolving power
def test_the_assertions_reject_perturbed_oracles_on_the_host():
    fx.resolving_power_frames()
    fx.resolving_power_weights()
    hits = fx.resolving_power_passes()
    assert len(hits) == 11 and all(h >= 1 for h in hits.values()), hits
    print({k[0]: v for k, v in hits.items()})
