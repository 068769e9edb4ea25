"""Prioritised replay in the per-slot DQN loop on the device: the slot-batched kernels of csrc/per.hip (uavenv_per_*_slots),
the weighted gradient of all slots (k_dqn_grad_slots_w of csrc/learner.hip), uavenv_dqn_slots_loop_set_per of csrc/loop.hip
(loop.DQNSlotsHotLoop(pers=...)) and the plugin path <fused_slots>1</fused_slots> with IsPriority_Replay = 1.

 (a) each slot kernel against its per-tree entry point, bit for bit (priorities, chunk sums, prefixes, group sums, chosen slots
     and their priorities, f32 weights, the unnormalised weights and the scratch tails, written leaves; sentinels behind every
     array), and against the host model oracle/per_oracle.py through tests/per_frame_fixtures.py at that file's own bars.
     U in {1, 2, 4, 8}; capacity 9 x 200 (two chunks, the second partial; frames inside a chunk, across the chunk edge, and the
     last frame with the retire wrapping to 0), once 5 x 13 200 (65 chunks: the sampler's segment stride is 2); batches 64 and
     320 (two weights workgroups, the second partial).  The slots' trees differ in seed and scale (so the weight maximum and
     int(total) are per slot), slot 1 is all zero, and every slot reads its own column of the valid plane.
 (b) uavenv_dqn_grad_slots_w against uavenv_dqn_grad_img with weights and |TD| out, slot by slot, bit for bit (partial rows and
     |TD|), and each slot's raw bucket and |TD| against oracle.dqn_grad_ref.dqn_grad_f64(is_weights=...) at the bound of
     tests/test_dqn_grad_kernels_gpu.py (check_a, F32).
 (c) the loop against the composition of the per-tree entry points issued from Python, bit for bit: ring planes, every learner's
     parameters, moments, target, loss and epoch, every tree's priorities and sums, beta, cursor and counter; the gate; the
     refusals of uavenv_dqn_slots_loop_set_per; a loop without trees equals the uniform composition.
 (d) the plugin: <fused_slots>1</fused_slots>, num_UAV = 2, IsPriority_Replay = 1 stays on the fused path for two episodes."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import per_frame_fixtures as fx
import test_dqn_grad_kernels_gpu as G
from oracle import philox as px
from oracle.dqn_grad_ref import dqn_grad_f64
from test_dqn_slots_loop_gpu import HEADS, M64, PARAM, build, compose, good_cfg, net_array, stream
from test_dqn_update_slots_gpu import GUARD, SENTINEL, bits, hand_pairs, make_nets, new_parts, ptrs
from test_per_frame_kernels_gpu import DEV, PAD, Tree, _dev, _weights

pytestmark = pytest.mark.gpu


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


@pytest.fixture(scope="module", autouse=True)
def _release_pool():
    """The row pool of tests/test_dqn_grad_kernels_gpu.py (the hand rings of (b) draw their rows from it) lives for this module."""
    yield
    if G._POOL is not None:
        G._POOL.env.close()
        G._POOL = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ (a) the slot kernels
ZERO_SLOT = 1                     # with two slots or more, this one's tree is all zero and so is its column of every valid plane


def tab(trees):
    return (C.POINTER(_lib().UavPer) * len(trees))(*[C.pointer(t.c) for t in trees])


def slot_prios(U, cap):
    """One tree per slot: another seed and another scale each (the totals differ by integers, the weight maxima too)."""
    out = [fx.initial_prio(cap, seed=11 + j) * (0.5 + 0.75 * j) for j in range(U)]
    if U > 1:
        out[ZERO_SLOT] = np.zeros(cap)
    return out


def slot_plane(n, U, t):
    """Frame t's valid plane, n rows of U flags: every column its own pattern; the zero slot's column all 0."""
    plane = fx.valid_plane(n, U, t).reshape(n, U).copy()
    for j in range(U):
        plane[(j + t) % (j + 3)::j + 3, j] = 0
    if U > 1:
        plane[:, ZERO_SLOT] = 0
    return np.ascontiguousarray(plane.reshape(-1))


class Out:
    """The slot-major outputs of a sample / weights pair, sentinels behind each."""

    def __init__(self, U, B):
        self.U, self.B, self.nwg = U, B, (B + 255) // 256
        self.slots = torch.full((U * B + PAD,), -7, dtype=torch.int64, device=DEV)
        row = np.concatenate([np.full(B, np.nan), np.full(self.nwg, np.nan)])
        self.prio = _dev(np.concatenate([np.tile(row, U), np.full(PAD, fx.SENTINEL)]))
        self.w = torch.full((U * B + PAD,), -3.0, dtype=torch.float32, device=DEV)
        self.pairs = torch.full((U * B * 2 + PAD,), -9, dtype=torch.int32, device=DEV)

    def read(self):
        torch.cuda.synchronize()
        U, B, nwg = self.U, self.B, self.nwg
        s, p, w, fa = self.slots.cpu().numpy(), self.prio.cpu().numpy(), self.w.cpu().numpy(), self.pairs.cpu().numpy()
        assert (s[U * B:] == -7).all() and fx.same_bits(p[U * (B + nwg):], np.full(PAD, fx.SENTINEL))
        assert (w[U * B:] == -3.0).all() and (fa[U * B * 2:] == -9).all()
        p = p[:U * (B + nwg)].reshape(U, B + nwg)
        return s[:U * B].reshape(U, B), p[:, :B], p[:, B:], w[:U * B].reshape(U, B), fa[:U * B * 2].reshape(U, B, 2)


def same_f32(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def one_pass(lib, A, R, F, n, t, B, fused, seed, counter, beta, rng):
    """Pass t on the trees A (the _slots calls) and R (the per-tree calls): fill / retire, rebuild, sample, weights, batch_update --
    each step compared bit for bit, and tree by tree with the host model."""
    L, U, cap = _lib(), len(A), F * n
    first, retire = fx.frame_ranges(F, n, t)
    value = fx.fill_value(t)
    plane = slot_plane(n, U, t)
    d_plane = _dev(plane)
    before = [tr.read().prio.copy() for tr in A]
    what = (U, F, n, t, B)
    # -- fill / retire and rebuild
    if fused:
        assert lib.uavenv_per_rebuild_slots(tab(A), U, first, n, value, d_plane.data_ptr(), retire, stream()) == L.OK
        for j, tr in enumerate(R):
            assert tr.rebuild_frame(first, n, value, _dev(plane[j::U].copy()), retire) == L.OK
    else:
        assert lib.uavenv_per_fill_frame_slots(tab(A), U, first, n, value, d_plane.data_ptr(), retire, stream()) == L.OK
        assert lib.uavenv_per_rebuild_slots(tab(A), U, 0, 0, 0.0, None, 0, stream()) == L.OK
        for j, tr in enumerate(R):
            assert tr.fill_frame_strided(first, n, value, d_plane, j, U, retire) == L.OK
            tr.rebuild()
    got = [tr.read() for tr in A]
    totals = []
    for j in range(U):
        assert fx.same_bits(got[j].all, R[j].read().all), (what, j)      # prio, chunk_sum, chunk_prefix, group_sum, sentinels
        assert not np.isnan(got[j].all).any(), (what, j)
        fx.check_frame(got[j].prio, before[j], first, n, value, plane[j:], U, retire, what=(what, j))
        fx.check_sums(got[j].prio, 0, got[j].chunk_sum, got[j].chunk_prefix, got[j].group_sum, what=(what, j))
        totals.append(float(got[j].chunk_prefix[-1]))
    if U > 1:
        assert totals[ZERO_SLOT] == 0.0
        if t == 1:                 # the first pass of a walk, on the trees as slot_prios scaled them: int(total) is per slot
            assert len({int(x) for x in totals}) == U
    # -- sample
    out = Out(U, B)
    assert lib.uavenv_per_sample_slots(tab(A), U, B, seed, counter, out.slots.data_ptr(), out.prio.data_ptr(), stream()) == L.OK
    s_all, p_all, tail0, _, _ = out.read()
    assert np.isnan(tail0).all()                                         # the sampler leaves the scratch tails alone
    ref_s, ref_p = [], []
    for j, tr in enumerate(R):
        s, p = tr.sample(B, None, (seed + j) & M64, counter)
        ref_s.append(s)
        ref_p.append(p.cpu().numpy())
        assert np.array_equal(s_all[j], s.cpu().numpy()) and fx.same_bits(p_all[j], ref_p[j]), (what, j)
        if U > 1 and j == ZERO_SLOT:
            assert (p_all[j] == 0.0).all()
            continue
        draws = px.per_draws(B, (seed + j) & M64, counter, totals[j])
        dec = fx.decided_draws(got[j].prio, 0, draws, totals[j])
        fx.check_selection(s_all[j], p_all[j], got[j].prio, 0, draws, dec, what=(what, j))
        assert (s_all[j] // n != retire // n).all(), (what, j)           # the head frame is never drawn
    # -- weights and the (frame, agent) pairs
    n_entries = min(t + 1, F - 1) * n
    assert lib.uavenv_per_weights_slots(tab(A), U, out.slots.data_ptr(), out.prio.data_ptr(), B, n_entries, beta, n, out.w.data_ptr(),
                                        out.pairs.data_ptr(), stream()) == L.OK
    _, w64, tails, w32, pairs = out.read()
    w_max = []
    for j, tr in enumerate(R):
        rc, rw32, rtail, rfa, rw64 = _weights(tr, ref_s[j], ref_p[j], n_entries, beta, n)
        assert rc == L.OK
        assert same_f32(w32[j], rw32) and fx.same_bits(tails[j], rtail) and fx.same_bits(w64[j], rw64), (what, j)
        s = s_all[j]
        assert np.array_equal(pairs[j, :, 0], s // n) and np.array_equal(pairs[j, :, 1], (s % n) * U + j), (what, j)
        assert np.array_equal(rfa[:, 0], s // n) and np.array_equal(rfa[:, 1], s % n)
        if U > 1 and j == ZERO_SLOT:
            assert (w32[j] == 0.0).all() and (tails[j] == 0.0).all()
            continue
        fx.check_weights(w32[j], tails[j], rfa, p_all[j], s, n_entries, totals[j], beta, n, what=(what, j))
        w_max.append(float(tails[j].max()))
    assert len(set(w_max)) == len(w_max)                                 # the maximum each slot divides by is its own
    # -- batch_update
    err = rng.uniform(0.0, 2.0, (U, B)).astype(np.float32)
    err[:, ::17] *= -1.0
    err[:, 5::11] = 0.0
    d_err = _dev(err)
    assert lib.uavenv_per_set_f32_slots_gated(tab(A), U, out.slots.data_ptr(), d_err.data_ptr(), B, fx.EPSILON, fx.ALPHA, fx.CLIP,
                                              None, 0, stream()) == L.OK
    for j, tr in enumerate(R):
        assert lib.uavenv_per_set_f32_gated(tr.ref, ref_s[j].data_ptr(), d_err.data_ptr() + 4 * j * B, B, fx.EPSILON, fx.ALPHA, fx.CLIP,
                                            None, 0, stream()) == L.OK
    after = [tr.read() for tr in A]
    for j in range(U):
        assert fx.same_bits(after[j].all, R[j].read().all), (what, j)
        fx.check_set(after[j].prio, got[j].prio, s_all[j], err[j], fx.EPSILON, fx.ALPHA, fx.CLIP, what=(what, j))
        if U > 1 and j == ZERO_SLOT:
            assert (after[j].prio == 0.0).all()                          # an empty leaf stays empty
        else:
            assert not fx.same_bits(after[j].prio, got[j].prio)


@pytest.mark.parametrize("B", [64, 320])
@pytest.mark.parametrize("U", [1, 2, 4, 8])
def test_slot_kernels_equal_the_per_tree_entry_points_and_the_host_model(U, B):
    lib = _lib().load()
    F, n = 9, 200
    cap = F * n
    prios = slot_prios(U, cap)
    A = [Tree(cap, 0, p) for p in prios]
    R = [Tree(cap, 0, p) for p in prios]
    assert A[0].nc == 2 and cap % 1024 != 0
    rng = np.random.default_rng([U, B])
    # frame 1 begins and ends inside chunk 0, frame 5 = [1000, 1200) crosses the chunk edge, frame 8 ends on the last leaf of the
    # partial chunk and retires frame 0
    for k, (t, fused) in enumerate(((1, False), (5, True), (8, True))):
        seed = (0x5EED << 32) | (40 + U) if k < 2 else M64 - 2           # (the last one wraps: slot j's key is seed + j mod 2^64)
        one_pass(lib, A, R, F, n, t, B, fused, seed, (0x3 << 32) | (t + B), 0.4 + 0.15 * k, rng)


def test_slot_kernels_on_65_chunks():
    """capacity 5 x 13 200 = 66 000: 65 chunks, so the sampler's first round covers segments of 2 chunks."""
    lib = _lib().load()
    U, F, n, B = 2, 5, 13200, 64
    prios = slot_prios(U, F * n)
    A = [Tree(F * n, 0, p) for p in prios]
    R = [Tree(F * n, 0, p) for p in prios]
    assert A[0].nc == 65
    one_pass(lib, A, R, F, n, 1, B, True, (0x77 << 32) | 5, (1 << 32) | 9, 0.7, np.random.default_rng(65))


@pytest.mark.parametrize("U", [2, 4])
def test_set_slots_runs_row_ends_and_the_gate(U):
    L = _lib()
    lib = L.load()
    cap, B = 1800, 320
    rng = np.random.default_rng([3, U])
    prios = [fx.initial_prio(cap, seed=31 + j) * (1.0 + j) for j in range(U)]
    slots = np.stack([np.sort(rng.choice(np.arange(100, cap), B, replace=False)) for _ in range(U)]).astype(np.int64)
    err = rng.uniform(0.0, 0.9, (U, B)).astype(np.float32)
    err[rng.uniform(0.0, 1.0, (U, B)) < 0.2] += 1.5                      # above the clip
    err[:, ::7] = 0.0
    for j in range(U):
        slots[j, 254:259] = slots[j, 254]                                # a run of one tree slot across the 256-thread edge
        err[j, 254:259] = [0.2, 3.0, -0.4, 0.0, 0.55 + 0.01 * j]         # distinct: the last one wins
        prios[j][slots[j, 254]] = 0.3
        slots[j, 10:13] = slots[j, 10]
    for j in range(U - 1):                                               # the last entry of slot j == the first of slot j + 1: no run
        x = 7 + j                                                        # (below 100: nowhere else in either row)
        slots[j, B - 1] = slots[j + 1, 0] = x
        prios[j][x], prios[j + 1][x] = 0.25, 0.35
        err[j, B - 1], err[j + 1, 0] = 0.125, 0.5
    A = [Tree(cap, 0, p) for p in prios]
    R = [Tree(cap, 0, p) for p in prios]
    d_slots = torch.cat([_dev(slots.reshape(-1)), torch.full((PAD,), -7, dtype=torch.int64, device=DEV)])
    d_err = _dev(err)
    word = torch.tensor([77], dtype=torch.int32, device=DEV)
    start = [tr.read().all.copy() for tr in A]

    def call(go, value):
        return lib.uavenv_per_set_f32_slots_gated(tab(A), U, d_slots.data_ptr(), d_err.data_ptr(), B, fx.EPSILON, fx.ALPHA, fx.CLIP, go,
                                                  value, stream())

    assert call(word.data_ptr(), 78) == L.OK                             # a closed gate changes no byte
    for j in range(U):
        assert fx.same_bits(A[j].read().all, start[j]), j
    assert call(word.data_ptr(), 77) == L.OK
    for j, tr in enumerate(R):
        assert lib.uavenv_per_set_f32_gated(tr.ref, d_slots.data_ptr() + 8 * j * B, d_err.data_ptr() + 4 * j * B, B, fx.EPSILON, fx.ALPHA,
                                            fx.CLIP, None, 0, stream()) == L.OK
    for j in range(U):
        g = A[j].read()
        assert fx.same_bits(g.all, R[j].read().all), j
        fx.check_set(g.prio, prios[j], slots[j], err[j], fx.EPSILON, fx.ALPHA, fx.CLIP, what=j)
        edge = g.prio[slots[j, 254]]
        assert abs(edge - (float(err[j, 258]) + fx.EPSILON) ** fx.ALPHA) < 1e-12   # the last of the run, not 0.3
    for j in range(U - 1):                                               # both sides of a row end were written, each in its own tree
        x = 7 + j
        assert abs(A[j].read().prio[x] - (0.125 + fx.EPSILON) ** fx.ALPHA) < 1e-12
        assert abs(A[j + 1].read().prio[x] - (0.5 + fx.EPSILON) ** fx.ALPHA) < 1e-12


# ------------------------------------------------------------------------------------------------ (b) the weighted gradient
@pytest.fixture(scope="module")
def hand():
    """One small hand ring (two frames of 512 agents, a quarter of the rows invalid) per action count."""
    rings = {}

    def get(A):
        if A not in rings:
            rings[A] = G.make_hand("packed", 512, np.random.default_rng(40 + A), A, invalid_frac=0.25)
            assert (rings[A].host["valid"][0] == 0).any()
        return rings[A]
    return get


def slot_weights(rng, U, B):
    w = rng.uniform(0.05, 1.0, (U, B)).astype(np.float32)
    w[:, 3::9] = 0.0                                                     # some weights exactly 0
    w[:, 0] = 1.0
    return torch.tensor(w, device="cuda").contiguous()


def abs_buf(U, B):
    return torch.full((U * B + GUARD,), -1.0, device="cuda")


def grad_slots_w(ring, nets, pairs, kind, huber, w, abs_out, parts, images=None, expect=0):
    L = _lib()
    B = pairs.shape[1]
    rc = L.load().uavenv_dqn_grad_slots_w_img(C.byref(ring._c), ring.head, ring.filled, B, 0, 0, pairs.data_ptr(), net_array(nets),
                                              len(nets), kind, G.GAMMA, huber, w.data_ptr(), abs_out.data_ptr(), ptrs(parts),
                                              None if images is None else ptrs(images), stream())
    assert rc == expect, rc


def grad_one_w(ring, net, pairs_j, kind, huber, w_j, abs_j, part, image=None):
    L = _lib()
    rc = L.load().uavenv_dqn_grad_img(C.byref(ring._c), ring.head, ring.filled, pairs_j.shape[0], 0, 0, pairs_j.data_ptr(),
                                      C.byref(net.net), kind, G.GAMMA, huber, w_j.data_ptr(), abs_j.data_ptr(), part.data_ptr(),
                                      None if image is None else image.data_ptr(), stream())
    assert rc == 0, rc


def per_slot_reference(ring, nets, pairs, kind, huber, w, images):
    U, B = pairs.shape[0], pairs.shape[1]
    want, rows = new_parts(nets[0], B, U)
    want_abs = abs_buf(U, B)
    for j in range(U):
        grad_one_w(ring, nets[j], pairs[j], kind, huber, w[j], want_abs[j * B:(j + 1) * B], want[j], None if images is None else images[j])
    torch.cuda.synchronize()
    return [bits(x) for x in want], bits(want_abs), rows


@pytest.mark.parametrize("A,dueling", HEADS, ids=lambda x: str(x))
@pytest.mark.parametrize("U", [1, 2, 4])
def test_grad_slots_w_equals_the_weighted_gradient_kernel_per_slot(hand, U, A, dueling):
    ring = hand(A)
    rng = np.random.default_rng([U, A, int(dueling), 7])
    for which, kind, huber in (("fresh", 0, 0), ("stress", 1, 1), ("fresh", 1, 0), ("stress", 0, 1)):
        nets = make_nets(A, dueling, which, U)
        images = [n.image() for n in nets]
        for B in (64, 128):
            _, pairs = hand_pairs(rng, ring, U, B)
            w = slot_weights(rng, U, B)
            want, want_abs, rows = per_slot_reference(ring, nets, pairs, kind, huber, w, images)
            P = nets[0].flat.size
            assert all(np.isfinite(x[:rows, :P + 2].view(np.float32)).all() and (x[rows:] == SENTINEL).all() for x in want)
            a = want_abs.view(np.float32)
            assert (a[:U * B] >= 0).all() and (a[U * B:] == -1.0).all() and len(np.unique(a[:U * B])) > B // 2
            for imgs in (images, None):
                got, _ = new_parts(nets[0], B, U)
                got_abs = abs_buf(U, B)
                grad_slots_w(ring, nets, pairs, kind, huber, w, got_abs, got, imgs)
                torch.cuda.synchronize()
                for j in range(U):
                    assert np.array_equal(bits(got[j]), want[j]), (which, kind, huber, B, j, imgs is None)
                assert np.array_equal(bits(got_abs), want_abs), (which, kind, huber, B, imgs is None)
            if B == 128:                      # the weights count: the unweighted launch writes other rows, the same |TD|
                plain, _ = new_parts(nets[0], B, U)
                plain_abs = abs_buf(U, B)
                grad_slots_w(ring, nets, pairs, kind, huber, torch.ones_like(w), plain_abs, plain, images)
                torch.cuda.synchronize()
                assert all(not np.array_equal(bits(plain[j]), want[j]) for j in range(U))
                assert np.array_equal(bits(plain_abs), want_abs)


@pytest.mark.parametrize("with_images", [True, False])
def test_grad_slots_w_persistent_workgroups(hand, with_images):
    """64 x 258 samples per slot: 258 tiles on 256 workgroups, so workgroups 0 and 1 of every slot take a second tile."""
    U, A, B = 2, 3, 64 * 258
    ring = hand(A)
    nets = make_nets(A, False, "stress", U)
    images = [n.image() for n in nets] if with_images else None
    rng = np.random.default_rng(258)
    _, pairs = hand_pairs(rng, ring, U, B)
    w = slot_weights(rng, U, B)
    want, want_abs, rows = per_slot_reference(ring, nets, pairs, 1, 0, w, images)
    assert rows == 256
    got, _ = new_parts(nets[0], B, U)
    got_abs = abs_buf(U, B)
    grad_slots_w(ring, nets, pairs, 1, 0, w, got_abs, got, images)
    torch.cuda.synchronize()
    for j in range(U):
        assert np.array_equal(bits(got[j]), want[j]) and (want[j][rows:] == SENTINEL).all()
    assert np.array_equal(bits(got_abs), want_abs)


@pytest.mark.parametrize("A,dueling", HEADS, ids=lambda x: str(x))
def test_grad_slots_w_against_f64(hand, A, dueling):
    lib = _lib().load()
    U, B = 2, 128
    ring = hand(A)
    kind = 1 if dueling or A == 4 else 0
    kind_name = "dueling" if dueling else ("ddqn" if kind else "dqn")
    nets = make_nets(A, dueling, "stress" if A != 2 else "fresh", U)
    images = [n.image() for n in nets]
    rng = np.random.default_rng([65, A, int(dueling)])
    fa, pairs = hand_pairs(rng, ring, U, B)
    w = slot_weights(rng, U, B)
    parts, rows = new_parts(nets[0], B, U)
    abs_out = abs_buf(U, B)
    grad_slots_w(ring, nets, pairs, kind, 0, w, abs_out, parts, images)
    P = nets[0].flat.size
    for j in range(U):
        raw = torch.empty(P + 2, device="cuda")
        assert lib.uavenv_dqn_reduce(C.byref(nets[j].net), parts[j].data_ptr(), rows, raw.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        raw, abs_td = raw.cpu().numpy(), abs_out[j * B:(j + 1) * B].cpu().numpy()
        hb = G.host_batch(ring, (fa[0][j], fa[1][j]), w[j], False)
        fl = nets[j].buf[:2, :P].cpu().numpy().astype(np.float64)
        kw = dict(kind=kind_name, dueling=dueling, n_actions=A, gamma=float(np.float32(G.GAMMA)), huber=False,
                  relu_eps=G.F32["relu_eps"], tie_eps=G.F32["tie_eps"])
        args = (hb["s"], hb["s2"], hb["actions"], hb["rewards"], hb["dones"], hb["valid"], fl[0], fl[1])
        r = dqn_grad_f64(*args, is_weights=hb["is_weights"], **kw)
        if r["near_tie"].any():               # (as run_case: a DDQN argmax within tie_eps is held to the kernel's own choice)
            alt = np.abs(abs_td - np.abs(r["delta_alt"])) < np.abs(abs_td - r["abs_td"])
            na = np.where(r["near_tie"], np.where(alt, r["a_alt"], r["a_next"]), -1)
            r = dqn_grad_f64(*args, is_weights=hb["is_weights"], next_action=na, **kw)
        ok, worst = G.check_a(raw, abs_td, r, P, G.F32)
        print("slot", j, "worst ratio", round(worst, 4))
        assert ok, (A, dueling, j, worst, raw[P + 1], r["count"])
        assert 0 < r["count"] < B


# ------------------------------------------------------------------------------------------------ (c) the loop
def make_pers(ring, U, **kw):
    from dqn_based_uav_3d_path_planer_amd.replay import DevicePER
    return [DevicePER(ring.frames * (ring.env.N // U), device="cuda:0", tree_order=False, **kw) for _ in range(U)]


def compose_per(ring, Ls, pers, passes, batch, seed, eps, counter0=0, learn_start=0):
    """The prioritised passes as the per-tree entry points give them, issued from here: per slot the act (as compose), the step,
    then per slot uavenv_per_fill_frame_strided -- or, on a learning pass, uavenv_per_rebuild_frame, uavenv_per_sample under
    seed + 7 + j, uavenv_per_weights over (frame, env) with the env mapped to agent env * U + j, the weighted update
    (uavenv_dqn_grad_w, uavenv_dqn_reduce_adam) and uavenv_per_set_f32_gated.  -> beta"""
    lib = _lib().load()
    U, B = len(Ls), batch
    n_envs = ring.env.N // U
    p0 = pers[0]
    beta = p0.beta
    per_new = math.pow(0.0 + p0.epsilon, p0.alpha)
    bufs = [p.make_bufs(B) for p in pers]
    for c in range(counter0, counter0 + passes):
        obs, act = ring.current_obs(), ring.current_action()
        for j, Lj in enumerate(Ls):
            a = torch.empty(n_envs, dtype=torch.int32, device="cuda")
            Lj.act(obs[j::U].contiguous(), eps, (seed + j) & M64, c, index_out=a)
            act[j::U] = a
        t = ring.head
        ring.step_env(auto_reset=False, skip_done=True)
        nxt = ring.head
        valid_t = ring.valid[t]
        learn = ring.filled * n_envs >= max(learn_start, B)
        if learn:
            beta = beta + p0.beta_inc if beta + p0.beta_inc < 1.0 else 1.0
        for j, (Lj, p, b) in enumerate(zip(Ls, pers, bufs)):
            per = C.byref(p._c)
            if not learn:
                assert lib.uavenv_per_fill_frame_strided(per, t * n_envs, n_envs, per_new, valid_t.data_ptr() + j, U, nxt * n_envs,
                                                         stream()) == 0
                continue
            col = valid_t[j::U].contiguous()
            assert lib.uavenv_per_rebuild_frame(per, t * n_envs, n_envs, per_new, col.data_ptr(), nxt * n_envs, stream()) == 0
            assert lib.uavenv_per_sample(per, B, None, (seed + 7 + j) & M64, c, b["slots"].data_ptr(), b["prio"].data_ptr(), stream()) == 0
            assert lib.uavenv_per_weights(per, b["slots"].data_ptr(), b["prio"].data_ptr(), B, ring.filled * n_envs, beta, n_envs,
                                          b["w"].data_ptr(), b["pairs"].data_ptr(), stream()) == 0
            b["pairs"][:, 1] = b["pairs"][:, 1] * U + j
            Lj.learn_from_ring(ring, B, seed, c, explicit_idx=b["pairs"], is_weights=b["w"], abs_td_out=b["abs"])
            assert lib.uavenv_per_set_f32_gated(per, b["slots"].data_ptr(), b["abs"].data_ptr(), B, p.epsilon, p.alpha, p.clip, None, 0,
                                                stream()) == 0
    torch.cuda.synchronize()
    return beta


def age(env, ring):
    """Every third agent is put 3 .. 13 steps before Max_Step (the same in every env built alike): it loses within the run, is
    skipped from then on and never restarted -- its later rows are invalid.  Called after the first pass: the first step after a
    reset pops the sub-goal that aliases the position, which sets Step back to 0."""
    from dqn_based_uav_3d_path_planer_amd.data import load_city26
    max_step = int(load_city26()["max_step"])
    st, sub, alias = env.get_state(0, env.N, want_sub=True)
    step = st[:, 9].astype(np.int32)
    i = np.arange(env.N)
    step[i % 3 == 0] = max_step - 3 - (i[i % 3 == 0] % 11)
    env.set_state(0, st[:, [0, 1, 2, 3, 4, 6, 7, 8]], step, st[:, 11].astype(np.int32), sub, alias)
    env.observe(ring.obs[ring.head])


def tree_state(p):
    return [p.prio, p._chunk_sum, p._chunk_prefix, p._group_sum]


@pytest.mark.parametrize("U,batch,net,kind", [(4, 64, "Qnet2", "dqn"), (2, 128, "VAnet2", "dueling")])
def test_per_loop_equals_the_composition(U, batch, net, kind):
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    n_envs, passes, seed, eps = 200, 23, 9, 0.2
    env_a, ring_a, La = build(n_envs, U, net, kind)
    assert ring_a.frames == 9 and env_a.N == n_envs * U                  # 23 passes: the ring wraps twice
    pers_a = make_pers(ring_a, U)
    pers_a[0].beta = compose_per(ring_a, La, pers_a, 1, batch, seed, eps)
    age(env_a, ring_a)
    beta_a = compose_per(ring_a, La, pers_a, passes - 1, batch, seed, eps, counter0=1)
    env_b, ring_b, Lb = build(n_envs, U, net, kind)
    pers_b = make_pers(ring_b, U)
    loop = DQNSlotsHotLoop(ring_b, Lb, batch, seed=seed, eps=eps, auto_reset=False, skip_done=True, pers=pers_b, multi_update=False)
    assert loop.multi_update                                             # implied by the trees
    with pytest.raises(_lib().UavEnvError):
        loop.set_multi_update(False)
    assert loop.multi_update
    loop.run(1)
    age(env_b, ring_b)
    loop.run(9)
    assert loop.in_sync(batch)
    loop.run(passes - 10)
    torch.cuda.synchronize()
    assert (ring_b.head, ring_b.filled, loop.counter) == (ring_a.head, ring_a.filled, passes)
    assert [x.epoch for x in Lb] == [x.epoch for x in La] and 0 < La[0].epoch <= passes
    for name in ("obs", "action", "reward", "done", "valid"):
        assert torch.equal(getattr(ring_a, name), getattr(ring_b, name)), name
    live = [(ring_b.head - 1 - k) % ring_b.frames for k in range(ring_b.filled)]
    assert not bool(ring_b.valid[live].all()) and bool(ring_b.valid[live].any())     # invalid rows exist
    for j, (a, b) in enumerate(zip(La, Lb)):
        assert torch.equal(a.flat, b.flat), j                            # parameters, target, moments
        assert float(a.loss) == float(b.loss) and np.isfinite(float(b.loss)), j
    assert len({float(x.flat[0].sum()) for x in Lb}) == U
    updates = La[0].epoch
    for j, (a, b) in enumerate(zip(pers_a, pers_b)):
        for x, y in zip(tree_state(a), tree_state(b)):
            assert torch.equal(x, y), j
        assert b.beta == beta_a
        assert b.n_entries == ring_b.filled * n_envs
        pr = b.prio.view(ring_b.frames, n_envs)
        assert bool((pr >= 0).all()) and bool(torch.isfinite(pr).all()) and bool((pr[ring_b.head] == 0).all())
        assert bool((pr[ring_b.valid.view(ring_b.frames, n_envs, U)[:, :, j] == 0] == 0).all())       # invalid rows carry priority 0
        assert bool((pr > 0).any())
    assert abs(beta_a - (0.4 + updates * 0.001)) < 1e-12 and pers_b[0].beta == beta_a
    assert len({float(p.prio.sum()) for p in pers_b}) == U
    loop.close()
    env_a.close()
    env_b.close()


def test_gated_per_loop_with_every_agent_finished():
    """With every agent finished the learners stay as they are, and the priorities too, apart from fill and retire."""
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    U, n_envs = 2, 64
    env, ring, Ls = build(n_envs, U, "Qnet2", "dqn")
    pers = make_pers(ring, U)
    loop = DQNSlotsHotLoop(ring, Ls, 64, seed=6, eps=0.3, auto_reset=False, skip_done=True, gate_updates=True, pers=pers)
    w0 = [L.flat.clone() for L in Ls]
    for _ in range(1500):                      # no restarts: the episode ends for every agent; stop within 2 passes of that
        loop.run(2)
        torch.cuda.synchronize()
        if not bool(ring.valid[(ring.head - 1) % ring.frames].any()):
            break
    assert not bool(ring.valid[(ring.head - 1) % ring.frames].any()), "the episode did not end"
    assert not any(torch.equal(L.flat, w) for L, w in zip(Ls, w0))
    w1, l1, e1 = [L.flat.clone() for L in Ls], [float(L.loss) for L in Ls], [L.epoch for L in Ls]
    p1, beta1 = [p.prio.clone() for p in pers], pers[0].beta
    t0 = ring.head
    loop.run(2)
    torch.cuda.synchronize()
    assert all(torch.equal(L.flat, w) for L, w in zip(Ls, w1)) and [float(L.loss) for L in Ls] == l1
    assert [L.epoch for L in Ls] == [e + 2 for e in e1]                  # (the host's counts go on, as without trees)
    assert abs(pers[0].beta - min(1.0, beta1 + 2 * 0.001)) < 1e-12        # (beta is the host's too: it moves with the passes)
    left = 0
    for p, before in zip(pers, p1):
        want = before.view(ring.frames, n_envs).clone()
        for k in range(3):                     # frames t0, t0 + 1 were written by nobody (valid 0), t0 + 1, t0 + 2 retired
            want[(t0 + k) % ring.frames] = 0.0
        assert torch.equal(p.prio.view(ring.frames, n_envs), want)
        left += int((want > 0).sum())
    assert left > 0                            # ... and there was something to leave alone (in the tree of the last slot to finish)
    loop.close()
    env.close()


def test_a_loop_without_trees_is_the_uniform_loop():
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    U, batch, passes, seed, eps = 2, 64, 12, 9, 0.2
    env_a, ring_a, La = build(200, U, "Qnet2", "dqn")
    compose(ring_a, La, passes, batch, seed, eps, True, True, False)
    env_b, ring_b, Lb = build(200, U, "Qnet2", "dqn")
    loop = DQNSlotsHotLoop(ring_b, Lb, batch, seed=seed, eps=eps, pers=[None] * U)
    assert not loop.multi_update and loop._pers is None
    beta = C.c_double(-1.0)
    assert loop.lib.uavenv_dqn_slots_loop_get_per(loop._h, C.byref(beta)) == 0 and beta.value == 0.0
    loop.run(passes)
    torch.cuda.synchronize()
    for name in ("obs", "action", "reward", "done", "valid"):
        assert torch.equal(getattr(ring_a, name), getattr(ring_b, name)), name
    for a, b in zip(La, Lb):
        assert torch.equal(a.flat, b.flat) and float(a.loss) == float(b.loss) and a.epoch == b.epoch == passes
    loop.close()
    env_a.close()
    env_b.close()


def test_set_per_refusals_leave_the_loop_as_it_was():
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    L = _lib()
    lib = L.load()
    E = L.EINVAL
    env, ring, Ls = build(64, 2, "Qnet2", "dqn")
    n_envs, B = 64, 64
    pers = make_pers(ring, 2)
    keep = []
    bufs = (torch.zeros((2, B), dtype=torch.int64, device="cuda"), torch.zeros((2, B + 1), dtype=torch.float64, device="cuda"),
            torch.zeros((2, B), dtype=torch.float32, device="cuda"), torch.zeros((2, B), dtype=torch.float32, device="cuda"))

    def per_cfg(mut=None):
        pc = L.UavDqnSlotsPer()
        for j, p in enumerate(pers):
            pc.per[j] = p._c
        pc.slots_dev, pc.prio_dev, pc.w_dev, pc.abs_dev = (t.data_ptr() for t in bufs)
        pc.alpha, pc.beta, pc.beta_inc, pc.eps, pc.clip = 0.6, 0.4, 0.001, 0.01, 1.0
        if mut:
            mut(pc)
        return pc

    def loop_of(mut=None, learners=Ls):
        cfg = good_cfg(ring, learners, B, keep)
        cfg.step_flags = L.STEP_SKIP_DONE
        if mut:
            mut(cfg)
        h = C.c_void_p()
        assert lib.uavenv_dqn_slots_loop_create(C.byref(cfg), C.byref(h)) == 0
        return h

    h = loop_of()
    beta = C.c_double(-1.0)
    muts = {
        "another capacity": lambda pc: setattr(pc.per[1], "capacity", ring.frames * n_envs - 1),
        "capacity of the whole ring": lambda pc: [setattr(pc.per[j], "capacity", ring.frames * env.N) for j in range(2)],
        "no priorities": lambda pc: setattr(pc.per[0], "prio", None),
        "tree order": lambda pc: setattr(pc.per[1], "rot", 3),
        "group sums on one tree only": lambda pc: setattr(pc.per[1], "group_sum", None),
        "one tree twice": lambda pc: setattr(pc.per[1], "prio", pc.per[0].prio),
        "no slots buffer": lambda pc: setattr(pc, "slots_dev", None),
        "no prio buffer": lambda pc: setattr(pc, "prio_dev", None),
        "no weights buffer": lambda pc: setattr(pc, "w_dev", None),
        "no |TD| buffer": lambda pc: setattr(pc, "abs_dev", None),
    }
    for name, mut in muts.items():
        assert lib.uavenv_dqn_slots_loop_set_per(h, C.byref(per_cfg(mut))) == E, name
        assert lib.uavenv_dqn_slots_loop_set_multi_update(h, 0) == 0, name       # left as it was: still the uniform loop
        assert lib.uavenv_dqn_slots_loop_get_per(h, C.byref(beta)) == 0 and beta.value == 0.0
    assert lib.uavenv_dqn_slots_loop_set_per(h, C.byref(per_cfg())) == 0
    assert lib.uavenv_dqn_slots_loop_get_per(h, C.byref(beta)) == 0 and beta.value == 0.4
    assert lib.uavenv_dqn_slots_loop_set_multi_update(h, 0) == E and lib.uavenv_dqn_slots_loop_set_multi_update(h, 1) == 0
    assert lib.uavenv_dqn_slots_loop_set_per(h, None) == 0                       # NULL turns it off again
    assert lib.uavenv_dqn_slots_loop_set_multi_update(h, 0) == 0
    assert lib.uavenv_dqn_slots_loop_get_per(h, None) == E
    lib.uavenv_dqn_slots_loop_destroy(h)
    # the loop's own side: no valid plane, no batch, heads of more than 4 layer-2 outputs
    h = loop_of(lambda c: setattr(c.ring, "valid", None))
    assert lib.uavenv_dqn_slots_loop_set_per(h, C.byref(per_cfg())) == E
    lib.uavenv_dqn_slots_loop_destroy(h)
    h = loop_of(lambda c: setattr(c, "batch", 0))
    assert lib.uavenv_dqn_slots_loop_set_per(h, C.byref(per_cfg())) == E
    lib.uavenv_dqn_slots_loop_destroy(h)
    five = [FusedDQNLearner(dict(PARAM, NetWork="Qnet2", output="5"), "dqn", device="cuda:0") for _ in range(2)]
    h = loop_of(learners=five)
    assert lib.uavenv_dqn_slots_loop_set_per(h, C.byref(per_cfg())) == E
    lib.uavenv_dqn_slots_loop_destroy(h)
    torch.cuda.synchronize()
    assert all(float(p.prio.abs().sum()) == 0.0 for p in pers)                   # nothing was enqueued
    env.close()


def test_update_slots_weighted_equals_learn_from_ring_per_learner():
    from dqn_based_uav_3d_path_planer_amd.learner import update_slots
    U, B, n_envs = 2, 128, 100
    env_a, ring_a, La = build(n_envs, U, "Qnet2", "dqn")
    env_b, ring_b, Lb = build(n_envs, U, "Qnet2", "dqn")
    gen = torch.Generator(device="cuda").manual_seed(3)
    for _ in range(6):
        a = torch.randint(0, 3, (env_a.N,), generator=gen, device="cuda", dtype=torch.int32)
        for r in (ring_a, ring_b):
            r.current_action().copy_(a)
            r.step_env(auto_reset=True)
    rng = np.random.default_rng(5)
    for step in range(2):
        f = (ring_a.head - 1 - rng.integers(0, ring_a.filled, (U, B))) % ring_a.frames
        agent = rng.integers(0, n_envs, (U, B)) * U + np.arange(U)[:, None]
        pairs = torch.tensor(np.stack([f, agent], 2).astype(np.int32), device="cuda").contiguous()
        w = slot_weights(rng, U, B)
        abs_a, abs_b = torch.full((U, B), -1.0, device="cuda"), torch.full((U, B), -1.0, device="cuda")
        for j in range(U):
            La[j].learn_from_ring(ring_a, B, 0, 0, explicit_idx=pairs[j], is_weights=w[j], abs_td_out=abs_a[j])
        update_slots(Lb, ring_b, B, pairs, is_weights=w, abs_td_out=abs_b)
        torch.cuda.synchronize()
        assert torch.equal(abs_a, abs_b) and bool((abs_b >= 0).all())
        for j in range(U):
            assert torch.equal(La[j].flat, Lb[j].flat) and La[j].epoch == Lb[j].epoch == step + 1
            assert float(La[j].loss) == float(Lb[j].loss) and np.isfinite(float(Lb[j].loss))
    env_a.close()
    env_b.close()


# ------------------------------------------------------------------------------------------------ (d) the plugin
def test_plugin_fused_slots_with_prioritised_replay(tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver
    monkeypatch.chdir(tmp_path)
    xml = driver.make_config_dir(str(tmp_path), "DQN", num_envs=256, num_uav=2)
    s = open(xml).read()
    open(xml, "w").write(s.replace("<seed>42</seed>", "<seed>42</seed>\n        <fused_slots>1</fused_slots>"))
    t = tmp_path / "config" / "Trainer.xml"
    ts, n = re.subn(r"<Batch_Size>64</Batch_Size>", "<Batch_Size>64</Batch_Size>\n    <IsPriority_Replay>1</IsPriority_Replay>", t.read_text())
    assert n == 1
    t.write_text(ts)
    env = driver.simulator(xml).env
    assert env is not None and env.fast_slots and not env.fast and not env.fast_sac and env.backend.packed
    assert all(u.Trainer.IsPriority_Replay == 1 for u in env.Agents) and len(env._slots_per) == 2
    pers, ring = env._slots_per, env._ring
    beta0, inc = pers[0].beta, pers[0].beta_inc
    e0 = [u.Trainer.epoch for u in env.Agents]
    steps = 0
    for eps in (0.5, 0.3):
        res = env.run_eposide(eps)
        assert env.slots_loop_with_per is True
        assert env.Check_uav_Done() and np.isfinite(float(res["loss"]))
        steps += env.steps_last_episode
        assert 1 <= env.surplus_passes_last_episode <= env.done_check
    torch.cuda.synchronize()
    # one update per moving step on every trainer (256 envs: the ring holds a batch from the first step on)
    updates = [u.Trainer.epoch - e for u, e in zip(env.Agents, e0)]
    assert len(set(updates)) == 1 and updates[0] == steps and steps > 100
    live = [(ring.head - 1 - k) % ring.frames for k in range(ring.filled)]
    stored = 0
    for j, p in enumerate(pers):
        assert abs(p.beta - min(1.0, beta0 + updates[0] * inc)) < 1e-9
        assert p.n_entries == ring.filled * env.num_envs
        pr = p.prio.view(ring.frames, env.num_envs)
        assert bool(torch.isfinite(pr).all()) and bool((pr >= 0).all())
        col = ring.valid.view(ring.frames, env.num_envs, 2)[:, :, j]
        assert bool((pr[col == 0] == 0).all())                           # invalid rows carry priority 0
        assert bool(((pr[live] > 0) == (col[live] != 0)).all())          # ... and every stored transition of the slot a positive one
        stored += int((pr > 0).sum())
    assert stored > 0                      # (a slot whose agents all finished a ring's length before the end has none left)
    w = [u.Trainer.learner.flat[0] for u in env.Agents]
    assert not torch.equal(w[0], w[1])
