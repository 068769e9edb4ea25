"""The multi-GPU update path at kernel level, against float64 and against bit-exact f32 references (oracle/exchange_ref.py): the
split form uavenv_dqn_reduce -> all-reduce -> uavenv_dqn_adam (k_dqn_reduce, k_dqn_adam of csrc/learner.hip) and the on-stream peer
exchange of csrc/p2p.hip (k_p2p_reduce_push, k_p2p_pull_adam, k_p2p_push, k_p2p_pull_sum, k_p2p_hash_blocks), through the C ABI.
The partial rows are a plain float matrix, so the tests write them themselves: no environment, ring or gradient kernel.

ALL of this is same-device evidence: one process, or two / three ranks sharing ONE GPU whose receive areas are mapped through HIP
IPC.  It pins the kernels' arithmetic, indexing and protocol; it says nothing about a link between devices.

Part A, one process (a UavP2P of world 1 is connected without IPC), nets covering the four residues of (P + 2) mod 4 -- where the
checksum words P + 2, P + 3 fall inside a storing lane's 16 bytes -- and n_partials in {1, 31, 32, 33, 255, 256, 257, 600} (above 256
the reductions' `b0 += 256` loop runs a second and third trip):
 (a) uavenv_dqn_reduce: the raw bucket against the f64 column sums within column_sum_bound = gamma_depth sum_b |x_bp|,
     depth = 8 ceil(n / 256) + 10, counted from reduce_columns: a thread adds 8 rows per 256-row trip into its accumulator, the 32
     row groups are folded 4 -> 1 by two levels of pairwise adds, and lane p adds the 8 results one after another from zero.  The
     count exactly; the NaN pad columns reach no output; nothing is written behind P + 2.
 (b) uavenv_dqn_reduce_p2p + uavenv_dqn_adam_p2p(step_t = 0) at world 1: raw_out equals (a)'s bucket BIT FOR BIT, four calls back to
     back with different payloads (both parity slots twice).  k_p2p_reduce_push carries a hand copy of reduce_columns' summation:
     read side by side the two associate identically (the build forbids contraction), so bit equality is what ties them together.
 (c) the three Adam forms (uavenv_dqn_adam on (a)'s bucket, uavenv_dqn_adam_p2p, uavenv_dqn_reduce_adam) from non-zero moments, at
     step 5 with a hard update and step 4 without, against adam_step_f64 with gerr = column_sum_bound / count + 2^-23 |gbar|; the
     loss = f32(loss sum) * (1 / max(count, 1)) bit for bit; a divide by count +- 1 is rejected; total counts 0 and 1.
 (d) the *_img entry points: the layer-1 image after the step equals uavenv_dqn_split_image of the stepped net bit for bit (target
     half untouched without a hard update); weights, moments, target as with a null image.
 (e) uavenv_dqn_reduce_adam_gated: a closed gate leaves everything bitwise alone, an open one or a NULL word equals
     uavenv_dqn_reduce_adam.
 (f) the sticky error word (a software flag): uavenv_dqn_reduce_p2p returns EP2P and enqueues nothing, uavenv_dqn_adam_p2p leaves
     weights, moments, target, image and loss alone.  (This found a defect: behind a refused push the pull re-uses the last sequence
     number, whose healthy verdict every workgroup but the first took from the verdict word -- and stepped.)
 (g) uavenv_p2p_allreduce at world 1 over the sizes around k_p2p_pull_sum's grid-stride trip (32 768 floats = one trip of the capped
     32 x 256 grid), canaries, refusals; and the two parity slots are two: a slot written at sequence k survives sequence k + 1.
Part B, worlds 2 and 3 on one GPU (one spawn per world, every scenario on a fresh handle):
 (h) uavenv_p2p_allreduce = rank_order_sum_f32 of all ranks' payloads bit for bit, (g)'s sizes, four calls each.
 (i) the DQN bucket with 1 / 257 / 600 rows on ranks 0 / 1 / 2: raw_out = rank-order f32 sum of the per-rank buckets bit for bit.
 (j) a real uavenv_dqn_adam_p2p_img step against adam_step_f64 on (f64 sum over ranks) / (total count); the host rejects the total
     count +- 1, the mean over one rank's own count, a dropped and a doubled rank; (d)'s image property; ranks bit-identical.
 (k) checksum sensitivity at check_every = 1: one flipped mantissa bit of parameter P - 1 on the last rank, or two parameters swapped
     on rank 0 (same multiset of bit patterns: only position tells), raise DIVERGED on every rank within two steps; weights freeze.
 (l) uavenv_p2p_check_blocks with three unequal blocks: one ulp on the last float of the last block, a swap between blocks at the
     same index (only the block number tells) and a swap inside a block (only the index tells).

Worst measured ratio (error / bar) per kernel over the cases below, on an MI355X (printed with -s):
  k_dqn_reduce 0.228 (n = 32; 0.044 at n = 600)       k_p2p_reduce_push + k_p2p_pull_adam: no bit differs from k_dqn_reduce's bucket
  k_dqn_adam 0.452   k_p2p_pull_adam 0.452   k_dqn_reduce_adam 0.452      (check_adam's worst component, the same to four digits)
  k_p2p_pull_adam at world 2 / 3: 0.438 / 0.438       k_p2p_push + k_p2p_pull_sum, worlds 1 / 2 / 3: no bit differs
"""
import ctypes as C
import functools
import hashlib
import json
import os
import socket

import numpy as np
import pytest
import torch

from oracle.exchange_ref import column_sum_bound, partials, payload, rank_order_sum_f32, reduce_depth
from test_dqn_grad_kernels_gpu import check_adam, check_target

pytestmark = pytest.mark.gpu

NETS = {"plain2": (2, 0), "plain3": (3, 0), "duel3": (3, 1), "plain9": (9, 0)}      # (P + 2) mod 4 = 0, 1, 2, 3
SIZES = (1, 31, 32, 33, 255, 256, 257, 600)
CASES = [("plain3", n) for n in SIZES] + [(k, n) for k in ("plain2", "duel3", "plain9") for n in (1, 257, 600)]
COUNTS = (4, 1020, 1024, 1028, 32768, 32772)            # + bucket_pad, the largest size accepted
AR_BUCKET = 32772
AR_PAD = (AR_BUCKET + 2 + 63) & ~63                      # uavenv_p2p_create's padding of a slot
ROWS = (1, 257, 600)                                     # part B: partial rows of ranks 0, 1, 2
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
CANARY = -77.25
MAX_COUNT = 16384           # a 1 / count scale of the mean gradient stays above the step's f32 rounding (as at B = 16 384)
WORST = {}


def _L():
    from dqn_based_uav_3d_path_planer_amd import _lib
    return _lib


def _s():
    return torch.cuda.current_stream().cuda_stream


def dev(x):
    return torch.tensor(np.ascontiguousarray(x), device="cuda")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


class Net:
    """A UavDqnNet on plain tensors: rows local, target, m, v of a padded [4, P] block (every row 16-byte aligned)."""

    def __init__(self, key):
        L = _L()
        self.lib = L.load()
        A, duel = NETS[key]
        n2 = A + duel
        self.P = P = 64 * 100 + 64 + n2 * 64 + n2
        self._pad = torch.zeros((4, (P + 3) & ~3), device="cuda")
        self.flat = self._pad[:, :P]
        self.net = L.UavDqnNet(self.flat[0].data_ptr(), self.flat[1].data_ptr(), self.flat[2].data_ptr(), self.flat[3].data_ptr(),
                               100, 64, A, duel, L.MFMA_F32, 0)
        assert self.lib.uavenv_dqn_num_params(C.byref(self.net)) == P
        self.stride = self.lib.uavenv_dqn_partial_stride(C.byref(self.net))
        self.w_init = (np.random.default_rng([7, P]).standard_normal(P) * 0.1).astype(np.float32)

    def set_state(self, w, t, m, v):
        with torch.no_grad():
            for k, x in enumerate((w, t, m, v)):
                self.flat[k].copy_(dev(np.asarray(x, dtype=np.float32)))

    def state(self):
        torch.cuda.synchronize()
        return self.flat.cpu().numpy()

    def image(self):
        img = torch.zeros(2 * _L().DQN_IMAGE_FLOATS, device="cuda")
        assert self.lib.uavenv_dqn_split_image(C.byref(self.net), img.data_ptr(), _s()) == 0
        torch.cuda.synchronize()
        return img


@functools.lru_cache(maxsize=None)
def net(key):
    return Net(key)


@pytest.fixture(scope="module", autouse=True)
def _report_and_release():
    """The worst ratios of the module (shown with -s); the cached nets and partial rows live for this module only."""
    yield
    print("\nworst ratios (error / bar)", {k: round(v, 4) for k, v in sorted(WORST.items())})
    case.cache_clear()
    net.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def reduce_bucket(N, parts_dev, n):
    """uavenv_dqn_reduce -> P + 2 floats (64 canaries behind them must survive)."""
    raw = torch.full((N.P + 2 + 64,), CANARY, device="cuda")
    assert N.lib.uavenv_dqn_reduce(C.byref(N.net), parts_dev.data_ptr(), n, raw.data_ptr(), _s()) == 0
    torch.cuda.synchronize()
    r = raw.cpu().numpy()
    assert np.all(r[N.P + 2:] == np.float32(CANARY)), "uavenv_dqn_reduce wrote behind P + 2"
    return r[:N.P + 2].copy()


@functools.lru_cache(maxsize=3)
def case(key, n, call=0):
    """One rank's partial rows, their device copy, uavenv_dqn_reduce's bucket, the f64 column sums and the summation bound."""
    N = net(key)
    x = partials(0, n, N.P, N.stride, call=call, count_hi=min(64, MAX_COUNT // n))
    xd = dev(x)
    return dict(x=x, dev=xd, raw=reduce_bucket(N, xd, n), exact=x[:, :N.P + 2].astype(np.float64).sum(axis=0),
                bound=column_sum_bound(x[:, :N.P + 2], reduce_depth(n)))


def p2p_open(bucket, check_every=0):
    L = _L()
    lib, h = L.load(), C.c_void_p()
    assert lib.uavenv_p2p_create(1, 0, bucket, C.byref(h)) == 0
    assert lib.uavenv_p2p_configure(h, check_every, 0) == 0
    return h


def p2p_status(lib, h):
    out = (C.c_int32 * 4)()
    assert lib.uavenv_p2p_status(h, 1, out) == 0
    return {"code": int(out[0]), "timeouts": int(out[1]), "mismatches": int(out[2]), "checks": int(out[3])}


def pull_raw(N, h):
    """uavenv_dqn_adam_p2p(step_t = 0): the summed bucket only."""
    out = torch.full((N.P + 2 + 64,), CANARY, device="cuda")
    rc = N.lib.uavenv_dqn_adam_p2p(C.byref(N.net), h, 0.0, 0.9, 0.999, 1e-8, 0, 0, None, out.data_ptr(), _s())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[N.P + 2:] == np.float32(CANARY)), "the pull wrote behind P + 2"
    return rc, o[:N.P + 2].copy()


# ---- (a) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n", CASES)
def test_a_column_sums_against_f64(key, n):
    N, d = net(key), case(key, n)
    raw, P = d["raw"], N.P
    assert not np.isnan(raw).any(), "a NaN pad column reached the bucket"
    err = np.abs(raw[:P + 1].astype(np.float64) - d["exact"][:P + 1])
    ratio = float((err / (d["bound"][:P + 1] + 1e-300)).max())
    record("k_dqn_reduce", ratio)
    print(key, n, "k_dqn_reduce worst error / bound", round(ratio, 4))
    assert ratio <= 1.0
    assert raw[P + 1] == d["exact"][P + 1] and d["exact"][P + 1] <= MAX_COUNT
    if n > 1:       # resolving power: the same bar rejects the sums with the last row left out, in every column where that row's
        #             value exceeds the bar (2^e spread over 25 octaves against ~2^-19 of the column's |.|-sum: more than a quarter)
        err = np.abs(raw[:P + 1].astype(np.float64) - (d["exact"] - d["x"][-1, :P + 2].astype(np.float64))[:P + 1])
        assert np.mean(err > d["bound"][:P + 1]) > 0.25


# ---- (b) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n", CASES)
def test_b_push_pull_at_world_1_is_the_bucket_bit_for_bit(key, n):
    N = net(key)
    lib, h = N.lib, p2p_open(N.P + 2)
    try:
        for call in range(4):
            d = case(key, n, call)
            assert lib.uavenv_dqn_reduce_p2p(C.byref(N.net), d["dev"].data_ptr(), n, h, _s()) == 0
            rc, o = pull_raw(N, h)
            assert rc == 0
            assert same(o, d["raw"]), (call, int(np.sum(bits(o) != bits(d["raw"]))))
        st = p2p_status(lib, h)
        assert st["code"] == 0 and st["timeouts"] == 0 and st["mismatches"] == 0
    finally:
        lib.uavenv_p2p_destroy(h)


# ---- (c) (d) (e): the Adam forms ---------------------------------------------------------------------------------------------
def moments(gbar, P):
    rng = np.random.default_rng(5)
    m0 = (gbar * rng.choice([-1.0, 1.0], P) * rng.uniform(0.5, 1.5, P)).astype(np.float32)
    v0 = (gbar * gbar * rng.uniform(0.5, 2.0, P)).astype(np.float32)
    return m0, v0


def run_form(N, form, xd, n, t, hard, h=None, img=None, gate=None, entry=None):
    """One update through `form` from the net's present state -> (state [4, P], loss bits, raw bucket or None, rc).
    gate = (word tensor or None, go_value): the gated entry points."""
    lib, P = N.lib, N.P
    loss = torch.full((1,), CANARY, device="cuda")
    raw = torch.full((P + 2 + 64,), CANARY, device="cuda")
    nb, ip = C.byref(N.net), None if img is None else img.data_ptr()
    a = (LR, BETAS[0], BETAS[1], EPS, t, 1 if hard else 0)
    if form == "split":
        assert lib.uavenv_dqn_reduce(nb, xd.data_ptr(), n, raw.data_ptr(), _s()) == 0
        if img is None:
            rc = lib.uavenv_dqn_adam(nb, raw.data_ptr(), *a, loss.data_ptr(), _s())
        else:
            rc = lib.uavenv_dqn_adam_img(nb, raw.data_ptr(), *a, loss.data_ptr(), ip, _s())
    elif form == "p2p":
        assert lib.uavenv_dqn_reduce_p2p(nb, xd.data_ptr(), n, h, _s()) == 0
        if img is None:
            rc = lib.uavenv_dqn_adam_p2p(nb, h, *a, loss.data_ptr(), raw.data_ptr(), _s())
        else:
            rc = lib.uavenv_dqn_adam_p2p_img(nb, h, *a, loss.data_ptr(), raw.data_ptr(), ip, _s())
    elif gate is not None:
        word = None if gate[0] is None else gate[0].data_ptr()
        if entry == "img":
            rc = lib.uavenv_dqn_reduce_adam_img(nb, xd.data_ptr(), n, *a, loss.data_ptr(), raw.data_ptr(), word, gate[1], ip, _s())
        else:
            rc = lib.uavenv_dqn_reduce_adam_gated(nb, xd.data_ptr(), n, *a, loss.data_ptr(), raw.data_ptr(), word, gate[1], _s())
    elif img is None:
        rc = lib.uavenv_dqn_reduce_adam(nb, xd.data_ptr(), n, *a, loss.data_ptr(), raw.data_ptr(), _s())
    else:
        rc = lib.uavenv_dqn_reduce_adam_img(nb, xd.data_ptr(), n, *a, loss.data_ptr(), raw.data_ptr(), None, 0, ip, _s())
    torch.cuda.synchronize()
    r = raw.cpu().numpy()
    assert np.all(r[P + 2:] == np.float32(CANARY))
    return N.state(), loss.cpu().numpy()[0], r[:P + 2].copy(), rc


def check_forms(key, n, x, xd, exact, bound, cases=((5, True), (4, False))):
    """(c) for one set of partial rows: every form, both steps."""
    N = net(key)
    P = N.P
    cnt = float(exact[P + 1])
    div = max(cnt, 1.0)
    gbar = exact[:P] / div
    gerr = bound[:P] / div + 2.0 ** -23 * np.abs(gbar)
    m0, v0 = moments(gbar, P)
    w0, t0 = N.w_init, N.w_init + np.float32(1.0)
    h = p2p_open(P + 2)
    try:
        for t, hard in cases:
            for form in ("split", "p2p", "fused"):
                N.set_state(w0, t0, m0, v0)
                f, loss, raw, rc = run_form(N, form, xd, n, t, hard, h=h)
                assert rc == 0, (form, rc)
                assert not np.isnan(f).any() and not np.isnan(raw).any()
                # each form's own bucket within the summation bound; count exact
                rr = float((np.abs(raw[:P + 1].astype(np.float64) - exact[:P + 1]) / (bound[:P + 1] + 1e-300)).max())
                assert rr <= 1.0 and raw[P + 1] == cnt, (form, rr)
                want = np.float32(raw[P]) * (np.float32(1.0) / np.float32(div))
                assert bits(loss) == bits(want), (form, loss, want)
                f64 = f.astype(np.float64)
                ok, worst = check_adam(f64, w0.astype(np.float64), m0, v0, gbar, gerr, t, LR, BETAS, EPS, hard)
                record("adam/" + form, worst)
                assert ok, (form, t, worst)
                for alt in (div - 1.0, div + 1.0):         # a divide by count +- 1 is rejected (count 0 and 1 divide by 1: only + 1)
                    if alt >= 1.0:
                        assert not check_adam(f64, w0.astype(np.float64), m0, v0, exact[:P] / alt, gerr, t, LR, BETAS, EPS, hard)[0], (form, alt)
                check_target(N, t0, hard)
        print(key, n, "count", cnt, "adam worst ratios", {k: round(v, 4) for k, v in WORST.items() if k.startswith("adam/")})
    finally:
        N.lib.uavenv_p2p_destroy(h)


@pytest.mark.parametrize("key,n", CASES)
def test_c_three_adam_forms_against_f64(key, n):
    d = case(key, n)
    check_forms(key, n, d["x"], d["dev"], d["exact"], d["bound"])


@pytest.mark.parametrize("total", [0, 1])
def test_c_count_edges(total):
    """A total count of 0 divides by 1 (max(count, 1)); a total count of 1."""
    N, n = net("plain3"), 33
    x = partials(0, n, N.P, N.stride, call=9).copy()
    x[:, N.P + 1] = 0.0
    if total:
        x[17, N.P + 1] = 1.0
    exact = x[:, :N.P + 2].astype(np.float64).sum(axis=0)
    assert exact[N.P + 1] == total
    check_forms("plain3", n, x, dev(x), exact, column_sum_bound(x[:, :N.P + 2], reduce_depth(n)), cases=((5, True),))


@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("key", list(NETS))
def test_d_image_follows_the_parameters(key, hard):
    N, n = net(key), 257
    d = case(key, n)
    P, F = N.P, _L().DQN_IMAGE_FLOATS
    gbar = d["exact"][:P] / max(d["exact"][P + 1], 1.0)
    m0, v0 = moments(gbar, P)
    w0, t0 = N.w_init, N.w_init + np.float32(1.0)
    t = 5 if hard else 4
    h = p2p_open(P + 2)
    try:
        for form in ("split", "p2p", "fused"):
            N.set_state(w0, t0, m0, v0)
            f_null, loss_null, _, rc = run_form(N, form, d["dev"], n, t, hard, h=h)
            assert rc == 0
            N.set_state(w0, t0, m0, v0)
            img = N.image()
            before = img.cpu().numpy()
            f_img, loss_img, _, rc = run_form(N, form, d["dev"], n, t, hard, h=h, img=img)
            assert rc == 0
            assert same(f_img, f_null) and bits(loss_img) == bits(loss_null), form
            got, want = img.cpu().numpy(), N.image().cpu().numpy()
            assert not same(got[:F], before[:F]), "the step did not move layer 1"
            assert same(got[:F], want[:F]), (form, "local half", int(np.sum(bits(got[:F]) != bits(want[:F]))))
            if hard:
                assert same(got[F:], want[F:]), (form, "target half", int(np.sum(bits(got[F:]) != bits(want[F:]))))
                assert not same(got[F:], before[F:])
            else:
                assert same(got[F:], before[F:]), (form, "target half touched without a hard update")
    finally:
        N.lib.uavenv_p2p_destroy(h)


def test_e_gated_update():
    N, n, t, hard = net("plain3"), 257, 5, True
    d = case("plain3", n)
    P = N.P
    gbar = d["exact"][:P] / max(d["exact"][P + 1], 1.0)
    m0, v0 = moments(gbar, P)
    w0, t0 = N.w_init, N.w_init + np.float32(1.0)
    word = torch.tensor([7], dtype=torch.int32, device="cuda")
    N.set_state(w0, t0, m0, v0)
    start = N.state()
    want = run_form(N, "fused", d["dev"], n, t, hard)
    assert want[3] == 0 and not same(want[0], start)
    for entry in ("gated", "img"):
        N.set_state(w0, t0, m0, v0)
        img = N.image() if entry == "img" else None
        img0 = None if img is None else img.cpu().numpy()
        f, loss, raw, rc = run_form(N, "fused", d["dev"], n, t, hard, img=img, gate=(word, 8), entry=entry)     # 7 != 8: closed
        assert rc == 0 and same(f, start), entry
        assert loss == np.float32(CANARY) and np.all(raw == np.float32(CANARY)), entry
        if img is not None:
            assert same(img.cpu().numpy(), img0)
        for gate in ((word, 7), (None, 123)):                                                                    # open; no word
            N.set_state(w0, t0, m0, v0)
            img = N.image() if entry == "img" else None
            f, loss, raw, rc = run_form(N, "fused", d["dev"], n, t, hard, img=img, gate=gate, entry=entry)
            assert rc == 0 and same(f, want[0]) and bits(loss) == bits(want[1]) and same(raw, want[2]), (entry, gate[1])


# ---- (f) -------------------------------------------------------------------------------------------------------------------
def test_f_sticky_error_word_freezes_the_rank():
    L = _L()
    N, n = net("plain3"), 33
    lib, P = N.lib, N.P
    d0, d1 = case("plain3", n, 0), case("plain3", n, 1)
    gbar = d1["exact"][:P] / max(d1["exact"][P + 1], 1.0)
    m0, v0 = moments(gbar, P)
    h = p2p_open(P + 2)
    try:
        assert lib.uavenv_dqn_reduce_p2p(C.byref(N.net), d0["dev"].data_ptr(), n, h, _s()) == 0
        rc, o = pull_raw(N, h)
        assert rc == 0 and same(o, d0["raw"])
        assert lib.uavenv_p2p_inject_fault(h, L.P2P_ERR_DIVERGED) == 0
        assert lib.uavenv_dqn_reduce_p2p(C.byref(N.net), d1["dev"].data_ptr(), n, h, _s()) == L.EP2P
        N.set_state(N.w_init, N.w_init + np.float32(1.0), m0, v0)
        start, img = N.state(), N.image()
        img0 = img.cpu().numpy()
        loss = torch.full((1,), CANARY, device="cuda")
        raw = torch.full((P + 2,), CANARY, device="cuda")
        rc = lib.uavenv_dqn_adam_p2p_img(C.byref(N.net), h, LR, BETAS[0], BETAS[1], EPS, 5, 1, loss.data_ptr(), raw.data_ptr(),
                                         img.data_ptr(), _s())
        assert rc == L.EP2P
        after = N.state()
        assert same(after, start), ("a frozen rank stepped", int(np.sum(bits(after) != bits(start))))
        assert same(img.cpu().numpy(), img0) and float(loss[0]) == CANARY
        # nothing was enqueued by the refused push: the slot the pull reports is still call 0's
        assert same(raw.cpu().numpy(), d0["raw"])
        assert p2p_status(lib, h)["code"] == L.P2P_ERR_DIVERGED
    finally:
        lib.uavenv_p2p_destroy(h)


# ---- (g) -------------------------------------------------------------------------------------------------------------------
def allreduce_call(lib, h, mine, n):
    """-> (rc, the n floats after the call); 64 canaries behind them must survive."""
    buf = dev(np.concatenate([mine, np.full(64, CANARY, dtype=np.float32)]))
    rc = lib.uavenv_p2p_allreduce(h, buf.data_ptr(), n, _s())
    torch.cuda.synchronize()
    o = buf.cpu().numpy()
    assert np.all(o[n:] == np.float32(CANARY)), "uavenv_p2p_allreduce wrote behind count"
    return rc, o[:n].copy()


def test_g_allreduce_at_world_1_is_the_identity():
    L = _L()
    lib, h = L.load(), p2p_open(AR_BUCKET)
    try:
        for k, n in enumerate(COUNTS + (AR_PAD,)):
            x = payload(0, 100 + k, n)
            rc, o = allreduce_call(lib, h, x, n)
            assert rc == 0 and same(o, x), (n, int(np.sum(bits(o) != bits(x))))
        buf = dev(payload(0, 0, AR_PAD + 64))
        for count, off in ((1022, 0), (AR_PAD + 4, 0), (1024, 4), (0, 0)):          # count % 4, too large, misaligned, empty
            assert lib.uavenv_p2p_allreduce(h, buf.data_ptr() + off, count, _s()) == L.EINVAL, (count, off)
        st = p2p_status(lib, h)
        assert st["code"] == 0 and st["timeouts"] == 0
    finally:
        lib.uavenv_p2p_destroy(h)


def test_g_parity_slots_are_two():
    """A rank may be one update ahead of a peer: what it pushes at sequence k + 1 must not land on what the peer still reads at k.
    Sequence 1 and 2 fill both slots (X, Y); sequence 3 writes four floats (Z); a DQN pull at sequence 3 reads P + 2 floats of that
    slot: Z, then what sequence 1 left -- X, not Y."""
    N = net("plain3")
    lib, P, n = N.lib, N.P, 8192
    X, Y, Z = payload(0, 1, n), payload(0, 2, n), payload(0, 3, 4)
    h = p2p_open(AR_BUCKET)
    try:
        for x in (X, Y, Z):
            rc, o = allreduce_call(lib, h, x, len(x))
            assert rc == 0 and same(o, x)
        rc, o = pull_raw(N, h)
        assert rc == 0 and same(o[:4], Z)
        assert same(o[4:], X[4:P + 2]), "sequence 3 does not read the slot sequence 1 wrote"
    finally:
        lib.uavenv_p2p_destroy(h)


# ---- part B: several ranks on one GPU ---------------------------------------------------------------------------------------
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def rank_data(N, world, call):
    """Every rank's partial rows of exchange `call`, their buckets (uavenv_dqn_reduce, here) and f64 sums: every rank computes all."""
    hi = min(64, MAX_COUNT // sum(ROWS[:world]))
    xs = [partials(r, ROWS[r], N.P, N.stride, call=call, count_hi=hi) for r in range(world)]
    devs = [dev(x) for x in xs]
    return xs, devs, [reduce_bucket(N, devs[r], ROWS[r]) for r in range(world)]


def sha(x):
    return hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()


def _worker(rank, world, port, out_dir):
    import datetime
    import torch.distributed as dist
    from dqn_based_uav_3d_path_planer_amd import exchange
    L = _L()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
    torch.cuda.set_device(0)
    lib, device = L.load(), torch.device("cuda:0")
    N = Net("plain3")
    P = N.P
    res = {"fails": [], "worst": {}, "hash": {}}

    def chk(name, cond, info=""):
        if not cond:
            res["fails"].append(f"{name}: {info}")
        return bool(cond)

    def scenario(name, bucket, body, check_every=0):
        """A fresh handle per scenario (spin_limit 0 = the library's bounded wait): a sticky error ends the scenario, not the process."""
        h = exchange.open_p2p(lib, device, bucket, check_every=check_every, spin_limit=0)
        if not chk(name, h is not None, "open_p2p failed"):
            return
        try:
            body(h, name)
        except Exception as e:                               # noqa: BLE001 -- recorded; every rank still meets at the barrier
            res["fails"].append(f"{name}: {type(e).__name__}: {e}")
        torch.cuda.synchronize()
        dist.barrier()
        lib.uavenv_p2p_destroy(h)

    def healthy(h, name):
        st = p2p_status(lib, h)
        return chk(name, st["code"] == 0 and st["timeouts"] == 0 and st["mismatches"] == 0, f"status {st}")

    # (h)
    def body_h(h, name):
        for k, n in enumerate(COUNTS + (AR_PAD,)):
            for call in range(4):
                xs = [payload(r, 1000 * k + call, n) for r in range(world)]
                rc, o = allreduce_call(lib, h, xs[rank], n)
                want = rank_order_sum_f32(xs)
                chk(name, rc == 0 and same(o, want), f"count {n} call {call}: rc {rc}, {int(np.sum(bits(o) != bits(want)))} elements differ")
        healthy(h, name)
    scenario("h", AR_BUCKET, body_h)

    # (i)
    cache = {}

    def body_i(h, name):
        for call in range(4):
            xs, devs, buckets = rank_data(N, world, call)
            if call == 0:
                cache["d"] = (xs, devs, buckets)
            want = rank_order_sum_f32(buckets)
            rc1 = lib.uavenv_dqn_reduce_p2p(C.byref(N.net), devs[rank].data_ptr(), ROWS[rank], h, _s())
            rc2, o = pull_raw(N, h)
            chk(name, rc1 == 0 and rc2 == 0 and same(o, want),
                f"call {call}: rc {rc1} {rc2}, {int(np.sum(bits(o) != bits(want)))} elements differ, count {o[P + 1]} / {want[P + 1]}")
        healthy(h, name)
    scenario("i", P + 2, body_i)

    # (j)
    def body_j(h, name):
        xs, devs, buckets = cache["d"] if "d" in cache else rank_data(N, world, 0)
        cols = [x[:, :P + 2].astype(np.float64).sum(axis=0) for x in xs]
        exact = np.sum(cols, axis=0)
        bounds = [column_sum_bound(x[:, :P + 2], reduce_depth(ROWS[r])) for r, x in enumerate(xs)]
        # the bucket: every rank's own f32 column sums (their bound), then world - 1 f32 additions of the buckets, each rounding a
        # partial sum of magnitude at most sum_r |bucket_r| (|bucket_r| <= |col_r| + bound_r)
        sum_bound = np.sum(bounds, axis=0) + (world - 1) * 2.0 ** -24 * np.sum([np.abs(c) + b for c, b in zip(cols, bounds)], axis=0)
        cnt = float(exact[P + 1])
        chk(name, 2 <= cnt <= MAX_COUNT, f"count {cnt}")
        gbar = exact[:P] / cnt
        gerr = sum_bound[:P] / cnt + 2.0 ** -23 * np.abs(gbar)
        m0, v0 = moments(gbar, P)
        w0, t0 = N.w_init, N.w_init + np.float32(1.0)
        N.set_state(w0, t0, m0, v0)
        img = N.image()
        f, loss, raw, rc = run_form(N, "p2p", devs[rank], ROWS[rank], 5, True, h=h, img=img)
        chk(name, rc == 0, f"rc {rc}")
        chk(name, same(raw, rank_order_sum_f32(buckets)), "raw_out is not the rank-order sum")
        chk(name, bits(loss) == bits(np.float32(raw[P]) * (np.float32(1.0) / np.float32(cnt))), f"loss {loss}")
        f64, w64 = f.astype(np.float64), w0.astype(np.float64)
        ok, worst = check_adam(f64, w64, m0, v0, gbar, gerr, 5, LR, BETAS, EPS, True)
        res["worst"]["k_p2p_pull_adam"] = worst
        chk(name, ok, f"check_adam worst ratio {worst}")
        wrong = {"count - 1": exact[:P] / (cnt - 1), "count + 1": exact[:P] / (cnt + 1)}
        for r in range(world):
            own = float(cols[r][P + 1])
            if own >= 1 and own != cnt:
                wrong[f"rank {r}'s own count"] = exact[:P] / own
            wrong[f"rank {r} dropped"] = (exact - cols[r])[:P] / cnt
            wrong[f"rank {r} doubled"] = (exact + cols[r])[:P] / cnt
        for what, g in wrong.items():
            chk(name, not check_adam(f64, w64, m0, v0, g, gerr, 5, LR, BETAS, EPS, True)[0], f"not rejected: {what}")
        chk(name, same(f[1], f[0]), "hard update: target != local")
        got, want = img.cpu().numpy(), N.image().cpu().numpy()
        chk(name, same(got, want), f"image: {int(np.sum(bits(got) != bits(want)))} floats differ from the split form of the stepped net")
        res["hash"]["j_state"], res["hash"]["j_image"] = sha(f), sha(got)
        healthy(h, name)
    scenario("j", P + 2, body_j)

    # (k): two parameters whose gradient columns are equal on every rank, from zero moments: both take the SAME step, so swapping their
    # values on one rank leaves the multiset of the stepped weights' bit patterns as it was -- only position tells
    p1, p2 = 10, 4001

    def k_rows(step):
        x = partials(rank, ROWS[rank], P, N.stride, call=20 + step, count_hi=min(64, MAX_COUNT // sum(ROWS[:world]))).copy()
        x[:, p2] = x[:, p1]
        return dev(x)

    def k_reset():
        w = N.w_init.copy()
        w[P - 1] = 0.75               # a step of ~1e-3 keeps it inside [0.5, 1): one ulp stays one ulp
        assert w[p1] != w[p2]
        N.set_state(w, w, np.zeros(P), np.zeros(P))

    def k_step(h, t):
        rc1 = lib.uavenv_dqn_reduce_p2p(C.byref(N.net), k_rows(t).data_ptr(), ROWS[rank], h, _s())
        rc2 = rc1
        if rc1 == 0:
            rc2 = lib.uavenv_dqn_adam_p2p(C.byref(N.net), h, LR, BETAS[0], BETAS[1], EPS, t, 0, None, None, _s())
        torch.cuda.synchronize()
        return rc1, rc2

    def body_k_healthy(h, name):
        k_reset()
        for t in (1, 2, 3):
            rc = k_step(h, t)
            chk(name, rc == (0, 0), f"step {t}: rc {rc}")
        st = p2p_status(lib, h)
        chk(name, st["code"] == 0 and st["mismatches"] == 0 and st["timeouts"] == 0 and st["checks"] >= 2, f"status {st}")
        res["hash"]["k_weights"] = sha(N.state()[0])
        chk(name, not same(N.state()[0][[p1, p2, P - 1]], np.float32([N.w_init[p1], N.w_init[p2], 0.75])), "no step was taken")
    scenario("k_healthy", P + 2, body_k_healthy, check_every=1)

    def perturbed(perturb):
        def body(h, name):
            k_reset()
            chk(name, k_step(h, 1) == (0, 0), "step 1")
            perturb()
            torch.cuda.synchronize()
            dist.barrier()
            frozen_at = None
            for t in (2, 3):                      # within two further steps
                before = N.state()
                k_step(h, t)
                st = p2p_status(lib, h)
                if st["code"] != 0:
                    chk(name, same(N.state(), before), f"step {t}: DIVERGED was raised and the weights or moments moved")
                    frozen_at = frozen_at or t
            st = p2p_status(lib, h)
            chk(name, st["code"] == L.P2P_ERR_DIVERGED and st["mismatches"] >= 1 and st["timeouts"] == 0, f"status {st}")
            chk(name, frozen_at is not None, "never frozen")
            w = N.state()[0].copy()
            rc = lib.uavenv_dqn_reduce_p2p(C.byref(N.net), k_rows(4).data_ptr(), ROWS[rank], h, _s())
            chk(name, rc == L.EP2P and same(N.state()[0], w), f"after DIVERGED: rc {rc}")
        return body

    def flip():
        if rank == world - 1:
            N.flat[0].view(torch.int32)[P - 1] ^= 1

    def swap():
        if rank == 0:
            a, b = N.flat[0][p1].clone(), N.flat[0][p2].clone()
            N.flat[0][p1], N.flat[0][p2] = b, a
    scenario("k_flip", P + 2, perturbed(flip), check_every=1)
    scenario("k_swap", P + 2, perturbed(swap), check_every=1)

    # (l)
    lens = (5, 1000, 4097)

    def blocks_case(perturb):
        def body(h, name):
            blocks = [payload(0, 50 + b, n).copy() for b, n in enumerate(lens)]
            if perturb is not None:
                perturb(blocks)
            bd = [dev(b) for b in blocks]
            ptrs = (C.c_void_p * 3)(*[b.data_ptr() for b in bd])
            nf = (C.c_int32 * 3)(*lens)
            rc = lib.uavenv_p2p_check_blocks(h, ptrs, nf, 3, _s())
            torch.cuda.synchronize()
            st = p2p_status(lib, h)
            if perturb is None:
                chk(name, rc == 0 and st["code"] == 0 and st["mismatches"] == 0 and st["checks"] == 1, f"rc {rc} status {st}")
            else:
                chk(name, st["code"] == L.P2P_ERR_DIVERGED and st["mismatches"] >= 1 and st["timeouts"] == 0, f"rc {rc} status {st}")
                ptr1 = (C.c_void_p * 1)(bd[0].data_ptr())
                chk(name, lib.uavenv_p2p_check_blocks(h, ptr1, (C.c_int32 * 1)(5), 1, _s()) == L.EP2P, "not sticky")
        return body

    def ulp(blocks):
        if rank == world - 1:
            blocks[2].view(np.uint32)[-1] ^= 1

    def swap_across(blocks):                      # same index in blocks 0 and 2: only the block number tells
        if rank == 0:
            assert blocks[0][3] != blocks[2][3]
            blocks[0][3], blocks[2][3] = blocks[2][3], blocks[0][3]

    def swap_inside(blocks):                      # two indices of block 2 (the second on a later grid-stride trip): only the index tells
        if rank == 0:
            assert blocks[2][7] != blocks[2][3000]
            blocks[2][7], blocks[2][3000] = blocks[2][3000], blocks[2][7]
    scenario("l_same", 64, blocks_case(None))
    scenario("l_ulp", 64, blocks_case(ulp))
    scenario("l_swap_across", 64, blocks_case(swap_across))
    scenario("l_swap_inside", 64, blocks_case(swap_inside))

    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as fh:
        json.dump(res, fh)
    dist.barrier()
    dist.destroy_process_group()


_RUNS = {}


def ranks_of(world, tmp_path_factory):
    """One spawn per world: `world` fresh child processes (with this one: at most four on the device) run every scenario."""
    if world not in _RUNS:
        import torch.multiprocessing as mp
        out = tmp_path_factory.mktemp(f"world{world}")
        try:
            if "dead" in _RUNS:                                  # ranks of another world died: start no more on this device
                raise _RUNS["dead"]
            torch.cuda.synchronize()                             # (raises if an earlier launch of this process faulted)
            mp.spawn(_worker, args=(world, _port(), str(out)), nprocs=world, join=True)
            _RUNS[world] = [json.load(open(os.path.join(out, f"r{r}.json"))) for r in range(world)]
        except Exception as e:                                   # noqa: BLE001 -- run once: every test of this world reports it
            _RUNS[world] = _RUNS["dead"] = e
    if isinstance(_RUNS[world], Exception):
        raise _RUNS[world]
    return _RUNS[world]


def scenario_fails(rs, prefix):
    return [f"rank {r}: {f}" for r, d in enumerate(rs) for f in d["fails"] if f.startswith(prefix)]


@pytest.mark.parametrize("world", [2, 3])
def test_h_allreduce_is_the_rank_order_sum(world, tmp_path_factory):
    assert scenario_fails(ranks_of(world, tmp_path_factory), "h:") == []


@pytest.mark.parametrize("world", [2, 3])
def test_i_dqn_bucket_is_the_rank_order_sum_of_the_rank_buckets(world, tmp_path_factory):
    assert scenario_fails(ranks_of(world, tmp_path_factory), "i:") == []


@pytest.mark.parametrize("world", [2, 3])
def test_j_real_step_against_f64(world, tmp_path_factory):
    rs = ranks_of(world, tmp_path_factory)
    assert scenario_fails(rs, "j:") == []
    for d in rs:
        record(f"k_p2p_pull_adam/world{world}", d["worst"]["k_p2p_pull_adam"])
    print("world", world, "k_p2p_pull_adam worst ratio", [round(d["worst"]["k_p2p_pull_adam"], 4) for d in rs])
    assert len({d["hash"]["j_state"] for d in rs}) == 1 and len({d["hash"]["j_image"] for d in rs}) == 1     # ranks bit-identical


@pytest.mark.parametrize("world", [2, 3])
def test_k_checksum_sees_one_bit_and_position(world, tmp_path_factory):
    rs = ranks_of(world, tmp_path_factory)
    assert scenario_fails(rs, "k_") == []
    assert len({d["hash"]["k_weights"] for d in rs}) == 1


@pytest.mark.parametrize("world", [2, 3])
def test_l_check_blocks_sees_one_bit_block_and_position(world, tmp_path_factory):
    assert scenario_fails(ranks_of(world, tmp_path_factory), "l_") == []
