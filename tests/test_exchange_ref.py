"""oracle/exchange_ref.py on the CPU: the helpers the GPU tests of the exchange kernels lean on (tests/test_exchange_kernels_gpu.py),
and the resolving power of the generated inputs -- a test that asks for a bit-identical rank-order sum says nothing unless another
order, a dropped rank or a doubled one would actually change the bits."""
import numpy as np
import pytest

from oracle.exchange_ref import (column_sum_bound, gamma, pairwise_sum_f32, partials, payload, rank_order_sum_f32, reduce_depth,
                                 sequential_sum_f32)

N = 8192


def test_payload_is_reproducible_and_distinct():
    a = payload(1, 2, N)
    assert a.dtype == np.float32 and a.shape == (N,) and np.array_equal(a, payload(1, 2, N))
    assert not np.array_equal(a, payload(2, 2, N)) and not np.array_equal(a, payload(1, 3, N))
    assert np.isfinite(a).all() and not np.any(a == 0.0)          # (no -0.0: 0 + x would turn it positive)
    e = np.floor(np.log2(np.abs(a)))
    assert e.min() < -12 and e.max() > 10                         # mixed magnitudes: the addition order matters


def test_partials_layout():
    P, stride = 6659, 6688
    x = partials(2, 257, P, stride, call=1, count_hi=19)
    assert x.shape == (257, stride) and x.dtype == np.float32
    assert np.isfinite(x[:, :P + 2]).all() and np.isnan(x[:, P + 2:]).all()
    assert (x[:, P] >= 0).all()
    c = x[:, P + 1]
    assert np.array_equal(c, np.round(c)) and c.min() >= 0 and c.max() <= 19 and c.max() > 10
    assert partials(0, 600, P, stride)[:, P + 1].max() <= 64
    assert not np.array_equal(x[:, :P], partials(2, 257, P, stride, call=2, count_hi=19)[:, :P])


def test_rank_order_sum_is_left_to_right_f32():
    xs = [np.float32([2.0 ** 24]), np.float32([1.0]), np.float32([1.0])]
    assert rank_order_sum_f32(xs)[0] == np.float32(2.0 ** 24)                 # (2^24 + 1) + 1: both ones are rounded away
    assert rank_order_sum_f32(xs[::-1])[0] == np.float32(2.0 ** 24 + 2.0)     # (1 + 1) + 2^24
    assert rank_order_sum_f32(xs).dtype == np.float32


def test_reduce_depth():
    assert [reduce_depth(n) for n in (1, 255, 256, 257, 512, 600)] == [18, 18, 18, 26, 26, 34]
    assert gamma(18) == pytest.approx(18 * 2.0 ** -24, rel=1e-5) and gamma(18) > 18 * 2.0 ** -24


@pytest.mark.parametrize("n", [1, 33, 257, 600])
def test_column_sum_bound_holds_for_sequential_and_pairwise_f32(n):
    """The bound is about the longest chain of additions, whatever the association: a sequential sum of n rows has n - 1 roundings
    in its chain (0 + x is exact), a pairwise one ceil(log2 n).  Both against the f64 sums of the generated columns -- and the
    pairwise bound, a few u, is tight enough that the sequential sum of 600 rows breaks it somewhere (it is not a bound one can
    apply without reading the kernel's order)."""
    P, stride = 2000, 2016
    x = partials(0, n, P, stride)[:, :P + 1]
    exact = x.astype(np.float64).sum(axis=0)
    seq = np.abs(sequential_sum_f32(x).astype(np.float64) - exact)
    pw = np.abs(pairwise_sum_f32(x).astype(np.float64) - exact)
    assert np.all(seq <= column_sum_bound(x, max(n - 1, 1)))
    d_pw = max(int(np.ceil(np.log2(n))), 1)
    assert np.all(pw <= column_sum_bound(x, d_pw))
    # the f32 result also has to be rounded once more than f64's own error: irrelevant at 2^-53
    if n == 600:
        assert np.any(seq > column_sum_bound(x, 1)) and np.all(seq <= column_sum_bound(x, n - 1))


@pytest.mark.parametrize("world,least", [(3, 0.10), (5, 0.10)])
def test_reverse_order_shows_in_the_bits(world, least):
    """World 3: about 22 % of the elements differ between ((x0 + x1) + x2) and ((x2 + x1) + x0); world 5: about 42 %.  World 2:
    f32 addition commutes, x0 + x1 == x1 + x0 bit for bit, so ORDER is not resolvable there -- world 3 is the smallest that sees it."""
    xs = [payload(r, 0, N) for r in range(world)]
    fwd, rev = rank_order_sum_f32(xs), rank_order_sum_f32(xs[::-1])
    frac = float(np.mean(fwd.view(np.uint32) != rev.view(np.uint32)))
    print("world", world, "reverse order differs in", round(frac, 3))
    assert frac >= least
    two = [payload(r, 0, N) for r in range(2)]
    assert np.array_equal(rank_order_sum_f32(two).view(np.uint32), rank_order_sum_f32(two[::-1]).view(np.uint32))


@pytest.mark.parametrize("world", [2, 3])
def test_a_dropped_or_doubled_rank_shows_almost_everywhere(world):
    xs = [payload(r, 1, N) for r in range(world)]
    full = rank_order_sum_f32(xs).view(np.uint32)
    drop = float(np.mean(full != rank_order_sum_f32(xs[:-1]).view(np.uint32)))
    dbl = float(np.mean(full != rank_order_sum_f32(xs + [xs[-1]]).view(np.uint32)))
    first = float(np.mean(full != rank_order_sum_f32(xs[1:]).view(np.uint32)))
    print("world", world, "dropped last / doubled last / dropped first:", round(drop, 3), round(dbl, 3), round(first, 3))
    assert drop > 0.95 and dbl > 0.95 and first > 0.95


def test_partial_buckets_resolve_rank_order_too():
    """The DQN bucket of the multi-rank test: per-rank column sums of 1, 257 and 600 rows, then added in rank order."""
    P, stride = 6659, 6688
    b = [sequential_sum_f32(partials(r, n, P, stride)[:, :P + 2]) for r, n in enumerate((1, 257, 600))]
    fwd, rev = rank_order_sum_f32(b), rank_order_sum_f32(b[::-1])
    frac = float(np.mean(fwd[:P].view(np.uint32) != rev[:P].view(np.uint32)))
    print("bucket: reverse order differs in", round(frac, 3))
    assert frac >= 0.10
