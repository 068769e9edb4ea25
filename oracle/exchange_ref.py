"""Inputs and bounds for the tests of the multi-GPU update kernels (csrc/p2p.hip, k_dqn_reduce / k_dqn_adam of csrc/learner.hip):
numpy only, so that every rank of a test regenerates every rank's data from seeds all of them know -- the expected sums need no
second transport -- and the CPU suite can check the generators' resolving power (tests/test_exchange_ref.py).

The values are standard normals scaled by 2^e, e uniform in [-12, 12]: neighbouring addends differ by up to seven decimal
orders, so the ORDER of an f32 summation shows in its bits (a reverse-order sum of three ranks differs from the rank-order sum
in about a fifth of the elements), and a dropped or doubled addend shows almost everywhere."""
from __future__ import annotations

import numpy as np

TAG_PAYLOAD = 0x9E3C
TAG_PARTIALS = 0x51D7
U = 2.0 ** -24                       # unit roundoff of f32, round to nearest


def _mixed(rng, shape):
    x = rng.standard_normal(shape) * np.exp2(rng.integers(-12, 13, shape))
    x = x.astype(np.float32)
    x[x == 0.0] = np.float32(1.0)    # (no zero of either sign: 0 + x turns -0.0 positive)
    return x


def payload(rank: int, call: int, n: int) -> np.ndarray:
    """What rank `rank` sends in exchange number `call`: n floats."""
    return _mixed(np.random.default_rng([TAG_PAYLOAD, int(rank), int(call)]), int(n))


def partials(rank: int, n_partials: int, P: int, stride: int, call: int = 0, count_hi: int = 64) -> np.ndarray:
    """Partial rows as the gradient kernels leave them for the reductions, [n_partials, stride] f32: columns [0, P) gradient
    shares, column P a non-negative loss share, column P + 1 an integer-valued valid count in [0, count_hi] (count_hi <= 64, one
    tile), columns [P + 2, stride) NaN -- pad that no kernel may let reach an output."""
    assert 0 <= count_hi <= 64 and stride >= P + 2
    rng = np.random.default_rng([TAG_PARTIALS, int(rank), int(call), int(n_partials)])
    x = np.full((int(n_partials), int(stride)), np.nan, dtype=np.float32)
    x[:, :P] = _mixed(rng, (n_partials, P))
    x[:, P] = np.abs(_mixed(rng, n_partials))
    x[:, P + 1] = rng.integers(0, count_hi + 1, n_partials).astype(np.float32)
    return x


def rank_order_sum_f32(xs) -> np.ndarray:
    """((x0 + x1) + x2) + ... in f32: the order in which k_p2p_pull_sum and k_p2p_pull_adam add the ranks' slots."""
    acc = np.asarray(xs[0], dtype=np.float32).copy()
    for x in xs[1:]:
        acc = (acc + np.asarray(x, dtype=np.float32)).astype(np.float32)
    return acc


def gamma(k: int) -> float:
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of k chained f32 additions."""
    return k * U / (1.0 - k * U)


def column_sum_bound(x, depth: int) -> np.ndarray:
    """|fl(sum_b x_bp) - sum_b x_bp| <= gamma_depth * sum_b |x_bp| for ANY f32 summation of a column whose longest chain of
    additions is `depth` long (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)."""
    return gamma(int(depth)) * np.abs(np.asarray(x, dtype=np.float64)).sum(axis=0)


def reduce_depth(n_partials: int) -> int:
    """The longest addition chain of reduce_columns (csrc/learner.hip) and its copy in k_p2p_reduce_push (csrc/p2p.hip): a thread
    adds 8 rows per 256-row trip into its accumulator (8 ceil(n / 256)), four row groups are added pairwise (2 levels), and lane
    p adds the eight results one after another starting from zero (8)."""
    return 8 * ((int(n_partials) + 255) // 256) + 10


def sequential_sum_f32(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    acc = np.zeros(x.shape[1:], dtype=np.float32)
    for row in x:
        acc = (acc + row).astype(np.float32)
    return acc


def pairwise_sum_f32(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    while x.shape[0] > 1:
        if x.shape[0] & 1:
            x = np.concatenate([x, np.zeros((1,) + x.shape[1:], dtype=np.float32)])
        x = (x[0::2] + x[1::2]).astype(np.float32)
    return x[0]
