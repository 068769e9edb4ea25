"""CPU restatement of the reference's prioritised replay (BaseClass/replay_buffer.py:57-223).  TEST INFRASTRUCTURE:
only tests/ may import this; the product path is csrc/per.hip.  Pinned against tests/golden/per.npz, which
oracle/gen_golden_per.py makes by executing the reference (tests/test_oracle_golden.py::test_per_*).

What is restated, with the reference's quirks:
  * the sum tree is a flat array of 2c-1 nodes, leaf of data slot d at node c-1+d (:60-66, :84-90); priorities
    reach the inner nodes as propagated DIFFERENCES (:70-79), so an inner node is a history-dependent float sum;
  * the descent goes left when v <= tree[left] (:103-110); with a capacity that is not a power of two the leaves
    are therefore visited in a rotated slot order;
  * total() truncates the root to an int (:117-118) and that int is what segments and probabilities use (:147,:163);
  * priority on push: (|error| + 0.01) ** 0.6, no clip (:143-144); on batch_update: min(|error| + 0.01, 1) ** 0.6
    (:215-222); beta <- min(1, beta + 0.001) on every sample() (:155); weights (n_entries * p / total) ** -beta,
    divided by their maximum (:176-178).

Below the tree: the flat-array contract of include/uavenv.h (UavPer) in plain numpy -- ring_fill, batch_update_seq, is_weights,
exact_sums, decided -- for tests/test_per_frame_kernels_gpu.py; tests/test_per_ref.py pins them to the golden file and the tree.
"""
import math
from fractions import Fraction

import numpy as np


class PerOracle:
    def __init__(self, capacity, alpha=0.6, beta=0.4, beta_inc=0.001, epsilon=0.01, clip=1.0):
        self.c = int(capacity)
        self.node = np.zeros(2 * self.c - 1)          # :66
        self.ptr = 0
        self.n_entries = 0
        self.alpha, self.beta, self.beta_inc, self.epsilon, self.clip = alpha, beta, beta_inc, epsilon, clip

    # ---- SumTree.update / add (:68-97)
    def _set_leaf(self, node_idx, p):
        delta = p - self.node[node_idx]
        self.node[node_idx] = p
        k = node_idx
        while k != 0:
            k = (k - 1) // 2
            self.node[k] += delta

    def push(self, error):
        p = (abs(float(error)) + self.epsilon) ** self.alpha                 # :143
        slot = self.ptr
        self._set_leaf(slot + self.c - 1, p)
        self.ptr = (self.ptr + 1) % self.c
        self.n_entries = min(self.n_entries + 1, self.c)
        return slot

    def batch_update(self, slots, abs_errors):
        e = np.minimum(np.asarray(abs_errors, dtype=np.float64) + self.epsilon, self.clip)   # :216-218
        for s, p in zip(slots, np.power(e, self.alpha)):
            self._set_leaf(int(s) + self.c - 1, p)

    def priorities(self):
        return self.node[self.c - 1:].copy()

    def total_int(self):
        return int(self.node[0])                                             # :117-118

    # ---- SumTree.get_leaf (:99-115)
    def _descend(self, v):
        k = 0
        while 2 * k + 1 < len(self.node):
            left = 2 * k + 1
            if v <= self.node[left]:
                k = left
            else:
                v -= self.node[left]
                k = left + 1
        return k

    def segments(self, batch):
        seg = self.total_int() / batch                                       # :147
        return seg * np.arange(batch), seg * (np.arange(batch) + 1)

    def sample(self, batch, draws):
        """draws[i] is what random.uniform(seg*i, seg*(i+1)) returned.  -> (slots, priorities, weights)"""
        self.beta = min(1.0, self.beta + self.beta_inc)                      # :155
        leaves = np.array([self._descend(float(v)) for v in draws])
        p = self.node[leaves]
        prob = p / self.total_int()                                          # :175
        w = np.power(self.n_entries * prob, -self.beta)                      # :176
        w /= w.max()
        return leaves - (self.c - 1), p, w


def leaf_rotation(capacity):
    """In-order position q of the flat tree's leaves holds data slot (q + rot) % capacity."""
    depth = int(np.floor(np.log2(2 * capacity - 1)))
    return (1 << depth) - capacity


def sample_by_cumsum(prio, total_for_nothing, draws, rot=None):
    """The same selection without a tree: first in-order position whose inclusive cumulative priority reaches v
    (what csrc/per.hip does).  Agrees with the descent except when v falls within rounding of a boundary, and for a draw of
    exactly 0 in front of empty leaves: the descent ends on leaf 0 whatever it holds, the device on the first leaf with a
    positive priority (it never returns an empty leaf while one is filled).  rot: the in-order rotation (default: the flat
    tree's, leaf_rotation; 0 = DevicePER(tree_order=False))."""
    c = len(prio)
    rot = leaf_rotation(c) if rot is None else int(rot)
    order = (np.arange(c) + rot) % c
    cs = np.cumsum(prio[order])
    v = np.asarray(draws)
    q = np.where(v > 0, np.searchsorted(cs, v, side="left"), np.searchsorted(cs, 0.0, side="right"))
    return order[np.minimum(q, c - 1)]


# ---- the flat-array contract of include/uavenv.h (UavPer: "prioritised replay ... on the device"), restated from the header's
# ---- words and the reference alone -- the kernels these hold to account (csrc/per.hip) are not consulted.  Plain numpy.
CHUNK, GROUP = 1024, 16          # leaves per chunk / per group sum (include/uavenv.h: "sums of 16 consecutive in-order leaves")


def ring_fill(prio, first, count, value, valid, valid_stride, retire_first):
    """uavenv_per_fill_frame / _strided / _rebuild_frame: [retire_first, retire_first + count) <- 0, and [first, first + count)
    <- `value` where valid[i * valid_stride] != 0 (valid None: everywhere), 0 elsewhere.  Every other slot keeps its bits."""
    out = np.array(prio, dtype=np.float64, copy=True)
    first, count, retire_first = int(first), int(count), int(retire_first)
    if count <= 0:
        return out
    assert 0 <= first and first + count <= len(out) and 0 <= retire_first and retire_first + count <= len(out)
    out[retire_first:retire_first + count] = 0.0
    if valid is None:
        out[first:first + count] = value
    else:
        flags = np.asarray(valid).reshape(-1)[np.arange(count) * int(valid_stride)]
        out[first:first + count] = np.where(flags != 0, np.float64(value), 0.0)
    return out


def batch_update_seq(prio, slots, abs_err, epsilon, alpha, clip):
    """ReplayTree.batch_update (replay_buffer.py:215-222) as the sequential loop it is -- a slot listed several times ends with
    the LAST of its errors -- with the header's rules: slots outside [0, capacity) are ignored; clip > 0 leaves an empty leaf
    (priority 0) at 0; clip <= 0 means no clip: ReplayTree.push (:143), which also writes empty leaves."""
    out = np.array(prio, dtype=np.float64, copy=True)
    c = len(out)
    e = np.abs(np.asarray(abs_err, dtype=np.float64)) + epsilon
    if clip > 0.0:
        e = np.minimum(e, clip)                                              # :216-218
    for s, p in zip(np.asarray(slots).tolist(), np.power(e, alpha).tolist()):
        if s < 0 or s >= c:
            continue
        if clip > 0.0 and out[s] == 0.0:
            continue
        out[s] = p
    return out


def is_weights(p, n_entries, total, beta, normalise=True):
    """ReplayTree.sample's importance weights (:175-178): (n_entries * (p / max(int(total), 1))) ** -beta, divided by their
    maximum; a zero priority gets weight 0 (and an all-zero batch stays all zero).  normalise=False: before the division."""
    p = np.asarray(p, dtype=np.float64)
    t = max(math.floor(float(total)), 1)
    w = np.zeros_like(p)
    pos = p > 0.0
    w[pos] = np.power(np.float64(n_entries) * (p[pos] / np.float64(t)), -np.float64(beta))
    if not normalise:
        return w
    m = w.max() if len(w) else 0.0
    return w / m if m > 0.0 else w


def in_order(prio, rot):
    """The priorities in the order the tree visits its leaves: position q holds slot (q + rot) % c."""
    prio = np.asarray(prio, dtype=np.float64)
    return prio[(np.arange(len(prio)) + int(rot)) % len(prio)]


def exact_sums(prio, rot):
    """-> dict(group [n_chunks * 64], chunk [n_chunks], prefix [n_chunks + 1]): the correctly rounded sums of the in-order
    leaves -- math.fsum per 16-leaf group and per 1 024-leaf chunk (positions past the capacity count as 0); prefix[b] = the sum
    of every leaf in front of chunk b, prefix[n_chunks] the total.  The prefix is accumulated exactly (each chunk as its fsum
    plus the fsum of what that rounding left behind, added as rationals) and rounded once per entry, which is what math.fsum
    over all those leaves returns, without summing them n_chunks times over."""
    x = in_order(prio, rot)
    n_chunks = (len(x) + CHUNK - 1) // CHUNK
    pad = np.zeros(n_chunks * CHUNK)
    pad[:len(x)] = x
    leaves = pad.tolist()
    group = np.array([math.fsum(leaves[k:k + GROUP]) for k in range(0, len(leaves), GROUP)])
    chunk = np.empty(n_chunks)
    prefix = np.empty(n_chunks + 1)
    run = Fraction(0)
    for b in range(n_chunks):
        part = leaves[b * CHUNK:(b + 1) * CHUNK]
        hi = math.fsum(part)
        lo = math.fsum(part + [-hi])
        chunk[b] = hi
        prefix[b] = float(run)
        run += Fraction(hi) + Fraction(lo)
    prefix[n_chunks] = float(run)
    return dict(group=group, chunk=chunk, prefix=prefix)


def decided(prio, rot, draws, margin):
    """-> bool per draw: True when the draw lies further than `margin` from every leaf boundary (the inclusive cumulative
    priorities in in-order position, and 0), so that no summation order can move it into another leaf.  Boundaries in
    np.longdouble."""
    cs = np.concatenate([[np.longdouble(0.0)], np.cumsum(in_order(prio, rot).astype(np.longdouble))])
    v = np.asarray(draws, dtype=np.float64).astype(np.longdouble)
    k = np.clip(np.searchsorted(cs, v, side="left"), 1, len(cs) - 1)
    dist = np.minimum(np.abs(v - cs[k - 1]), np.abs(cs[k] - v))
    return np.asarray(dist > np.longdouble(margin))
