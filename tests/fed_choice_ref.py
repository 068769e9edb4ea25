"""Shared by tests/test_federated_choice.py (CPU) and tests/test_federated_choice_gpu.py: the selective federated merge
(Federated_Learning_choice, Envs/PathPlan_City.py:644-684; csrc/fed.hip: uavenv_fed_choice) restated on the host -- distances in
float64 (oracle.dqn_grad_ref.forward_f64) with the bar the GPU test holds the kernel's f32 distances to, the stable choice, the
f32 merge -- and the inputs both files use: a one-parameter family of nets and the case list.

The bar.  With e = q_p - q_j (float64, S x A) and beta = TAU_Q (q_abs_p + q_abs_j) -- TAU_Q q_abs is the project's forward bar of
tests/test_dqn_act_kernels_gpu.py, so |e_out - e| <= beta element by element -- the squared differences are off by at most
2 |e| beta + beta^2 each, and the mean of S x A <= 224 of them by their mean plus the rounding of at most 224 f32 squares and adds,
covered by 2^-16 d:   |d_out - d| <= mean(2 |e| beta + beta^2) + 2^-16 d.

The gap condition.  Sorted by float64 distance, every pair of neighbours among the chosen and across the selection boundary lies
more than 4 bars apart (the larger of the two bars): the kernel's own distances, each within one bar, then sort the same way, so
"chosen = stable sort of the kernel's distances" and "distances within the bar" pin the choice to float64."""
import numpy as np

from oracle.dqn_grad_ref import forward_f64, q_abs_f64, unflatten

W, HID = 100, 64
TAU_Q = 2.0 ** -16
U_ALL, S_ALL = (1, 2, 3, 5, 8), (1, 10, 16)
HEADS = [(3, False), (3, True), (9, True)]
CASES = [(U, S, A, d) for U in U_ALL for S in S_ALL for (A, d) in HEADS]
# the family's coordinates: no two differences |c_p - c_j| are close, before or after the merges (the gap condition checks)
C_FAMILY = (0.0, 27.58, 18.13, 9.02, 14.73, 12.19, 44.94, 39.2)


def n_params(A, dueling):
    n2 = A + (1 if dueling else 0)
    return HID * W + HID + n2 * HID + n2


def family(A, dueling, U, seed=5):
    """U flat f32 blocks base + c_j D.  A mean of members is (up to f32 rounding) a member again, and for small D the distance
    between two members grows with |c_p - c_j|: well-separated coordinates give well-separated distances at every step."""
    rng = np.random.default_rng(seed + 100 * A + int(dueling))
    P = n_params(A, dueling)
    base = (rng.normal(0, 1, P) * 0.15).astype(np.float32)
    D = (rng.normal(0, 1, P) * 0.1).astype(np.float32)
    return [(base + np.float32(C_FAMILY[j]) * D).astype(np.float32) for j in range(U)]


RING_FRAMES, RING_AGENTS = 3, 40


def episode_ring(ep_obs):
    """A [3, 40, 100] f32 ring of rows the reference's own state_PathPlan produced (tests/golden/episodes.npz: `obs`) -- known
    without a GPU, so the gap condition is asserted on exactly the rows the GPU cases read."""
    rng = np.random.default_rng(77)
    pick = rng.choice(len(ep_obs), RING_FRAMES * RING_AGENTS, replace=False)
    return np.ascontiguousarray(ep_obs[pick], dtype=np.float32).reshape(RING_FRAMES, RING_AGENTS, W)


def case_pairs(U, S, A, frames, n_agents):
    """int32 [U, S, 2] (frame, agent) pairs of a case; the corners of the ring are among them as far as U x S allows: frame 0,
    the last frame, agent 0 and agent n_agents - 1 are where an index error would leave the ring."""
    rng = np.random.default_rng(1000 * U + 10 * S + A)
    pairs = np.stack([rng.integers(0, frames, U * S), rng.integers(0, n_agents, U * S)], 1).astype(np.int32)
    corners = [(frames - 1, n_agents - 1), (0, 0), (0, n_agents - 1), (frames - 1, 0)]
    for i, c in enumerate(corners[:min(4, U * S)]):
        pairs[-1 if i == 0 else i - 1] = c
    return pairs.reshape(U, S, 2)


def states_of(ring_rows, pairs):
    return ring_rows[pairs[..., 0], pairs[..., 1]]


def q64(flat, X, A, dueling):
    n2 = A + (1 if dueling else 0)
    W1, b1, W2, b2 = unflatten(flat, W, HID, n2)
    X = np.asarray(X, dtype=np.float64)
    return forward_f64(X, W1, b1, W2, b2, dueling, A)[2], q_abs_f64(X, W1, b1, W2, b2, dueling, A)


def step_distances(flats, p, X, A, dueling):
    """-> (d [U], bar [U]) in float64 for step p on the blocks as they are; entry p is 0."""
    U = len(flats)
    d, bar = np.zeros(U), np.zeros(U)
    qp, ap = q64(flats[p], X, A, dueling)
    for j in range(U):
        if j == p:
            continue
        qj, aj = q64(flats[j], X, A, dueling)
        e, beta = qp - qj, TAU_Q * (ap + aj)
        d[j] = np.mean(e * e)
        bar[j] = np.mean(2 * np.abs(e) * beta + beta * beta) + 2.0 ** -16 * d[j]
    return d, bar


def stable_choice(d_row, p):
    """The others sorted by distance, stably (ties keep the index order); the first (U - 1) // 2."""
    others = [j for j in range(len(d_row)) if j != p]
    order = sorted(others, key=lambda j: d_row[j])
    return order[:len(others) // 2]


def gap_margin(d, bar, p):
    """min over the neighbours that matter of (d_next - d_this) / (4 max(bar)); > 1 = the gap condition holds.  inf when nothing
    is chosen (no choice to pin) or nobody is left out and one is chosen."""
    others = sorted([j for j in range(len(d)) if j != p], key=lambda j: d[j])
    k = len(others) // 2
    worst = np.inf
    for i in range(min(k, len(others) - 1)):
        a, b = others[i], others[i + 1]
        worst = min(worst, (d[b] - d[a]) / (4 * max(bar[a], bar[b])))
    return worst


def merge_f32(flats, p, chosen, reciprocal=False):
    """w_p <- (w_p + w_c0 + w_c1 ...) / (k + 1): f32 adds in chosen order, a true f32 division (reciprocal: the mutation that
    multiplies by float32(1 / (k + 1)) instead).  In place."""
    if not chosen:
        return
    t = flats[p].astype(np.float32).copy()
    for c in chosen:
        t = (t + flats[c]).astype(np.float32)
    n = np.float32(len(chosen) + 1)
    flats[p] = (t * (np.float32(1.0) / n) if reciprocal else t / n).astype(np.float32)


def restate(flats, states, A, dueling, reciprocal=False):
    """The whole merge, sequential in p, choosing on float64 distances.  states[p]: [S, 100].  flats is changed in place.
    -> (chosen lists, d [U, U], bar [U, U], the smallest gap margin)."""
    U = len(flats)
    chosen_all, D, B, margin = [], np.zeros((U, U)), np.zeros((U, U)), np.inf
    for p in range(U):
        D[p], B[p] = step_distances(flats, p, states[p], A, dueling)
        margin = min(margin, gap_margin(D[p], B[p], p))
        ch = stable_choice(D[p], p)
        chosen_all.append(ch)
        merge_f32(flats, p, ch, reciprocal)
    return chosen_all, D, B, margin
