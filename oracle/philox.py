"""TEST INFRASTRUCTURE (oracle): independent numpy restatement of the counter-based random streams the device uses.

* philox4x32_10: Salmon, Moraes, Dror, Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3" (SC'11), the
  Philox-4x32 bijection with 10 rounds, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 /
  0xBB67AE85.  Pinned against the Random123 known-answer vectors in tests/test_oracle_philox.py.
* replay_draws: which stored transitions `uavenv_replay_sample` / `uavenv_dqn_grad` must pick for update
  (seed, counter): ReplayMemory.sample2 = random.sample(memory, batch) (BaseClass/replay_buffer.py:48-51) draws
  DISTINCT transitions; the device realises that as the first `batch` images of a keyed pseudo-random permutation
  of the D = filled * n_agents stored transitions (6-round alternating Feistel network over ceil(log2 D) bits,
  cycle-walked into [0, D); csrc/uavenv_device.hpp: replay_perm / replay_perm_apply).
* replay_draws_valid / replay_draws_slots: the same draws over the valid rows only and as one (frame, agent) list for every UAV slot
  (uavenv_replay_draw_valid / uavenv_replay_draw_slots, csrc/replay.hip); draw s starts at permutation position s mod D.
* act_draws: the epsilon-greedy stream of uavenv_dqn_act / uavenv_select_actions (DuelingDQN_Trainer.py:86-97).
* the other seven device streams ("Random streams"), written from include/uavenv.h, DESIGN.md and the kernels' comments:
  randn (uavenv_randn: every rsample() of SAC training), eval_noise (evaluate.sac_noise / the SAC evaluation's sample mode),
  per_draws (the stratified draws of uavenv_per_sample), reset_draws (uavenv_reset_all and the step's auto-reset),
  eval_headings / eval_eps_draws (the evaluation kernels' default heading and eps draw), rrt_stream (the planner's own U[0,1)).
  Every stream is Philox4x32-10 keyed by the 64-bit seed; the counter's fourth word carries the stream's constant (STREAMS), which
  keeps the streams apart (tests/test_oracle_philox.py::test_fourth_counter_word_separates_the_streams).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may import this module.
"""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: (..., 4) uint32-valued, key: (2,) or (..., 2) -> (..., 4) uint32.  Vectorised over the leading axes."""
    c = np.asarray(ctr, dtype=np.uint64) & U32
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64) & U32, c.shape[:-1] + (2,)).copy()
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0 = M0 * c0                      # 32 x 32 -> 64 bit products (fit in uint64)
        p1 = M1 * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & U32
        hi1, lo1 = p1 >> np.uint64(32), p1 & U32
        c0, c1, c2, c3 = (hi1 ^ c1 ^ k0) & U32, lo1, (hi0 ^ c3 ^ k1) & U32, lo0
        k0 = (k0 + np.uint64(W0)) & U32
        k1 = (k1 + np.uint64(W1)) & U32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _key(seed: int):
    return np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)


def fmix32(h):
    """MurmurHash3's 32-bit finaliser (Appleby, public domain) on uint64-held 32-bit values."""
    h = np.asarray(h, dtype=np.uint64) & U32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & U32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & U32
    h ^= h >> np.uint64(16)
    return h


def replay_slots(batch: int, seed: int, counter, filled: int, n_agents: int, *, positions=None, swap_halves: bool = False,
                 rounds: int = 6, walk: bool = True) -> np.ndarray:
    """Transition slot (0 = newest frame's agent 0 ... D-1) of samples 0..batch-1 -- or of the permutation positions `positions`
    (any non-negative integers; taken mod D), and then `counter` may be an array of their shape: position i under the keys of
    update counter[i].  swap_halves / rounds / walk exist for the mutation tests only."""
    D = filled * n_agents
    pos = np.arange(batch, dtype=np.uint64) if positions is None else np.asarray(positions, dtype=np.uint64)
    if D <= 1:
        return np.zeros(pos.shape, dtype=np.int64)
    per_position = np.ndim(counter) > 0
    c = np.asarray(counter, dtype=np.uint64) if per_position else np.uint64(int(counter) & 0xFFFFFFFFFFFFFFFF)
    lo_c, hi_c = c & U32, c >> np.uint64(32)
    a = philox4x32_10(_words(0, lo_c, hi_c, 0x5A3B), _key(seed))
    b = philox4x32_10(_words(1, lo_c, hi_c, 0x5A3B), _key(seed))
    keys = [k.astype(np.uint64) for k in (a[..., 0], a[..., 1], a[..., 2], a[..., 3], b[..., 0], b[..., 1])]
    bits = max(2, int(D - 1).bit_length())
    la = bits // 2
    lb = bits - la
    if swap_halves:
        la, lb = lb, la
    ma = np.uint64((1 << la) - 1)
    sa, sb = np.uint64(32 - la), np.uint64(32 - lb)
    x = pos % np.uint64(D)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        v = x[todo]
        k = [kr[todo] for kr in keys] if per_position else keys
        lo, hi = v & ma, v >> np.uint64(la)
        for r in range(rounds):
            if r % 2 == 0:
                lo = lo ^ (fmix32(hi ^ k[r]) >> sa)                # even round: low part ^= F(high part)
            else:
                hi = hi ^ (fmix32(lo ^ k[r]) >> sb)                # odd round: high part ^= F(low part)
        v = (hi << np.uint64(la)) | lo
        if not walk:
            x[todo] = v % np.uint64(D)
            break
        x[todo] = v
        todo[todo] = v >= np.uint64(D)
    return x.astype(np.int64)


def slots_to_rows(slot, head: int, frames: int, n_agents: int, *, short_division: bool = False, head_offset: int = 1):
    """Transition slot -> (frame, agent): slot // n_agents + 1 frames behind the ring head.  short_division (the quotient as
    floor(slot * floor(2^32 / n_agents) / 2^32) -- at most one short -- WITHOUT the correction) and head_offset exist for the
    mutation tests only."""
    slot = np.asarray(slot, dtype=np.int64)
    if short_division:
        magic = min((1 << 32) // n_agents, 0xFFFFFFFF)
        back = ((slot.astype(np.uint64) * np.uint64(magic)) >> np.uint64(32)).astype(np.int64)    # slot, magic < 2^32: fits
    else:
        back = slot // n_agents
    agent = slot - back * n_agents
    f = (head - head_offset - back) % frames
    return f.astype(np.int64), agent.astype(np.int64)


def replay_draws(batch: int, seed: int, counter: int, head: int, filled: int, frames: int, n_agents: int, **mutation):
    """-> (frame [batch], agent [batch]) of the transitions update (seed, counter) must use.  Sample s >= D = filled * n_agents
    wraps to sample s mod D (the reference raises there).  **mutation: replay_slots' / slots_to_rows' mutation knobs."""
    to_rows = {k: mutation.pop(k) for k in ("short_division", "head_offset") if k in mutation}
    slot = replay_slots(batch, seed, counter, filled, n_agents, **mutation)
    return slots_to_rows(slot, head, frames, n_agents, **to_rows)


def replay_draws_valid(batch: int, n_slots: int, uav_per_env: int, first_slot: int, valid: np.ndarray, max_tries: int, seed: int,
                       counter: int, head: int, filled: int, frames: int, n_envs: int, *, stride=None):
    """uavenv_replay_draw_valid: -> (frame [S], env [S], found [S]), S = n_slots * batch.  valid: the ring's plane
    [frames][n_envs * uav_per_env].  Try t of draw s (slot first_slot + s // batch) looks at permutation position
    (s mod D) + t S while that is < D = filled * n_envs and t < max_tries, and stops at the first row of ITS slot with valid != 0; a
    draw that finds none keeps the row of its try 0.  S > D is defined by the `mod`: with every row valid the result is
    replay_draws(S) for every S and D, and every output is a stored row.  stride (the try stride, S) exists for the mutation tests
    only."""
    S, D = batch * n_slots, filled * n_envs
    stride = S if stride is None else stride
    first = np.arange(S, dtype=np.int64) % D
    n_pos = min(D, int(first.max()) + 1 + stride * (max_tries - 1))
    f_all, e_all = replay_draws(n_pos, seed, counter, head, filled, frames, n_envs)
    valid = np.asarray(valid).reshape(frames, n_envs, uav_per_env)
    f_out, e_out, found = f_all[first].copy(), e_all[first].copy(), np.zeros(S, dtype=bool)
    slot = first_slot + np.arange(S) // batch
    for t in range(max_tries):
        q = first + t * stride
        ok = (q < D) & ~found
        if not ok.any():
            break
        qq = q[ok]
        hit = valid[f_all[qq], e_all[qq], slot[ok]] != 0
        idx = np.nonzero(ok)[0][hit]
        f_out[idx], e_out[idx], found[idx] = f_all[qq[hit]], e_all[qq[hit]], True
    return f_out, e_out, found


def replay_draws_slots(batch: int, uav_per_env: int, valid, max_tries: int, seed: int, counter: int, head: int, filled: int,
                       frames: int, n_envs: int):
    """uavenv_replay_draw_slots: -> (frame [U * batch], agent [U * batch], found [U * batch]) with agent = env * U + slot and slot =
    s // batch (U = uav_per_env): the draws of replay_draws_valid(batch, U, U, 0, valid, ...) with a plane, of
    replay_draws(U * batch) over the n_envs-wide ring with valid None (found is all True then: no row is tested)."""
    S = batch * uav_per_env
    slot = np.arange(S, dtype=np.int64) // batch
    if valid is None:
        f, e = replay_draws(S, seed, counter, head, filled, frames, n_envs)
        found = np.ones(S, dtype=bool)
    else:
        f, e, found = replay_draws_valid(batch, uav_per_env, uav_per_env, 0, valid, max_tries, seed, counter, head, filled, frames,
                                         n_envs)
    return f, e * uav_per_env + slot, found


def act_draws(n: int, seed: int, counter: int, n_actions: int):
    """-> (u [n] float32 in [0,1), random_action [n]) of the epsilon-greedy stream: greedy iff u > eps."""
    lo, hi = counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF
    ctr = np.stack([np.arange(n, dtype=np.uint64), np.full(n, lo, np.uint64), np.full(n, hi, np.uint64),
                    np.full(n, 0xAC7, np.uint64)], axis=-1)
    r = philox4x32_10(ctr, _key(seed)).astype(np.uint64)
    u = ((r[:, 0] >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)
    rnd = ((r[:, 1] * np.uint64(n_actions)) >> np.uint64(32)).astype(np.int64)
    return u, rnd


# ---------------------------------------------------------------------------------------------------------------------
# The streams' counter words.  STREAMS: the constant in the counter's fourth word -- the domain separation.
# ---------------------------------------------------------------------------------------------------------------------
STREAMS = {"replay": 0x5A3B, "act": 0x0AC7, "randn": 0x6A55, "eval_noise": 0x5AC0, "per": 0x09E7, "reset": 0x5EED,
           "eval_heading": 0xE7A1, "eval_eps": 0xE75F, "rrt": 0x7272}
TWO_PI = 6.283185307179586                    # the f64 2 pi of random.uniform(0, 2 * pi)
TWO_PI_F32 = np.float32(6.283185307179586)    # what an f32 kernel multiplies by: 6.2831855


def _words(w0, w1, w2, w3):
    """Counter words, each a scalar or an array, broadcast together -> (..., 4) uint64 holding 32-bit values."""
    return np.stack(np.broadcast_arrays(*(np.asarray(w, dtype=np.uint64) & U32 for w in (w0, w1, w2, w3))), axis=-1)


def _split(v: int):
    return int(v) & 0xFFFFFFFF, (int(v) >> 32) & 0xFFFFFFFF


def stream_counters(name: str, index, a: int = 0, b: int = 0):
    """The counter words of stream `name` for element(s) `index`:
      replay        (index, counter_lo, counter_hi, c)        a = the update's counter; index 0 and 1 give the six round keys
      act, per      (index, counter_lo, counter_hi, c)        a = counter; index = agent / sample
      reset         (index, tick_lo, tick_hi, c)              a = tick; index = agent
      randn         (quad_lo, quad_hi, counter_lo, counter_hi ^ c)      a = counter; index = quad = element // 4
      eval_noise, eval_eps      (episode, step, 0, c)         index = episode, a = step
      eval_heading  (episode, 0, 0, c)
      rrt           (k, scenario, attempt, c)                 index = k (the k-th uniform), a = scenario, b = attempt"""
    c = STREAMS[name]
    if name in ("replay", "act", "per", "reset"):
        lo, hi = _split(a)
        return _words(index, lo, hi, c)
    if name == "randn":
        lo, hi = _split(a)
        q = np.asarray(index, dtype=np.uint64)
        return _words(q, q >> np.uint64(32), lo, hi ^ c)
    if name in ("eval_noise", "eval_eps"):
        return _words(index, a, 0, c)
    if name == "eval_heading":
        return _words(index, 0, 0, c)
    if name == "rrt":
        return _words(index, a, b, c)
    raise KeyError(name)


def u53(a, b):
    """CPython's random(): ((a >> 5) * 2^26 + (b >> 6)) * 2^-53 from two 32-bit words -> float64 in [0, 1).  Exact: the integer
    has at most 53 bits."""
    a = np.asarray(a, dtype=np.uint64) & U32
    b = np.asarray(b, dtype=np.uint64) & U32
    k = (a >> np.uint64(5)) * np.uint64(1 << 26) + (b >> np.uint64(6))
    return k.astype(np.float64) * 2.0 ** -53


class Normals:
    """Box-Muller on 24-bit uniforms, element by element: u1 in (0, 1], u2 in [0, 1) and the angle t = fl32(fl32(2 pi) u2) are the
    float32 values an f32 kernel holds (all three exact in numpy float32); rad = sqrt(-2 ln u1) and z = rad cos t (even
    elements) / rad sin t (odd elements) are float64, evaluated AT those float32 inputs."""

    def __init__(self, u1, u2, t, rad, z):
        self.u1, self.u2, self.t, self.rad, self.z = u1, u2, t, rad, z


def box_muller(w1, w2, *, shift: int = 8, plus: int = 1, two_pi=TWO_PI_F32):
    """Words w1, w2 (same shape S) -> Normals of shape S + (2,): [..., 0] the cosine branch, [..., 1] the sine branch.
    u1 = ((w1 >> 8) + 1) 2^-24, u2 = (w2 >> 8) 2^-24.  shift / plus / two_pi exist for the mutation tests only."""
    w1 = np.asarray(w1, dtype=np.uint64) & U32
    w2 = np.asarray(w2, dtype=np.uint64) & U32
    s = np.float32(2.0 ** -24)
    u1 = ((w1 >> np.uint64(shift)) + np.uint64(plus)).astype(np.float32) * s
    u2 = (w2 >> np.uint64(shift)).astype(np.float32) * s
    t = (two_pi * u2).astype(np.float32)               # f32 x f32 -> one f32 rounding; an f64 two_pi rounds the f64 product
    with np.errstate(divide="ignore"):
        rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    t64 = t.astype(np.float64)
    z = np.stack([rad * np.cos(t64), rad * np.sin(t64)], axis=-1)
    two = lambda x: np.stack([x, x], axis=-1)          # noqa: E731
    return Normals(two(u1), two(u2), two(t), two(rad), z)


def _flatten_pairs(parts, n):
    """Normals of shape (quads, 2 pairs, 2 components) -> the first n elements in element order."""
    return Normals(*(getattr(parts, k).reshape(-1)[:n] for k in ("u1", "u2", "t", "rad", "z")))


def randn(n: int, seed: int, counter: int) -> Normals:
    """uavenv_randn(seed, counter, n): elements 4q .. 4q + 3 come from the four words (x, y, z, w) of quad q's Philox block:
    (x, y) -> ra cos, ra sin; (z, w) -> rb cos, rb sin."""
    quads = (int(n) + 3) // 4
    r = philox4x32_10(stream_counters("randn", np.arange(quads, dtype=np.uint64), counter), _key(seed))
    return _flatten_pairs(box_muller(r[:, [0, 2]], r[:, [1, 3]]), n)


def eval_noise(n: int, steps: int, seed: int) -> Normals:
    """evaluate.sac_noise(n, steps, seed): arrays [n, steps, 2]; component 0 is the cosine branch, component 1 the sine branch of
    the block of (episode, step)."""
    e = np.arange(n, dtype=np.uint64)[:, None]
    st = np.arange(steps, dtype=np.uint64)[None, :]
    r = philox4x32_10(stream_counters("eval_noise", e, st), _key(seed))
    return box_muller(r[..., 0], r[..., 1])


def per_draws(batch: int, seed: int, counter: int, total: float) -> np.ndarray:
    """The stratified draws of ReplayTree.sample (replay_buffer.py:147, :160-162) as uavenv_per_sample makes them without a
    caller's stream: random.uniform(seg i, seg (i + 1)) = a + (b - a) random() with seg = int(total) / batch, pulled back onto
    `total` (the library's clamp).  Plain float64, one rounding per operation."""
    i = np.arange(batch, dtype=np.uint64)
    r = philox4x32_10(stream_counters("per", i, counter), _key(seed))
    seg = np.floor(np.float64(total)) / np.float64(batch)
    a = seg * i.astype(np.float64)
    b = seg * (i.astype(np.float64) + 1.0)
    v = a + (b - a) * u53(r[:, 0], r[:, 1])
    return np.minimum(v, np.float64(total))


def reset_draws(n: int, seed: int, tick: int, m: int):
    """UAV.reset() of agents 0..n-1 at `tick` from a bank of m scenarios -> (scn [n] int64, heading [n] float64): the scenario is
    floor(z m / 2^32) from the block's third word, the heading random.uniform(0, 2 pi) = 2 pi u53(x, y)."""
    r = philox4x32_10(stream_counters("reset", np.arange(n, dtype=np.uint64), tick), _key(seed))
    scn = ((r[:, 2].astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
    return scn, TWO_PI * u53(r[:, 0], r[:, 1])


def eval_headings(n: int, seed: int) -> np.ndarray:
    """The default initial heading of evaluation episodes 0..n-1 (v0 = None): 2 pi u53(x, y)."""
    r = philox4x32_10(stream_counters("eval_heading", np.arange(n, dtype=np.uint64)), _key(seed))
    return TWO_PI * u53(r[:, 0], r[:, 1])


def eval_eps_draws(n: int, steps: int, seed: int, n_actions: int):
    """-> (u [n, steps] float32 in [0, 1), random_action [n, steps]): step t of episode e takes random_action where u < eps
    (strict), the greedy action otherwise."""
    e = np.arange(n, dtype=np.uint64)[:, None]
    st = np.arange(steps, dtype=np.uint64)[None, :]
    r = philox4x32_10(stream_counters("eval_eps", e, st), _key(seed)).astype(np.uint64)
    u = (r[..., 0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    rnd = ((r[..., 1] * np.uint64(n_actions)) >> np.uint64(32)).astype(np.int64)
    return u, rnd


def rrt_stream(seed: int, scenario: int, attempt: int, length: int) -> np.ndarray:
    """The planner's own random() for (scenario, attempt): uniforms 0..length-1, u53 of the first two words of block k."""
    r = philox4x32_10(stream_counters("rrt", np.arange(length, dtype=np.uint64), scenario, attempt), _key(seed))
    return u53(r[:, 0], r[:, 1])
