"""The uniform-replay layer at the ring's edges: the keyed Feistel permutation and its cycle-walk (replay_perm, replay_perm_apply),
the slot -> (frame, agent) division by multiplication (replay_slot_to_frame; csrc/uavenv_device.hpp), the four draw and gather
kernels of csrc/replay.hip (k_replay_draw, k_replay_draw_valid, k_replay_draw_slots, k_sample_gather in its three row formats) and
the four in-kernel copies of the draw in csrc/learner.hip -- against oracle/philox.py, through the C ABI, on hand-built rings whose
rows say which (frame, agent) they are (tests/replay_draw_checks.py).  Every check is an exact integer or bitwise equality; every
output has 130 sentinel rows behind it.

 (a) uavenv_replay_draw at D = filled * n_agents stored rows in {1 ... 9, 63, 64, 65, 2^11 + 1, 2^12 + 1, 2^16, 2^17 - 1}: below
     64, powers of two (the cycle-walk never iterates), 2^k + 1 (it rejects almost every second pass; 2^12 + 1 has 13 bits, so the
     Feistel halves differ in width); every D as filled x n_agents with n_agents 1 (the multiplier saturates), 3, a power of two and
     each prime factor; head 0, mid-ring and frames - 1 (frames behind head wrap below 0); the ring full (filled = frames - 1) and
     not; batch = D (a permutation of all D rows) and D + 7 (the wrap); seed and counter above 2^32.
 (b) 32 bits: D = 65 536 x 65 535 and D = (2^31 - 2) x 2, and 31 bits with n_agents = 1 at filled = 2^31 - 2, the largest that
     `filled` (an int32 below `frames`) can hold; the first size the entry point refuses (D = 2^32) returns EINVAL and writes nothing.
 (c) the second trip of every grid-stride loop: uavenv_replay_draw, _valid and _slots at 2 048 * 256 + 300 draws over D = 2^20 + 1;
     uavenv_replay_sample at batch 21 000 on an f32 and an f16 ring and at batch 105 000 on a packed ring of 4 x 1 000 rows (the
     batch wraps 26 times past D: the reference raises there, the ring repeats draw s - D).
 (d) uavenv_replay_sample in all three row formats: obs, next-obs, action, reward, done and valid are the ring's at (f, a) and
     ((f + 1) mod frames, a), bit for bit; valid_b NULL, ring.valid NULL (-> 1.0), f = frames - 1 with its next row in frame 0;
     D in {5, 65, 2^11 + 1}.
 (e) uavenv_replay_draw_valid / _slots at D far below, one below, at, one above and eight times the draws S = batch * n_slots, for
     1, 2 and 4 UAV slots, first_slot > 0 with n_slots < U, planes all valid / 60 % valid / one slot without a valid row,
     max_tries 1 and 8: every pair a stored row, a valid one exactly where the oracle found one.  Try t of draw s looks at position
     (s mod D) + t S: before this module's change draw s >= D returned (frame 0, env 0).
 (f) the in-kernel draw of all nine gradient forms (the four draw sites of csrc/learner.hip) on a wrapped 4-frame ring of 683 agents
     (D = 2 049): the partial sums equal, bit for bit, those of the same launch fed the oracle's pairs.
 (g) DQNSlotsHotLoop at 4 envs x 4 slots, batch 64, valid_draws: from the first learning pass (D = 68) until D >= 256 the loop's
     draws are the oracle's, stored rows all, and no slot learns from 64 copies of one row.
 (h) on the host: six wrong restatements (halves swapped, five rounds, `% D` for the cycle-walk, the quotient one short without its
     correction, f = head - back, try stride batch) put through the same checks, each rejected by the check named there -- and
     invisible at exactly the sizes the suite ran before (powers of two, even bit counts, one slot), which is why (a) - (e) have the
     cases they have.

One MI355X run of (a) - (g): no mismatch; the module's 45 GPU tests take about 3 s of wall time together (the slowest, (c) on the
draw kernels, 0.4 s).  The same run against the kernels as they were before the (s mod D) rule: (e) fails at every U (first at
D = 20, 36 and 68 for S = 64, 128 and 256) and (g) at its first learning pass (D = 68), everything else passes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_draw_checks as rc
import test_dqn_grad_kernels_gpu as G
from oracle import philox as px

gpu = pytest.mark.gpu

M64 = (1 << 64) - 1
SEED, COUNTER = (0x1234 << 32) | 0x9ABCDEF1, (5 << 32) | 77
DRAW_D = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 2 ** 11 + 1, 2 ** 12 + 1, 2 ** 16, 2 ** 17 - 1]


def _L():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


def draw_cases(D, full=True):
    """(n_agents, filled, frames, head, batch) of (a) for one D; full=False: one ring length and head per factorisation."""
    for n in rc.factorisations(D):
        filled = D // n
        for frames in ((filled + 1, filled + 4) if full else (filled + 1,)):
            for head in (sorted({0, frames // 2, frames - 1}) if full else (frames // 2,)):
                for batch in (D, D + 7):
                    yield n, filled, frames, head, batch


def planes(rng, frames, n_envs, U, dead_slot):
    """All rows valid; 60 % valid; slot dead_slot without a single valid row."""
    dead = (rng.random((frames, n_envs, U)) < 0.9).astype(np.uint8)
    dead[:, :, dead_slot] = 0
    return [np.ones((frames, n_envs, U), dtype=np.uint8), (rng.random((frames, n_envs, U)) < 0.6).astype(np.uint8), dead]


def _envs_for(D):
    """D = filled x n_envs: n_envs the smallest prime factor of a composite D, 1 for a prime."""
    d = 2
    while d * d <= D:
        if D % d == 0:
            return d
        d += 1
    return 1


def valid_cases(U, batch=64):
    """(n_slots, first_slot, n_envs, filled, frames, head, plane index, plane, max_tries) of (e) for U slots per env."""
    rng = np.random.default_rng([3, U])
    for n_slots, first in [(U, 0)] + ([(U // 2, 1)] if U > 1 else []):
        S = batch * n_slots
        for D, n_envs in ((S // 4 + 4, 4), (S - 1, _envs_for(S - 1)), (S, 4), (S + 1, _envs_for(S + 1)), (8 * S + 8, 8)):
            filled = D // n_envs
            frames = filled + 1 + filled % 2
            head = (3 * filled + 1) % frames
            for k, plane in enumerate(planes(rng, frames, n_envs, U, first)):
                for max_tries in (1, 8):
                    yield n_slots, first, n_envs, filled, frames, head, k, plane, max_tries


# ---- (a) ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("D", DRAW_D)
def test_draw_is_the_oracles_permutation_of_the_stored_rows(D):
    lib = _L().load()
    counter = COUNTER + D
    for n, filled, frames, head, batch in draw_cases(D):
        want = rc.oracle_draws(batch, SEED, counter, head, filled, frames, n)
        got = rc.draw_raw(lib.uavenv_replay_draw, batch, frames, n, head, filled, batch, SEED, counter)
        try:
            rc.check_draw(got[:, 0], got[:, 1], want, head, filled, frames, n)
        except AssertionError as e:
            raise AssertionError("D %d = %d x %d, frames %d, head %d, batch %d: %s" % (D, filled, n, frames, head, batch, e))


# ---- (b) ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("frames,filled,n", [(65537, 65536, 65535), (2 ** 31 - 1, 2 ** 31 - 2, 2), (2 ** 31 - 1, 2 ** 31 - 2, 1)],
                         ids=["32bits-65535-agents", "32bits-2-agents", "31bits-1-agent"])
def test_draw_at_the_widest_permutation(frames, filled, n):
    lib, batch = _L().load(), 4096
    assert (filled * n - 1).bit_length() == (31 if n == 1 else 32)
    for head in (0, frames // 2, frames - 1):
        want = px.replay_draws(batch, SEED, COUNTER, head, filled, frames, n)
        got = rc.draw_raw(lib.uavenv_replay_draw, batch, frames, n, head, filled, batch, SEED, COUNTER)
        rc.check_draw(got[:, 0], got[:, 1], want, head, filled, frames, n)
        back = (head - 1 - got[:, 0]) % frames
        assert (back * n + got[:, 1]).max() > 0.99 * filled * n          # slots next to D - 1 went through the division


@gpu
def test_draw_refuses_2_to_the_32_rows_and_writes_nothing():
    L = _L()
    lib = L.load()
    rc.draw_raw(lib.uavenv_replay_draw, 4096, 65537, 65536, 0, 65536, 4096, SEED, COUNTER, expect=L.EINVAL)     # D = 2^32
    got = rc.draw_raw(lib.uavenv_replay_draw, 64, 65537, 65536, 0, 65535, 64, SEED, COUNTER)                  # D = 2^32 - 65536
    assert got is not None


# ---- (c) ---------------------------------------------------------------------------------------------------------------------

BIG_D, BIG_S = 2 ** 20 + 1, 2048 * 256 + 300          # D = 17 x 61 681; S = 4 x 131 147: past the 2 048-workgroup cap


@gpu
def test_draw_kernels_go_round_their_grid_stride_loops_twice():
    L = _L()
    lib = L.load()
    filled, n, frames, head = 17, 61681, 18, 7
    assert filled * n == BIG_D and BIG_S > 2048 * 256
    want = px.replay_draws(BIG_S, SEED, COUNTER, head, filled, frames, n)
    got = rc.draw_raw(lib.uavenv_replay_draw, BIG_S, frames, n, head, filled, BIG_S, SEED, COUNTER)
    rc.check_draw(got[:, 0], got[:, 1], want, head, filled, frames, n)
    U, batch = 4, BIG_S // 4
    assert U * batch == BIG_S
    plane = (np.random.default_rng(5).random((frames, n, U)) < 0.6).astype(np.uint8)
    v = torch.tensor(plane.reshape(frames, n * U)).cuda().contiguous()
    wv = px.replay_draws_valid(batch, U, U, 0, plane, L.DRAW_MAX_TRIES, SEED, COUNTER, head, filled, frames, n)
    got = rc.draw_raw(lib.uavenv_replay_draw_valid, BIG_S, frames, n, head, filled, batch, U, U, 0, v.data_ptr(), L.DRAW_MAX_TRIES,
                      SEED, COUNTER)
    rc.check_valid_draw(got[:, 0], got[:, 1], wv, plane, batch, U, U, 0, head, filled, frames, n)
    assert wv[2].mean() > 0.8 and not np.array_equal(wv[0], want[0])             # second tries were taken (one fits: 2 S > D)
    ws = px.replay_draws_slots(batch, U, plane, L.DRAW_MAX_TRIES, SEED, COUNTER, head, filled, frames, n)
    got = rc.draw_raw(lib.uavenv_replay_draw_slots, BIG_S, frames, n, head, filled, batch, U, v.data_ptr(), L.DRAW_MAX_TRIES, SEED,
                      COUNTER)
    assert np.array_equal(got[:, 0], ws[0]) and np.array_equal(got[:, 1], ws[1])
    ws = px.replay_draws_slots(batch, U, None, 0, SEED, COUNTER, head, filled, frames, n)
    got = rc.draw_raw(lib.uavenv_replay_draw_slots, BIG_S, frames, n, head, filled, batch, U, None, 0, SEED, COUNTER)
    assert np.array_equal(got[:, 0], ws[0]) and np.array_equal(got[:, 1], ws[1])


@gpu
@pytest.mark.parametrize("kind,frames,n,batch", [("f32", 8, 3001, 21000), ("f16", 8, 3001, 21000), ("packed", 5, 1000, 105000)])
def test_sample_goes_round_its_grid_stride_loop_twice(kind, frames, n, batch):
    filled, head = frames - 1, 2
    assert batch * (10 if kind == "packed" else 50) > 4096 * 256                 # past the 4 096-workgroup cap
    ring = rc.RowRing(kind, frames, n)
    f, a = px.replay_draws(batch, SEED, COUNTER, head, filled, frames, n)
    if kind == "packed":
        assert batch > 26 * filled * n and np.array_equal(f[filled * n:2 * filled * n], f[:filled * n])        # the wrap
    out = rc.sample(ring, head, filled, batch, SEED, COUNTER)
    rc.check_sample(out, ring, f, a)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("kind", ["f32", "f16", "packed"])
@pytest.mark.parametrize("D", [5, 65, 2 ** 11 + 1])
def test_sample_returns_the_rows_the_oracle_names(kind, D):
    last_frame_seen = 0
    for n in rc.factorisations(D):
        filled = D // n
        frames = filled + 1
        rings = [rc.RowRing(kind, frames, n), rc.RowRing(kind, frames, n, with_valid=False)]
        for head in sorted({0, frames // 2, frames - 1}):
            for batch in (D, D + 7):
                f, a = rc.oracle_draws(batch, SEED, COUNTER + D, head, filled, frames, n)
                last_frame_seen += int((f == frames - 1).sum())                  # its next row is in frame 0
                for ring in rings:
                    for want_valid in (True, False):
                        out = rc.sample(ring, head, filled, batch, SEED, COUNTER + D, want_valid=want_valid)
                        rc.check_sample(out, ring, f, a, want_valid=want_valid)
    assert last_frame_seen > 0


# ---- (e) ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("U", [1, 2, 4])
def test_valid_and_slot_draws_around_the_stored_row_count(U):
    L = _L()
    lib = L.load()
    batch, counter = 64, COUNTER + U
    short = 0
    for n_slots, first, n_envs, filled, frames, head, k, plane, max_tries in valid_cases(U, batch):
        S, D = batch * n_slots, filled * n_envs
        short += S > D
        where = "U %d, slots %d from %d, D %d = %d x %d, S %d, plane %d, tries %d" % (U, n_slots, first, D, filled, n_envs, S, k, max_tries)
        v = torch.tensor(plane.reshape(frames, n_envs * U)).cuda().contiguous()
        want = px.replay_draws_valid(batch, n_slots, U, first, plane, max_tries, SEED, counter, head, filled, frames, n_envs)
        got = rc.draw_raw(lib.uavenv_replay_draw_valid, S, frames, n_envs, head, filled, batch, n_slots, U, first, v.data_ptr(), max_tries,
                          SEED, counter)
        try:
            rc.check_valid_draw(got[:, 0], got[:, 1], want, plane, batch, n_slots, U, first, head, filled, frames, n_envs)
        except AssertionError as e:
            raise AssertionError(where + ": " + str(e))
        if k == 0:                                                            # every row valid: uavenv_replay_draw's rows, wrap included
            all_rows = rc.draw_raw(lib.uavenv_replay_draw, S, frames, n_envs, head, filled, S, SEED, counter)
            assert np.array_equal(got, all_rows), where
        if n_slots == U:
            slot = np.arange(S) // batch
            ws = px.replay_draws_slots(batch, U, plane, max_tries, SEED, counter, head, filled, frames, n_envs)
            gs = rc.draw_raw(lib.uavenv_replay_draw_slots, S, frames, n_envs, head, filled, batch, U, v.data_ptr(), max_tries, SEED, counter)
            assert np.array_equal(gs[:, 0], ws[0]) and np.array_equal(gs[:, 1], ws[1]), where
            assert np.array_equal(gs[:, 0], got[:, 0]) and np.array_equal(gs[:, 1], got[:, 1] * U + slot), where
            rc.check_stored_rows(gs[:, 0], gs[:, 1], head, filled, frames, n_envs * U)
            assert np.array_equal(plane.reshape(frames, n_envs * U)[gs[:, 0], gs[:, 1]] != 0, ws[2]), where
            if k == 0 and max_tries == 1:                                     # and without a plane
                wn = px.replay_draws_slots(batch, U, None, 0, SEED, counter, head, filled, frames, n_envs)
                gn = rc.draw_raw(lib.uavenv_replay_draw_slots, S, frames, n_envs, head, filled, batch, U, None, 0, SEED, counter)
                assert np.array_equal(gn[:, 0], wn[0]) and np.array_equal(gn[:, 1], wn[1]), where
                assert np.array_equal(gn, gs), where
    assert short > 0


# ---- (f) ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("form", sorted(G.FORMS))
def test_in_kernel_draw_equals_the_oracles_pairs(form):
    obs_kind, _, use_img, A = G.FORMS[form]
    frames, n, filled, head, B = 4, 683, 3, 1, 1024
    ring = rc.FloatRing(obs_kind, frames, n, A, head, filled, seed=len(form) + A)
    L = G.make_learner(form, "dqn", False, 3)
    img = L.split_image() if use_img else None
    seed, counter = SEED + 1, COUNTER + 2
    f, a = px.replay_draws(B, seed, counter, head, filled, frames, n)
    assert (f == frames - 1).any() and (f == 0).any() and len(np.unique(f * n + a)) == B
    idx = torch.tensor(np.stack([f, a], 1).astype(np.int32), device="cuda").contiguous()

    def run(pairs):
        parts = L.new_partials(B).zero_()
        abs_td = torch.full((B,), -1.0, device="cuda")
        G.launch(L, ring, B, pairs, None, abs_td, img, parts.data_ptr(), seed, counter)
        torch.cuda.synchronize()
        return parts.cpu().numpy().view(np.uint32), abs_td.cpu().numpy().view(np.uint32)

    p_draw, t_draw = run(None)
    p_idx, t_idx = run(idx)
    assert np.array_equal(t_draw, t_idx), np.flatnonzero(t_draw != t_idx)[:8]
    assert np.array_equal(p_draw, p_idx)
    assert np.isfinite(p_draw.view(np.float32)).all() and p_draw.any()
    # the comparison can tell pairs apart: the same batch one draw further on gives other sums
    f2, a2 = px.replay_draws(B + 1, seed, counter, head, filled, frames, n)
    p_other, _ = run(torch.tensor(np.stack([f2[1:], a2[1:]], 1).astype(np.int32), device="cuda").contiguous())
    assert not np.array_equal(p_other, p_idx)


# ---- (g) ---------------------------------------------------------------------------------------------------------------------

@gpu
def test_slots_loop_draws_stored_rows_from_its_first_learning_pass():
    from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
    L = _L()
    n_envs, U, batch = 4, 4, 64
    env = make_city26_env(n_envs, obs_dtype="packed", uav_per_env=U)
    ring = DeviceReplayRing(env, 70 * env.N, discrete=True)
    ring.reset(seed=12)
    assert ring.frames == 71 and env.N == n_envs * U
    Ls = []
    for j in range(U):
        torch.manual_seed(1 + j)
        Ls.append(FusedDQNLearner(dict(G.PARAM, NetWork="Qnet2", output="3"), "dqn", device="cuda:0"))
    seed, counter0 = (0x33 << 32) | 5, (7 << 32) | 3
    loop = DQNSlotsHotLoop(ring, Ls, batch, seed=seed, eps=0.3, counter=counter0, learn_start=batch + 1, auto_reset=False,
                           skip_done=True, valid_draws=True)
    slot = np.arange(U * batch) // batch
    learning, short = 0, 0
    for _ in range(67):
        c = loop.counter
        loop.run(1)
        torch.cuda.synchronize()
        D = ring.filled * n_envs
        if D < batch + 1:
            assert all(x.epoch == 0 for x in Ls)
            continue
        learning += 1
        short += D < U * batch
        assert all(x.epoch == learning for x in Ls)
        got = loop._draws.cpu().numpy().astype(np.int64)
        plane = ring.valid.cpu().numpy()
        f, a, found = px.replay_draws_slots(batch, U, plane, L.DRAW_MAX_TRIES, (seed + 7) & M64, c, ring.head, ring.filled, ring.frames,
                                            n_envs)
        where = "pass %d, D %d" % (c - counter0, D)
        rc.check_stored_rows(got[:, 0], got[:, 1], ring.head, ring.filled, ring.frames, n_envs * U)
        assert np.array_equal(got[:, 1] % U, slot), where
        assert np.array_equal(got[:, 0], f) and np.array_equal(got[:, 1], a), where
        assert np.array_equal(plane[got[:, 0], got[:, 1]] != 0, found), where
        for j in range(U):
            rows = got[slot == j]
            assert len(np.unique(rows, axis=0)) > 1, where + ": slot %d learns from one row" % j
            hit = found[slot == j]
            assert len(np.unique(rows[hit], axis=0)) == hit.sum(), where            # batch <= D: valid rows distinct within a slot
    assert learning == 67 - 16 and short == 64 - 17 and ring.filled * n_envs >= U * batch
    assert all(torch.isfinite(x.flat).all() for x in Ls)
    loop.close()
    env.close()


# ---- (h) ---------------------------------------------------------------------------------------------------------------------

def _draw_verdicts(**mutation):
    """{D: set of the checks' names that rejected the mutated restatement somewhere among D's cases of (a)} (empty: invisible)."""
    out = {}
    for D in DRAW_D:
        seen = set()
        for n, filled, frames, head, batch in draw_cases(D, full=False):
            want = rc.oracle_draws(batch, SEED, COUNTER + D, head, filled, frames, n)
            f, a = px.replay_draws(batch, SEED, COUNTER + D, head, filled, frames, n, **mutation)
            try:
                rc.check_draw(f, a, want, head, filled, frames, n)
            except AssertionError as e:
                seen.add((str(e).split(":")[0], n))
        out[D] = seen
    return out


def _names(v):
    return {name for name, _ in v}


def test_mutation_halves_swapped_is_rejected_where_the_bit_count_is_odd():
    v = _draw_verdicts(swap_halves=True)
    for D in (65, 2 ** 12 + 1, 2 ** 17 - 1):                     # 7, 13 and 17 bits: la != lb
        assert _names(v[D]) == {"oracle"}, (D, v[D])
    for D in (64, 2 ** 11 + 1, 2 ** 16):                         # 6, 12 and 16 bits: the same network -- what the suite ran before
        assert not v[D], (D, v[D])


def test_mutation_five_rounds_is_rejected():
    v = _draw_verdicts(rounds=5)
    for D in DRAW_D:
        if D >= 63:
            assert _names(v[D]) == {"oracle"}, (D, v[D])           # still a permutation of the stored rows: only equality sees it


def test_mutation_modulo_for_the_cycle_walk_is_rejected_off_the_powers_of_two():
    v = _draw_verdicts(walk=False)
    for D in (5, 9, 65, 2 ** 11 + 1, 2 ** 12 + 1):               # 2^k + 1: almost every second pass leaves [0, D)
        assert "permutation" in _names(v[D]), (D, v[D])          # two positions share a row
    for D in (4, 8, 64, 2 ** 16):                                # the walk never iterates: what the suite ran before
        assert not v[D], (D, v[D])


def test_mutation_quotient_one_short_is_rejected_by_the_stored_row_check():
    v = _draw_verdicts(short_division=True)
    for D in DRAW_D:
        for n in rc.factorisations(D):
            exact = n > 1 and n & (n - 1) == 0                   # 2^32 / n exact: never short -- what the suite ran before
            hit = ("stored-row", n) in v[D]
            assert hit == (not exact and D > n or (n == 1 and D > 1)), (D, n, v[D])


def test_mutation_frames_behind_head_off_by_one_is_rejected_by_the_stored_row_check():
    v = _draw_verdicts(head_offset=0)
    for D in DRAW_D:
        assert _names(v[D]) == {"stored-row"} and len(v[D]) == len(rc.factorisations(D)), (D, v[D])     # the newest row is read from `head`


def test_mutation_try_stride_batch_is_rejected_with_more_than_one_slot():
    batch = 64
    for U in (1, 2, 4):
        for n_slots, first, n_envs, filled, frames, head, k, plane, max_tries in valid_cases(U, batch):
            S, D = batch * n_slots, filled * n_envs
            args = (batch, n_slots, U, first, plane, max_tries, SEED, COUNTER + U, head, filled, frames, n_envs)
            want = px.replay_draws_valid(*args)
            f, e, _ = px.replay_draws_valid(*args, stride=batch)
            try:
                rc.check_valid_draw(f, e, want, plane, batch, n_slots, U, first, head, filled, frames, n_envs)
                rejected = None
            except AssertionError as err:
                rejected = str(err).split(":")[0]
            if n_slots > 1 and k == 1 and max_tries == 8 and D >= 8 * S:
                assert rejected in ("distinct", "found", "oracle"), (U, n_slots, D, rejected)
            if n_slots == 1 or max_tries == 1 or k == 0:           # one slot (S = batch), one try, or nothing to reject: the same draws
                assert rejected is None, (U, n_slots, D, k, max_tries, rejected)
