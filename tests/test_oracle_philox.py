"""oracle/philox.py pinned: Random123's published known-answer vectors for philox4x32_10 (kat_vectors, Salmon et al.),
and the structural properties the replay draw relies on (a permutation: distinct draws, full coverage).

The other streams' restatements (randn, eval_noise, per_draws, reset_draws, eval_headings, eval_eps_draws, rrt_stream) are what
tests/test_random_streams_gpu.py holds the device to, value by value; here their own properties are pinned: u53's range, the
standard-normal law of the Box-Muller streams (the distribution claim lives HERE -- the GPU tests compare numbers), the
stratification of the prioritised draws, and the separation of the nine streams by the counter's fourth word."""
import numpy as np

from oracle import philox as px

# the planner case of tests/test_random_streams_gpu.py: seed, rows, uniforms per row, and the lowered max_iter of its second case
RRT_SEED, RRT_ROWS, RRT_LEN, RRT_MAX_ITER_LOW = (0x7272 << 32) | 11, 64, 6000, 84


def test_philox4x32_10_known_answers():
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, want in kat:
        got = px.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert tuple(int(v) for v in got) == want


def test_replay_slots_are_a_permutation():
    for filled, n in ((1, 64), (3, 100), (7, 1000), (63, 1024), (5, 1), (2, 3)):
        D = filled * n
        s = px.replay_slots(D, seed=9, counter=4, filled=filled, n_agents=n)
        assert sorted(s.tolist()) == list(range(D))                  # all D draws distinct = random.sample semantics
        s2 = px.replay_slots(D, seed=9, counter=5, filled=filled, n_agents=n)
        if D > 8:
            assert (s != s2).mean() > 0.5                            # another update, another permutation
    # batch > D wraps around (the reference raises there)
    s = px.replay_slots(10, seed=1, counter=0, filled=1, n_agents=4)
    assert (s[:4] == s[4:8]).all() and len(set(s[:4].tolist())) == 4


def test_replay_draws_map_slots_to_frames_behind_head():
    f, a = px.replay_draws(5000, seed=3, counter=1, head=2, filled=5, frames=8, n_agents=1000)
    assert set(np.unique(f).tolist()) == {1, 0, 7, 6, 5}             # 1..5 frames behind head 2, ring of 8
    assert a.min() >= 0 and a.max() < 1000
    # uniform over frames: 5000 of 5000 slots -> exactly 1000 per frame
    assert all((f == k).sum() == 1000 for k in (1, 0, 7, 6, 5))


def test_act_draws_range():
    u, r = px.act_draws(4096, seed=7, counter=3, n_actions=3)
    assert u.min() >= 0.0 and u.max() < 1.0 and set(np.unique(r).tolist()) == {0, 1, 2}
    assert abs(u.mean() - 0.5) < 0.03


def test_valid_only_draws_reject_over_the_permutation():
    """replay_draws_valid (the restatement uavenv_replay_draw_valid is tested against on the GPU): draws walk the permutation past
    rows whose valid flag is 0 -- accepted rows are valid rows of the draw's own slot, distinct within a slot, inside the stored
    frames; with every row valid they are replay_draws'; a draw that runs out of tries keeps its first row."""
    frames, n_envs, U, head, filled, batch = 17, 512, 4, 5, 16, 256
    rng = np.random.default_rng(1)
    valid = (rng.random((frames, n_envs * U)) >= 0.4).astype(np.uint8)
    f, e, found = px.replay_draws_valid(batch, U, U, 0, valid, 8, seed=5, counter=2, head=head, filled=filled, frames=frames, n_envs=n_envs)
    slot = np.arange(U * batch) // batch
    assert (valid.reshape(frames, n_envs, U)[f, e, slot][found] == 1).all()
    assert found.mean() > 0.995                                        # 0.4 ** 8 = 7e-4
    f0, e0 = px.replay_draws(U * batch, 5, 2, head, filled, frames, n_envs)
    assert (f[~found] == f0[~found]).all() and (e[~found] == e0[~found]).all()
    back = (head - 1 - f) % frames
    assert back.max() < filled
    for j in range(U):
        m = (slot == j) & found
        assert len(np.unique(back[m] * n_envs + e[m])) == m.sum()
    fa, ea, fo = px.replay_draws_valid(batch, U, U, 0, np.ones_like(valid), 8, 5, 2, head, filled, frames, n_envs)
    assert fo.all() and (fa == f0).all() and (ea == e0).all()
    # one slot alone, and a ring too small for a second try: positions past filled * n_envs are never looked at
    f1, e1, fo1 = px.replay_draws_valid(batch, 1, U, 3, valid, 8, 5, 2, head, filled, frames, n_envs)
    assert (valid.reshape(frames, n_envs, U)[f1, e1, 3][fo1] == 1).all()
    f2, e2, fo2 = px.replay_draws_valid(filled * n_envs, 1, U, 0, valid, 8, 5, 2, head, filled, frames, n_envs)
    fs, es = px.replay_draws(filled * n_envs, 5, 2, head, filled, frames, n_envs)
    assert (f2 == fs).all() and (e2 == es).all()                       # no second position exists: every draw keeps its first row


def _planes(rng, frames, n_envs, U):
    """All rows valid; 60 % valid; one slot (the last) without a single valid row."""
    dead = (rng.random((frames, n_envs, U)) < 0.9).astype(np.uint8)
    dead[:, :, U - 1] = 0
    return [np.ones((frames, n_envs, U), dtype=np.uint8), (rng.random((frames, n_envs, U)) < 0.6).astype(np.uint8), dead]


def _valid_draws_one_by_one(batch, n_slots, U, first_slot, valid, max_tries, seed, counter, head, filled, frames, n_envs):
    """The rule of replay_draws_valid as a loop over draws and tries: try t of draw s looks at (s mod D) + t S while that is < D."""
    S, D = batch * n_slots, filled * n_envs
    fp, ep = px.replay_draws(D, seed, counter, head, filled, frames, n_envs)            # the whole permutation
    valid = np.asarray(valid).reshape(frames, n_envs, U)
    out = []
    for s in range(S):
        slot, row, hit = first_slot + s // batch, None, False
        for t in range(max_tries):
            p = s % D + t * S
            if p >= D:
                break
            if t == 0:
                row = (fp[p], ep[p])
            if valid[fp[p], ep[p], slot]:
                row, hit = (fp[p], ep[p]), True
                break
        out.append((row[0], row[1], hit))
    o = np.array(out, dtype=np.int64)
    return o[:, 0], o[:, 1], o[:, 2].astype(bool)


def test_valid_only_draws_with_more_draws_than_stored_rows():
    """S = n_slots * batch draws over D = filled * n_envs stored rows, D far below, just below, at, just above and far above S (the
    slots loop learns from `batch` stored rows on while it draws for every slot: 4 envs x 4 slots x batch 64 start at D = 68 <
    S = 256).  Every output has length S and names a stored row; with every row valid the result is replay_draws(S), wrap
    included; rows are distinct within a slot whenever batch <= D; found is true exactly where the returned row is valid."""
    batch, n_envs = 64, 4
    rng = np.random.default_rng(11)
    for U, n_slots, first_slot in ((4, 4, 0), (2, 2, 0), (1, 1, 0), (4, 2, 1)):
        S = batch * n_slots
        fills = sorted({1, 3, 16, 17, (S - 1) // n_envs, S // n_envs, S // n_envs + 1, 8 * S // n_envs})
        for filled in fills:
            D = filled * n_envs
            frames = filled + 1 + filled % 3
            head = (5 * filled) % frames
            for max_tries in (1, 8):
                for k, plane in enumerate(_planes(rng, frames, n_envs, U)):
                    args = (batch, n_slots, U, first_slot, plane, max_tries, 0x5EED00000007, (3 << 32) + filled, head, filled, frames, n_envs)
                    f, e, found = px.replay_draws_valid(*args)
                    assert f.shape == e.shape == found.shape == (S,)
                    f1, e1, found1 = _valid_draws_one_by_one(*args)
                    assert np.array_equal(f, f1) and np.array_equal(e, e1) and np.array_equal(found, found1)
                    back = (head - 1 - f) % frames
                    assert back.min() >= 0 and back.max() < filled and e.min() >= 0 and e.max() < n_envs      # a stored row
                    slot = first_slot + np.arange(S) // batch
                    assert np.array_equal(found, plane[f, e, slot] != 0)
                    f0, e0 = px.replay_draws(S, args[6], args[7], head, filled, frames, n_envs)
                    assert np.array_equal(f[~found], f0[~found]) and np.array_equal(e[~found], e0[~found])   # try 0's row kept
                    if k == 0:
                        assert found.all() and np.array_equal(f, f0) and np.array_equal(e, e0)
                    if k == 2 and first_slot + n_slots == U:
                        assert not found[slot == U - 1].any()
                    if batch <= D:
                        for j in range(n_slots):
                            m = (slot == first_slot + j) & found
                            assert len(np.unique(back[m] * n_envs + e[m])) == m.sum()
                    if S <= D:                                            # nothing wraps: S distinct first positions
                        assert len(np.unique((head - 1 - f0) % frames * n_envs + e0)) == S


def test_draws_for_every_slot_as_frame_agent_pairs():
    """replay_draws_slots restates uavenv_replay_draw_slots: (frame, env * U + slot); with a plane the rows of replay_draws_valid for
    all U slots, without one those of replay_draws(U * batch) -- the two agree when every row is valid, for S below and above D."""
    batch, n_envs, U = 64, 4, 4
    S = batch * U
    slot = np.arange(S) // batch
    rng = np.random.default_rng(12)
    for filled in (1, 17, 63, 64, 65, 600):
        frames, head = filled + 2, filled // 2
        f0, e0 = px.replay_draws(S, 21, 1 << 33, head, filled, frames, n_envs)
        fa, aa, fo = px.replay_draws_slots(batch, U, None, 8, 21, 1 << 33, head, filled, frames, n_envs)
        assert fo.all() and np.array_equal(fa, f0) and np.array_equal(aa, e0 * U + slot)
        for k, plane in enumerate(_planes(rng, frames, n_envs, U)):
            fv, ev, found = px.replay_draws_valid(batch, U, U, 0, plane, 8, 21, 1 << 33, head, filled, frames, n_envs)
            fs, as_, fos = px.replay_draws_slots(batch, U, plane, 8, 21, 1 << 33, head, filled, frames, n_envs)
            assert np.array_equal(fs, fv) and np.array_equal(as_, ev * U + slot) and np.array_equal(fos, found)
            assert as_.min() >= 0 and as_.max() < n_envs * U and np.array_equal(as_ % U, slot)
            assert np.array_equal(fos, plane.reshape(frames, n_envs * U)[fs, as_] != 0)
            if k == 0:
                assert np.array_equal(fs, fa) and np.array_equal(as_, aa)


def test_first_draw_is_uniform_on_tiny_rings():
    """The slot of draw 0 over 4 000 updates (counters (5 << 32) + k at one seed) of rings with D = 2 ... 33 stored rows, the sizes
    where the Feistel halves are one to three bits wide and the cycle-walk rejects up to half of its passes: every cell within
    4.5 sigma of N / D (binomial; the largest seen is 2.9 sigma).  The GPU tests assert equality with this oracle, so the law is
    tested here alone.  PAIRS of draws are not uniform on such rings -- at D = 5 (3 bits, la = 1) the ordered pair (draw 0, draw 1)
    is 7.9 sigma off: six rounds over 3 bits are not a uniform random permutation ("Random streams") -- and are not
    asserted."""
    N, seed = 4000, 0x1234567890
    for D in (2, 3, 5, 9, 17, 33):
        counters = (5 << 32) + np.arange(N, dtype=np.uint64)
        first = px.replay_slots(N, seed, counters, D, 1, positions=np.zeros(N, dtype=np.uint64))      # draw 0 of each update
        for k in range(0, N, 397):
            assert first[k] == px.replay_slots(1, seed, (5 << 32) + k, D, 1)[0]
        hits = np.bincount(first, minlength=D)
        assert hits.sum() == N and len(hits) == D
        sigma = np.sqrt(N * (1.0 / D) * (1.0 - 1.0 / D))
        assert np.abs(hits - N / D).max() <= 4.5 * sigma, (D, hits)


def test_u53_range_and_monotonicity():
    assert px.u53(0, 0) == 0.0
    assert px.u53(2 ** 32 - 1, 2 ** 32 - 1) == 1.0 - 2.0 ** -53
    assert px.u53(31, 63) == 0.0 and px.u53(32, 0) == 2.0 ** -27 and px.u53(0, 64) == 2.0 ** -53     # the low 5 / 6 bits are dropped
    a = np.sort(np.random.default_rng(0).integers(0, 2 ** 32, 4096, dtype=np.uint64))
    for b in (0, 12345, 2 ** 32 - 1):
        u = px.u53(a, b)
        assert (np.diff(u) >= 0).all() and u.min() >= 0.0 and u.max() < 1.0                          # monotone in a
        assert ((np.diff(u) > 0) == (np.diff(a >> np.uint64(5)) > 0)).all()                          # strictly, per 32 values of a


def _standard_normal(z, lanes):
    from scipy import stats
    z = z.reshape(-1)
    assert stats.kstest(z, "norm").pvalue > 1e-4
    for k in range(lanes):
        assert stats.kstest(z[k::lanes], "norm").pvalue > 1e-4, k
    assert abs(np.corrcoef(z[0::2], z[1::2])[0, 1]) < 0.01                                           # cosine against sine branch
    assert np.abs(z).max() <= np.sqrt(48.0 * np.log(2.0))


def test_randn_and_eval_noise_are_standard_normal():
    n = 1 << 20
    g = px.randn(n, seed=(7 << 32) | 11, counter=(3 << 32) | 5)
    _standard_normal(g.z, 4)
    assert g.u1.dtype == np.float32 and g.u2.dtype == np.float32 and g.t.dtype == np.float32
    assert g.u1.min() > 0.0 and g.u1.max() <= 1.0 and g.u2.min() >= 0.0 and g.u2.max() < 1.0
    assert np.array_equal(g.t, (px.TWO_PI_F32 * g.u2).astype(np.float32)) and float(px.TWO_PI_F32) == 6.2831854820251465
    assert abs(np.corrcoef(g.z[0::4], g.z[2::4])[0, 1]) < 0.01                                       # the two pairs of a quad
    e = px.eval_noise(1 << 12, 1 << 7, seed=(9 << 32) | 2)                                           # 2^19 blocks, 2^20 values
    assert e.z.shape == (1 << 12, 1 << 7, 2)
    _standard_normal(e.z, 2)
    # a shorter request is a prefix; another counter / seed is another stream, also where only the high halves differ
    assert np.array_equal(px.randn(1027, 5, 9).z, px.randn(4099, 5, 9).z[:1027])
    for other in (px.randn(64, 5, 9 + (1 << 32)), px.randn(64, 5 + (1 << 32), 9), px.randn(64, 5, 10)):
        assert not np.array_equal(other.z, px.randn(64, 5, 9).z)


def test_box_muller_extreme_value():
    """rad is largest at the smallest u1 = 2^-24 (first word < 256): sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.768..., and nowhere else."""
    top = np.sqrt(48.0 * np.log(2.0))
    lo = px.box_muller(np.array([0, 255, 256, 2 ** 32 - 1]), np.array([0, 0, 0, 0]))
    assert lo.u1[0, 0] == np.float32(2.0 ** -24) and lo.u1[1, 0] == lo.u1[0, 0] and lo.u1[2, 0] == np.float32(2.0 ** -23)
    assert lo.rad[0, 0] == top and lo.rad[1, 0] == top and lo.rad[2, 0] < top
    assert lo.u1[3, 0] == 1.0 and lo.rad[3, 0] == 0.0 and lo.z[0, 0] == top and lo.z[0, 1] == 0.0     # u2 = 0: cos 1, sin 0
    hi = px.box_muller(np.array([0]), np.array([2 ** 32 - 1]))
    assert hi.u2[0, 0] == np.float32(1.0 - 2.0 ** -24) and hi.t[0, 0] < px.TWO_PI_F32


def test_per_draws_are_stratified_and_clamped():
    for batch, total in ((1, 0.5), (3, 7.25), (256, 1000.75), (1000, 12345.0)):
        v = px.per_draws(batch, seed=(4 << 32) | 1, counter=(2 << 32) | 3, total=total)
        seg = np.floor(total) / batch
        i = np.arange(batch)
        assert v.dtype == np.float64 and (v >= seg * i).all() and (v <= seg * (i + 1)).all() and (v <= total).all()
    assert (px.per_draws(8, 1, 0, 0.25) == 0.0).all()                                               # int(total) = 0: every draw is 0
    assert not np.array_equal(px.per_draws(64, 1, 5, 99.0), px.per_draws(64, 1, 5 + (1 << 32), 99.0))


def test_reset_eval_and_planner_draws_ranges():
    for m in (1, 3, 1000):
        scn, h = px.reset_draws(4096, seed=(1 << 40) | 7, tick=(1 << 33) | 2, m=m)
        assert scn.min() >= 0 and scn.max() < m and len(np.unique(scn)) >= 0.95 * m    # (1000 rows: e^-4.096 = 1.7 % unseen)
        assert h.min() >= 0.0 and h.max() < px.TWO_PI
    assert not np.array_equal(px.reset_draws(64, 3, 5, 1000)[0], px.reset_draws(64, 3, 5 + (1 << 32), 1000)[0])
    h = px.eval_headings(4096, seed=5)
    assert h.min() >= 0.0 and h.max() < px.TWO_PI and abs(h.mean() - np.pi) < 0.1
    u, r = px.eval_eps_draws(512, 8, seed=5, n_actions=3)
    assert u.dtype == np.float32 and u.shape == (512, 8) and u.min() >= 0.0 and u.max() < 1.0
    assert set(np.unique(r).tolist()) == {0, 1, 2}
    s = px.rrt_stream(seed=11, scenario=3, attempt=0, length=4096)
    assert s.min() >= 0.0 and s.max() < 1.0 and abs(s.mean() - 0.5) < 0.03
    assert not np.array_equal(s, px.rrt_stream(11, 3, 1, 4096)) and not np.array_equal(s, px.rrt_stream(11, 4, 0, 4096))


def test_fourth_counter_word_separates_the_streams():
    """For counters / ticks below 2^32 the fourth counter word of every stream is its own constant: no two streams of one seed can
    ever share a Philox block.  Above 2^32 seven of the nine keep it (their high half sits in the third word or is absent); randn
    xors its constant INTO the counter's high half, so there it can take another stream's value.  The one aliasing that exists:
    randn at counter_hi == 0x6a55 ^ 0x0ac7 has the act stream's fourth word, and its quad q (< 2^32) then reads the block of
    act_draws(index q, counter = counter_lo << 32) -- first word and all."""
    idx = np.arange(5, dtype=np.uint64)
    small = 0xFFFFFFFF
    consts = {}
    for name in px.STREAMS:
        w = px.stream_counters(name, idx, small, 3)
        assert w.shape == (5, 4) and len(set(w[:, 3].tolist())) == 1
        consts[name] = int(w[0, 3])
    assert consts == px.STREAMS and len(set(consts.values())) == len(px.STREAMS) == 9
    big = (0x1234 << 32) | 9
    for name in px.STREAMS:
        w3 = int(px.stream_counters(name, idx, big, 3)[0, 3])
        assert w3 == (px.STREAMS[name] ^ 0x1234 if name == "randn" else px.STREAMS[name])
    # the aliasing, in numbers: u1 of randn's element 4 q is the act stream's u plus 2^-24
    c_lo = 0x00C0FFEE
    g = px.randn(4 * 64, seed=77, counter=((0x6A55 ^ 0x0AC7) << 32) | c_lo)
    u, _ = px.act_draws(64, seed=77, counter=c_lo << 32, n_actions=3)
    assert np.array_equal(g.u1[0::4], u + np.float32(2.0 ** -24))
    g2 = px.randn(4 * 64, seed=77, counter=c_lo)
    assert not np.array_equal(g2.u1[0::4], u + np.float32(2.0 ** -24))


def test_oracle_planner_stays_inside_the_stream_on_the_restated_draws():
    """The GPU test of the planner's stream leaves out rows whose plan does not fit (2 <= nodes <= K = 64) or that may have run past
    the RRT_LEN uniforms handed to the stream-fed mode, and allows at most 1/8 of them: the CPU planner on the same restated stream
    must stay inside that cap by itself (it plans 64 of 64).  With max_iter lowered some first attempts fail and fit on the
    attempt-1 stream: the second GPU case is not empty."""
    from conftest import load_golden
    from oracle import pyoracle as po
    world = po.OracleWorld(load_golden("world_stock.npz")["buildings"])

    def plan(u, max_iter):
        # UAV.reset: the heading draw first, then start (x, y) and goal (x, y) by random.uniform, then the planner's own draws
        start = [10.0 + (210.0 - 10.0) * u[1], 1.0 + (10.0 - 1.0) * u[2], 0.0]
        goal = [330.0 + (490.0 - 330.0) * u[3], 420.0 + (490.0 - 420.0) * u[4], 0.0]
        path, it = po.rrt_get_path(world, po.OracleRng(0).replay(u[5:]), start, goal, max_iter=max_iter)
        return path is not None and 2 <= len(path) <= 64 and 5 + 4 * it <= RRT_LEN

    fit = sum(plan(px.rrt_stream(RRT_SEED, r, 0, RRT_LEN), 10000) for r in range(RRT_ROWS))
    assert fit >= RRT_ROWS - RRT_ROWS // 8, fit
    second = sum(not plan(px.rrt_stream(RRT_SEED, r, 0, RRT_LEN), RRT_MAX_ITER_LOW) and plan(px.rrt_stream(RRT_SEED, r, 1, RRT_LEN), RRT_MAX_ITER_LOW)
                 for r in range(RRT_ROWS))
    assert second >= 8, second
