"""Shared by tests/test_replay_draw_kernels_gpu.py: hand-built replay rings whose rows say which (frame, agent) they are, and the
checks every set of uniform replay draws is put through.  The checks take plain numpy arrays, so the same functions judge what
a kernel returned (the GPU tests) and what a deliberately wrong restatement returns (the host-only mutation tests): every check
raises AssertionError with its NAME in front, which is what the mutation tests match on.

Ring rows (RowRing): the observation row of (frame f, agent a) is `words` int32 values (row * 128 + column), row = f * n_agents + a
-- 100 words stand for an f32 row, 50 for an f16 row, 20 for a packed row; the gather copies bytes, so any bit pattern will do and
a wrong row is readable from the first word it returns.  action = row ^ 0x5a5a5a, reward = row + 0.25, done = row % 3 == 0,
valid = row % 5 != 0."""
import numpy as np

from oracle import philox as px

GUARD = 130                      # sentinel rows behind every output
WORDS = {"f32": 100, "f16": 50, "packed": 20}


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


# ---- the checks --------------------------------------------------------------------------------------------------------------

def check_stored_rows(f, a, head, filled, frames, n_agents):
    """Every (frame, agent) names a stored row: an agent of the ring, 1 .. filled frames behind head."""
    f, a = np.asarray(f, dtype=np.int64), np.asarray(a, dtype=np.int64)
    assert a.min() >= 0 and a.max() < n_agents, "stored-row: agent outside the ring"
    assert f.min() >= 0 and f.max() < frames, "stored-row: frame outside the ring"
    back = (head - 1 - f) % frames
    assert back.max() < filled, "stored-row: a frame that is not 1 .. filled behind head"
    return back


def check_draw(f, a, want, head, filled, frames, n_agents):
    """uavenv_replay_draw's output for `batch` draws: stored rows; the first D a permutation of all D stored rows; draw s >= D the
    row of draw s - D; and equal to the oracle's pairs `want`."""
    D, batch = filled * n_agents, len(f)
    back = check_stored_rows(f, a, head, filled, frames, n_agents)
    slot = back * n_agents + np.asarray(a, dtype=np.int64)
    k = min(batch, D)
    assert len(np.unique(slot[:k])) == k, "permutation: a row drawn twice"
    if batch > D:
        assert np.array_equal(slot[D:], slot[:batch - D]), "wrap: draw s >= D is not draw s - D"
    assert np.array_equal(f, want[0]) and np.array_equal(a, want[1]), "oracle: not the oracle's rows"


def check_valid_draw(f, e, want, plane, batch, n_slots, U, first_slot, head, filled, frames, n_envs):
    """uavenv_replay_draw_valid's output: stored rows; distinct within a slot among the draws that hold a valid row while
    batch <= D; a valid row wherever the oracle found one and an invalid one elsewhere; equal to the oracle's (frame, env, found)."""
    S, D = batch * n_slots, filled * n_envs
    assert len(f) == len(e) == S, "length: not n_slots * batch pairs"
    back = check_stored_rows(f, e, head, filled, frames, n_envs)
    slot = first_slot + np.arange(S) // batch
    ok = np.asarray(plane).reshape(frames, n_envs, U)[f, e, slot] != 0
    if batch <= D:
        for j in range(n_slots):
            m = (slot == first_slot + j) & ok
            assert len(np.unique(back[m] * n_envs + e[m])) == m.sum(), "distinct: a valid row twice in one slot"
    assert np.array_equal(ok, want[2]), "found: the returned row's valid flag is not the oracle's"
    assert np.array_equal(f, want[0]) and np.array_equal(e, want[1]), "oracle: not the oracle's rows"


# ---- rings -------------------------------------------------------------------------------------------------------------------

class RowRing:
    """A UavReplayRing of torch tensors, frames x n_agents, whose rows encode (frame, agent) as the module docstring says."""

    def __init__(self, kind, frames, n_agents, with_valid=True):
        import torch
        L = _lib()
        self.kind, self.frames, self.n = kind, frames, n_agents
        w = WORDS[kind]
        row = np.arange(frames * n_agents, dtype=np.int64).reshape(frames, n_agents)
        self.h_obs = (row[:, :, None] * 128 + np.arange(w)[None, None, :]).astype(np.int32)
        self.h_action = (row ^ 0x5A5A5A).astype(np.int32)
        self.h_reward = (row + 0.25).astype(np.float32)
        self.h_done = (row % 3 == 0).astype(np.uint8)
        self.h_valid = (row % 5 != 0).astype(np.uint8)
        self.obs, self.action, self.reward, self.done, self.valid = (torch.tensor(x).cuda().contiguous() for x in
                                                                     (self.h_obs, self.h_action, self.h_reward, self.h_done,
                                                                      self.h_valid))
        code = {"packed": L.OBS_PACKED, "f16": L.OBS_F16, "f32": L.OBS_F32}[kind]
        self._c = L.UavReplayRing(self.obs.data_ptr(), self.action.data_ptr(), self.reward.data_ptr(), self.done.data_ptr(),
                                  self.valid.data_ptr() if with_valid else None, frames, n_agents, code, 1)
        self.with_valid = with_valid


class FloatRing:
    """A ring of packed-representable float observation rows (values in [-1, 1), 0 / 1 flags, zero pad columns) stored as `kind`,
    with actions below n_actions, rewards, done and valid flags: what a gradient kernel can learn from."""

    def __init__(self, kind, frames, n_agents, n_actions, head, filled, seed):
        import torch
        from conftest import pack_obs_rows
        L = _lib()
        rng = np.random.default_rng(seed)
        rows = np.zeros((frames * n_agents, 100), dtype=np.float32)
        rows[:, :11] = rng.uniform(-1.0, 1.0, (len(rows), 11))
        rows[:, 11:86] = rng.random((len(rows), 75)) < 0.3
        rows[:, 86:90] = rng.uniform(-1.0, 1.0, (len(rows), 4))
        rows[:, 90:95] = rng.random((len(rows), 5)) < 0.5
        if kind == "packed":
            obs = torch.tensor(pack_obs_rows(rows).reshape(frames, n_agents, 20))
        else:
            obs = torch.tensor(rows.reshape(frames, n_agents, 100))
            obs = obs.half() if kind == "f16" else obs
        shape = (frames, n_agents)
        self.obs = obs.cuda().contiguous()
        self.action = torch.tensor(rng.integers(0, n_actions, shape).astype(np.int32)).cuda()
        self.reward = torch.tensor(rng.normal(-3.0, 5.0, shape).astype(np.float32)).cuda()
        self.done = torch.tensor((rng.random(shape) < 0.2).astype(np.uint8)).cuda()
        self.valid = torch.tensor((rng.random(shape) >= 0.1).astype(np.uint8)).cuda()
        code = {"packed": L.OBS_PACKED, "f16": L.OBS_F16, "f32": L.OBS_F32}[kind]
        self._c = L.UavReplayRing(self.obs.data_ptr(), self.action.data_ptr(), self.reward.data_ptr(), self.done.data_ptr(),
                                  self.valid.data_ptr(), frames, n_agents, code, 1)
        self.frames, self.n, self.head, self.filled = frames, n_agents, head, filled


def sample(ring, head, filled, batch, seed, counter, want_valid=True, expect=0):
    """uavenv_replay_sample into sentinel-filled outputs with GUARD rows behind the batch -> dict of numpy arrays (the batch rows),
    after asserting that nothing behind them was written."""
    import ctypes as C
    import torch
    L = _lib()
    w = WORDS[ring.kind]
    n = batch + GUARD
    obs = torch.full((n, w), -7, dtype=torch.int32, device="cuda")
    nxt = torch.full((n, w), -7, dtype=torch.int32, device="cuda")
    act = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    rew, done, valid = (torch.full((n,), -7.0, dtype=torch.float32, device="cuda") for _ in range(3))
    rc = L.load().uavenv_replay_sample(C.byref(ring._c), head, filled, batch, seed, counter, obs.data_ptr(), nxt.data_ptr(),
                                       act.data_ptr(), rew.data_ptr(), done.data_ptr(), valid.data_ptr() if want_valid else None,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in dict(obs=obs, next=nxt, action=act, reward=rew, done=done, valid=valid).items()}
    for k, v in out.items():
        assert np.all(v[batch:] == -7), "%s written past the batch" % k
    if not want_valid:
        assert np.all(out["valid"] == -7), "valid_b written though NULL was passed"
    return {k: v[:batch] for k, v in out.items()}


def check_sample(out, ring, f, a, want_valid=True):
    """Every returned row is, bit for bit, the ring's row at (f, a) -- next-obs at ((f + 1) mod frames, a)."""
    fn = (f + 1) % ring.frames
    assert np.array_equal(out["obs"][:, 0] // 128, f * ring.n + a), "gather: obs rows are other rows than (f, a)"
    assert np.array_equal(out["obs"], ring.h_obs[f, a]), "gather: obs bytes"
    assert np.array_equal(out["next"][:, 0] // 128, fn * ring.n + a), "gather: next-obs rows are other rows than (f + 1, a)"
    assert np.array_equal(out["next"], ring.h_obs[fn, a]), "gather: next-obs bytes"
    assert np.array_equal(out["action"], ring.h_action[f, a]), "gather: action"
    assert np.array_equal(out["reward"].view(np.uint32), ring.h_reward[f, a].view(np.uint32)), "gather: reward"
    assert np.array_equal(out["done"], ring.h_done[f, a].astype(np.float32)), "gather: done"
    if want_valid:
        want = ring.h_valid[f, a].astype(np.float32) if ring.with_valid else np.ones(len(f), dtype=np.float32)
        assert np.array_equal(out["valid"], want), "gather: valid"


def draw_raw(fn, total, *args, expect=0):
    """A draw entry point into a sentinel-filled (total + GUARD) x 2 output -> the first `total` pairs as int64 numpy."""
    import torch
    out = torch.full((total + GUARD, 2), -7, dtype=torch.int32, device="cuda")
    rc = fn(*args, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    o = out.cpu().numpy().astype(np.int64)
    if expect != 0:
        assert np.all(o == -7), "a refused call wrote its output"
        return None
    assert np.all(o[total:] == -7), "pairs written past the last draw"
    return o[:total]


def factorisations(D):
    """D = filled x n_agents with n_agents in {1, 3, a power of two, a prime}: every such n_agents that divides D."""
    ns = {1}
    if D % 3 == 0:
        ns.add(3)
    p2 = D & -D
    if p2 > 1:
        ns.update({2, p2})
    d, m = 2, D
    while d * d <= m:
        while m % d == 0:
            ns.add(d)
            m //= d
        d += 1
    if m > 1:
        ns.add(m)
    return sorted(ns)


_SLOTS = {}


def oracle_draws(batch, seed, counter, head, filled, frames, n_agents):
    """px.replay_draws, the permutation computed once per (D, n_agents, seed, counter) and shared among heads and ring lengths."""
    key = (filled * n_agents, n_agents, seed, counter)
    if key not in _SLOTS or len(_SLOTS[key]) < batch:
        _SLOTS[key] = px.replay_slots(batch, seed, counter, filled, n_agents)
        _SLOTS[key].setflags(write=False)
    return px.slots_to_rows(_SLOTS[key][:batch], head, frames, n_agents)
