"""One DQN-family learner per UAV slot on the device: uavenv_dqn_act_slots (k_dqn_act_slots, csrc/learner.hip),
uavenv_replay_draw_slots (csrc/replay.hip), the UavDqnSlotsLoop of csrc/loop.hip (loop.DQNSlotsHotLoop) and the plugin path
<fused_slots>1</fused_slots> of plugins/PathPlan_City.py.

 - the act kernel against the existing one: index_out and q_out equal, as bytes, uavenv_dqn_act with net j on slot j's rows
   gathered contiguously under the key seed + j; U in {1, 2, 4}, 1 / 63 / 65 / 1000 envs, four heads, fresh and trained
   ("stress") weights, eps in {0, 0.3, 1}, with and without layer-1 images; 130 guard rows behind each output stay untouched;
   replacing net k changes rows = k (mod U) only;
 - the act kernel against float64 (oracle.dqn_act_ref.act_f64 / decide, oracle.philox.act_draws keyed (seed + j mod 2^64; e,
   counter, 0xac7)) at the bound tests/test_dqn_act_kernels_gpu.py applies to the packed f32-MFMA form (its check_a / check_b, by
   import), exact ties taking the first maximum included;
 - the draws against uavenv_replay_draw_valid / uavenv_replay_draw;
 - the loop against the composition of the entry points that existed before it (per slot: gather, uavenv_dqn_act, scatter; the
   step; the draws; per slot the update), bit for bit over 23 passes on a 9-frame ring, run(10) + run(13);
 - slot isolation, a federated merge between two runs, every refusal leaving the env alone, and the plugin path."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from dqn_fixtures import Pool, tie_rows
from oracle.dqn_act_ref import act_f64, steer_of
from oracle.philox import act_draws
from test_dqn_act_kernels_gpu import GUARD, Net, check_a, check_b, fresh_flat, stress_flat

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
HEADS = [(3, False), (3, True), (2, False), (4, False)]
PARAM = {"w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99", "Update_loop": "3"}


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.env.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def slot_flats(A, dueling, which, U):
    """U distinct parameter blocks of one head shape: fresh nets of different seeds, or the trained golden scaled per slot."""
    if which == "fresh":
        return [fresh_flat(A, dueling, 100 + 10 * A + int(dueling) + 7 * j) for j in range(U)]
    base = stress_flat(A, dueling)
    return [(base * np.float32(1.0 + j / 16.0)).astype(np.float32) for j in range(U)]


def net_array(nets):
    return (C.POINTER(_lib().UavDqnNet) * len(nets))(*[C.pointer(n.net) for n in nets])


def act_slots_raw(nets, obs, n_envs, eps, seed, counter, images=None, want_q=True, expect=0):
    """uavenv_dqn_act_slots (or its image form) into sentinel-filled outputs with GUARD rows behind the last agent."""
    L, U, A = _lib(), len(nets), nets[0].A
    N = n_envs * U
    idx = torch.full((N + GUARD,), -7, dtype=torch.int32, device="cuda")
    q = torch.full((N + GUARD, A), float("nan"), device="cuda") if want_q else None
    qp = None if q is None else q.data_ptr()
    lib = L.load()
    if images is None:
        rc = lib.uavenv_dqn_act_slots(net_array(nets), U, obs.data_ptr(), L.OBS_PACKED, n_envs, float(eps), seed, counter,
                                      idx.data_ptr(), qp, stream())
    else:
        imgs = (C.c_void_p * U)(*[t.data_ptr() for t in images])
        rc = lib.uavenv_dqn_act_slots_img(net_array(nets), U, obs.data_ptr(), L.OBS_PACKED, n_envs, float(eps), seed, counter,
                                          idx.data_ptr(), qp, imgs, stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    idx_h = idx.cpu().numpy()
    assert np.all(idx_h[N:] == -7), "index_out written past the last agent"
    q_h = None
    if q is not None:
        q_h = q.cpu().numpy()
        assert np.isnan(q_h[N:]).all(), "q_out written past the last agent"
        q_h = q_h[:N]
    return idx_h[:N], q_h


def act_per_slot(nets, obs, n_envs, eps, seed, counter):
    """The definition: per slot, uavenv_dqn_act with net j on rows j::U gathered contiguously, key seed + j -> by agent."""
    L, U, A = _lib(), len(nets), nets[0].A
    idx = np.zeros(n_envs * U, dtype=np.int32)
    q = np.zeros((n_envs * U, A), dtype=np.float32)
    for j, net in enumerate(nets):
        rows = obs[j::U].contiguous()
        i_j = torch.full((n_envs,), -7, dtype=torch.int32, device="cuda")
        q_j = torch.full((n_envs, A), float("nan"), device="cuda")
        assert L.load().uavenv_dqn_act(C.byref(net.net), rows.data_ptr(), L.OBS_PACKED, n_envs, float(eps), (seed + j) & M64, counter,
                                       i_j.data_ptr(), None, q_j.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        idx[j::U] = i_j.cpu().numpy()
        q[j::U] = q_j.cpu().numpy()
    return idx, q


@pytest.mark.parametrize("which", ["fresh", "stress"])
@pytest.mark.parametrize("A,dueling", HEADS, ids=lambda x: str(x))
@pytest.mark.parametrize("U", [1, 2, 4])
def test_act_slots_equals_the_act_kernel_per_slot(pool, U, A, dueling, which):
    nets = [Net(f, A, dueling, "f32") for f in slot_flats(A, dueling, which, U)]
    images = [n.image() for n in nets]
    packed = pool.ring.obs.view(-1, pool.ring.obs.shape[-1])
    rng = np.random.default_rng([U, A, int(dueling), which == "fresh"])
    greedy_seen = random_seen = 0
    for n_envs in (1, 63, 65, 1000):
        obs = packed[torch.tensor(rng.integers(0, packed.shape[0], n_envs * U), device="cuda")].contiguous()
        for k, eps in enumerate((0.0, 0.3, 1.0)):
            seed, counter = (0x9E37 << 32) | (17 * n_envs + U), ((n_envs % 7 + 1) << 32) | (5 * n_envs + k)
            want_i, want_q = act_per_slot(nets, obs, n_envs, eps, seed, counter)
            for imgs in (None, images):
                got_i, got_q = act_slots_raw(nets, obs, n_envs, eps, seed, counter, images=imgs)
                assert np.array_equal(got_i, want_i), (n_envs, eps, imgs is not None, np.flatnonzero(got_i != want_i)[:8])
                assert np.array_equal(got_q.view(np.uint32), want_q.view(np.uint32)), (n_envs, eps, imgs is not None)
            i2, _ = act_slots_raw(nets, obs, n_envs, eps, seed, counter, want_q=False)      # q_out is nullable
            assert np.array_equal(i2, want_i)
            if eps == 0.3 and n_envs == 1000:
                g = np.argmax(want_q, axis=1)
                greedy_seen, random_seen = int((want_i == g).sum()), int((want_i != g).sum())
    assert greedy_seen > 0 and random_seen > 0            # eps = 0.3 took both branches
    # replacing net k changes the rows of slot k only
    n_envs = 65
    obs = packed[torch.tensor(rng.integers(0, packed.shape[0], n_envs * U), device="cuda")].contiguous()
    _, q0 = act_slots_raw(nets, obs, n_envs, 0.0, 5, 6)
    for k in range(U):
        other = list(nets)
        other[k] = Net(fresh_flat(A, dueling, 999 + k), A, dueling, "f32")
        _, q1 = act_slots_raw(other, obs, n_envs, 0.0, 5, 6)
        same = (q0.view(np.uint32) == q1.view(np.uint32)).all(1)
        agent = np.arange(n_envs * U)
        assert same[agent % U != k].all() and not same[agent % U == k].any()


@pytest.mark.parametrize("which", ["fresh", "stress"])
@pytest.mark.parametrize("U,A,dueling", [(4, 3, False), (2, 3, True), (4, 2, False), (2, 4, False), (1, 3, False)])
def test_act_slots_against_float64_and_the_philox_oracle(pool, U, A, dueling, which):
    flats = slot_flats(A, dueling, which, U)
    nets = [Net(f, A, dueling, "f32") for f in flats]
    images = [n.image() for n in nets]
    rng = np.random.default_rng([7, U, A, int(dueling)])
    n_envs = 1000
    pick = rng.integers(0, len(pool.rows), n_envs * U)
    packed = pool.ring.obs.view(-1, pool.ring.obs.shape[-1])
    obs = packed[torch.tensor(pick, device="cuda")].contiguous()
    X = pool.rows[pick].astype(np.float64)
    key = "slots/%s" % ("4" if A + dueling <= 4 else "NMAX")
    # the second seed wraps: slot j's key is (seed + j) mod 2^64
    for k, (eps, seed) in enumerate(((-1.0, (0x51 << 32) | 11), (0.0, M64 - 1), (0.3, (0xABCD << 32) | 5), (1.0, M64))):
        counter = (3 << 32) | (40 + k)
        for imgs in (None, images):
            idx, q = act_slots_raw(nets, obs, n_envs, eps, seed, counter, images=imgs)
            for j in range(U):
                r = act_f64(X[j::U], flats[j], n_actions=A, dueling=dueling, eps=0.0, seed=0, counter=0)
                u, rnd = act_draws(n_envs, (seed + j) & M64, counter, A)
                check_a(key, q[j::U], r["Q"], r["q_abs"], say=False)
                check_b(idx[j::U].astype(np.int64), steer_of(idx[j::U], A).view(np.uint32), q[j::U], u, rnd, eps, A)
                if eps == 1.0:
                    assert np.array_equal(idx[j::U], rnd)


def test_act_slots_exact_ties_take_the_first_maximum(pool):
    rng = np.random.default_rng(8)
    n_envs, U = 200, 4
    pick = rng.integers(0, len(pool.rows), n_envs * U)
    packed = pool.ring.obs.view(-1, pool.ring.obs.shape[-1])
    obs = packed[torch.tensor(pick, device="cuda")].contiguous()
    X = pool.rows[pick].astype(np.float64)
    for A, dueling, pairs in ((3, False, [(0, 1), (1, 2), (0, 2), (0, 1)]), (3, True, [(0, 2), (0, 1), (1, 2), (0, 2)])):
        flats = [tie_rows(fresh_flat(A, dueling, 3 + A + j), A, dueling, a, b) for j, (a, b) in enumerate(pairs)]
        nets = [Net(f, A, dueling, "f32") for f in flats]
        idx, q = act_slots_raw(nets, obs, n_envs, -1.0, 77, 78)
        for j, (a, b) in enumerate(pairs):
            r = act_f64(X[j::U], flats[j], n_actions=A, dueling=dueling, eps=-1.0, seed=0, counter=0)
            check_a("slots/ties", q[j::U], r["Q"], r["q_abs"], say=False)
            qj = q[j::U]
            assert np.array_equal(qj[:, a].view(np.uint32), qj[:, b].view(np.uint32))
            assert np.all(qj.max(1) == qj[:, a]) and np.all(idx[j::U] == a), (A, dueling, j, a, b)


# ---- the draws ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("U,n_envs,batch,frames,head,filled", [(4, 200, 64, 9, 3, 8), (2, 200, 128, 9, 0, 5), (4, 37, 64, 5, 4, 1),
                                                               (1, 100, 64, 3, 1, 2)])
def test_draw_slots_equals_the_existing_draws(U, n_envs, batch, frames, head, filled):
    L = _lib()
    lib = L.load()
    rng = np.random.default_rng([U, n_envs, batch])
    total = U * batch
    seed, counter = (0x77 << 32) | 9, (2 << 32) | 31

    def run(fn, *args):
        out = torch.full((total + GUARD, 2), -7, dtype=torch.int32, device="cuda")
        assert fn(*args, out.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.all(o[total:] == -7)
        return o[:total]

    slot = np.arange(total) // batch
    # every stored row: uavenv_replay_draw over U * batch draws
    ref = run(lib.uavenv_replay_draw, frames, n_envs, head, filled, total, seed, counter)
    got = run(lib.uavenv_replay_draw_slots, frames, n_envs, head, filled, batch, U, None, L.DRAW_MAX_TRIES, seed, counter)
    assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 1], ref[:, 1] * U + slot)
    assert got[:, 1].min() >= 0 and got[:, 1].max() < n_envs * U
    # valid planes: all rows valid; random rows; whole finished slots (a slot with no valid row at all included)
    planes = [np.ones((frames, n_envs, U), dtype=np.uint8), (rng.random((frames, n_envs, U)) < 0.6).astype(np.uint8)]
    fin = (rng.random((frames, n_envs, U)) < 0.9).astype(np.uint8)
    fin[:, : n_envs // 2, U - 1] = 0
    fin[:, :, 0] = 0 if U > 1 else fin[:, :, 0]
    planes.append(fin)
    for k, plane in enumerate(planes):
        v = torch.tensor(plane.reshape(frames, n_envs * U), device="cuda").contiguous()
        ref = run(lib.uavenv_replay_draw_valid, frames, n_envs, head, filled, batch, U, U, 0, v.data_ptr(), L.DRAW_MAX_TRIES, seed,
                  counter)
        got = run(lib.uavenv_replay_draw_slots, frames, n_envs, head, filled, batch, U, v.data_ptr(), L.DRAW_MAX_TRIES, seed, counter)
        assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 1], ref[:, 1] * U + slot), k
        if k == 0:                                             # (a draw past the stored rows wraps in both forms: draw s mod D)
            all_rows = run(lib.uavenv_replay_draw_slots, frames, n_envs, head, filled, batch, U, None, L.DRAW_MAX_TRIES, seed, counter)
            assert np.array_equal(got, all_rows)
        if k == 1 and filled * n_envs >= 8 * total:            # enough tries: (almost) every draw found a valid row
            assert plane[got[:, 0], got[:, 1] // U, got[:, 1] % U].mean() > 0.95


# ---- the loop ----------------------------------------------------------------------------------------------------------------

def build(n_envs, U, net, kind, frames_cap=8, seeds=None):
    from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
    env = make_city26_env(n_envs, obs_dtype="packed", uav_per_env=U)
    ring = DeviceReplayRing(env, frames_cap * env.N, discrete=True)
    ring.reset(seed=12)
    Ls = []
    for j in range(U):
        torch.manual_seed(1 + j if seeds is None else seeds[j])
        Ls.append(FusedDQNLearner(dict(PARAM, NetWork=net), kind, device="cuda:0"))
    return env, ring, Ls


def compose(ring, Ls, passes, batch, seed, eps, auto_reset, skip_done, valid_draws, counter0=0, learn_start=0):
    """The passes as the entry points that existed before the slots loop give them: per slot a strided gather, uavenv_dqn_act under
    seed + j and a scatter; the step; the draws (over the valid rows or over every stored row) turned into (frame, agent) pairs;
    per slot learn_from_ring on its slice."""
    L = _lib()
    lib = L.load()
    U = len(Ls)
    n_envs = ring.env.N // U
    draws = torch.zeros((U * batch, 2), dtype=torch.int32, device="cuda")
    slot = (torch.arange(U * batch, device="cuda") // batch).to(torch.int32)
    for c in range(counter0, counter0 + passes):
        obs, act = ring.current_obs(), ring.current_action()
        for j, Lj in enumerate(Ls):
            a = torch.empty(n_envs, dtype=torch.int32, device="cuda")
            Lj.act(obs[j::U].contiguous(), eps, (seed + j) & M64, c, index_out=a)
            act[j::U] = a
        ring.step_env(auto_reset=auto_reset, skip_done=skip_done)
        if ring.filled * n_envs >= max(learn_start, batch):
            if valid_draws:
                rc = lib.uavenv_replay_draw_valid(ring.frames, n_envs, ring.head, ring.filled, batch, U, U, 0, ring.valid.data_ptr(),
                                                  L.DRAW_MAX_TRIES, seed + 7, c, draws.data_ptr(), stream())
            else:
                rc = lib.uavenv_replay_draw(ring.frames, n_envs, ring.head, ring.filled, U * batch, seed + 7, c, draws.data_ptr(),
                                            stream())
            assert rc == 0
            draws[:, 1] = draws[:, 1] * U + slot
            for j, Lj in enumerate(Ls):
                Lj.learn_from_ring(ring, batch, seed, c, explicit_idx=draws[j * batch:(j + 1) * batch].contiguous())


@pytest.mark.parametrize("U,batch,net,kind,mode", [(4, 64, "Qnet2", "dqn", "reset"), (4, 64, "Qnet2", "dqn", "skip"),
                                                  (2, 128, "Qnet2", "dqn", "reset"), (4, 64, "VAnet2", "ddqn", "reset"),
                                                  (2, 128, "VAnet2", "ddqn", "skip")])
def test_slots_loop_equals_the_composition(U, batch, net, kind, mode):
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    n_envs, passes, seed, eps = 200, 23, 9, 0.2
    kind = "dueling" if net == "VAnet2" else kind          # (VAnet2 goes with the dueling trainer: the double-DQN target)
    auto_reset, valid_draws, gate = (True, False, False) if mode == "reset" else (False, True, True)
    env_a, ring_a, La = build(n_envs, U, net, kind)
    assert ring_a.frames == 9 and env_a.N == n_envs * U
    compose(ring_a, La, passes, batch, seed, eps, auto_reset, True, valid_draws)
    env_b, ring_b, Lb = build(n_envs, U, net, kind)
    for a, b in zip(La, Lb):
        assert a.epoch > 0 and b.epoch == 0 and not torch.equal(a.flat[0], b.flat[0])
    loop = DQNSlotsHotLoop(ring_b, Lb, batch, seed=seed, eps=eps, auto_reset=auto_reset, skip_done=True, gate_updates=gate,
                           valid_draws=valid_draws)
    loop.run(10)
    assert loop.in_sync(batch) and not loop.in_sync(batch + 64)
    loop.run(passes - 10)
    torch.cuda.synchronize()
    assert (ring_b.head, ring_b.filled, loop.counter) == (ring_a.head, ring_a.filled, passes)
    assert [x.epoch for x in Lb] == [x.epoch for x in La] and La[0].epoch == passes
    for name in ("obs", "action", "reward", "done", "valid"):
        assert torch.equal(getattr(ring_a, name), getattr(ring_b, name)), name
    for j, (a, b) in enumerate(zip(La, Lb)):
        assert torch.equal(a.flat, b.flat), j
        assert float(a.loss) == float(b.loss) and np.isfinite(float(b.loss)), j
    assert len({float(x.flat[0].sum()) for x in Lb}) == U          # the slots learnt different things
    assert len(torch.unique(ring_b.action)) == 3
    loop.close()
    env_a.close()
    env_b.close()


def test_slots_do_not_interact():
    """Agents of one env do not interact: slot 0's parameters after a run are the same whether slot 1 starts from weights A or B."""
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    out = []
    for s1 in (2, 31):
        env, ring, Ls = build(200, 2, "Qnet2", "dqn", seeds=[1, s1])
        loop = DQNSlotsHotLoop(ring, Ls, 64, seed=4, eps=0.2)
        loop.run(12)
        torch.cuda.synchronize()
        out.append((Ls[0].flat.clone(), Ls[1].flat.clone(), float(Ls[0].loss)))
        loop.close()
        env.close()
    assert torch.equal(out[0][0], out[1][0]) and out[0][2] == out[1][2]
    assert not torch.equal(out[0][1][0], out[1][1][0])


def test_a_federated_merge_between_two_runs_reaches_the_next_pass():
    """federated_learning_q replaces every q_local between two runs: the next pass acts with the MERGED weights (the loop rebuilds
    its layer-1 images when a run starts), not with the images of its own last Adam launches."""
    from dqn_based_uav_3d_path_planer_amd import federated
    from dqn_based_uav_3d_path_planer_amd.learner import act_slots
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop

    class T:
        fused = True

        def __init__(self, L):
            self.learner, self.q_local = L, L.q_local

    env, ring, Ls = build(200, 4, "Qnet2", "dqn")
    loop = DQNSlotsHotLoop(ring, Ls, 64, seed=4, eps=0.1)
    loop.run(6)
    torch.cuda.synchronize()
    before = [L.flat[0].clone() for L in Ls]
    assert federated.federated_learning_q([T(L) for L in Ls], "mean") == "device"
    torch.cuda.synchronize()
    assert all(torch.equal(L.flat[0], Ls[0].flat[0]) for L in Ls) and not torch.equal(Ls[0].flat[0], before[0])
    t, c = ring.head, loop.counter
    want = torch.full((env.N,), -7, dtype=torch.int32, device="cuda")
    act_slots(Ls, ring.obs[t], 0.1, 4, c, want)
    stale = torch.full((env.N,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    loop.run(1)
    torch.cuda.synchronize()
    assert torch.equal(ring.action[t], want)
    # (the check can tell: the weights before the merge act differently somewhere)
    for L, w in zip(Ls, before):
        keep = L.flat[0].clone()
        L.flat[0].copy_(w)
        w.copy_(keep)
    act_slots(Ls, ring.obs[t], 0.1, 4, c, stale)
    torch.cuda.synchronize()
    assert not torch.equal(stale, want)
    loop.close()
    env.close()


def good_cfg(ring, Ls, batch, keep):
    L = _lib()
    cfg = L.UavDqnSlotsLoopConfig()
    cfg.env, cfg.ring = ring.env._h, ring._c
    draws = torch.zeros((len(Ls) * batch, 2), dtype=torch.int32, device="cuda")
    keep.append(draws)
    cfg.draws_dev = draws.data_ptr()
    cfg.n_slots, cfg.batch, cfg.head, cfg.filled = len(Ls), batch, ring.head, ring.filled
    cfg.kind, cfg.huber, cfg.update_loop, cfg.learn_start = 0, 0, 3, 0
    cfg.step_flags = L.STEP_AUTO_RESET | L.STEP_SKIP_DONE
    cfg.seed, cfg.counter = 3, 0
    cfg.eps, cfg.gamma, cfg.lr, cfg.beta1, cfg.beta2, cfg.adam_eps = 0.1, 0.99, 1e-3, 0.9, 0.999, 1e-8
    for j, Lj in enumerate(Ls):
        cfg.slot[j].net = Lj.net
        p = Lj.new_partials(batch)
        keep.append(p)
        cfg.slot[j].partials_dev, cfg.slot[j].loss_dev, cfg.slot[j].epoch = p.data_ptr(), Lj.loss.data_ptr(), 0
    return cfg


def test_refusals_leave_the_env_alone(pool):
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    L = _lib()
    lib = L.load()
    env, ring, Ls = build(64, 2, "Qnet2", "dqn")
    torch.cuda.synchronize()

    def snap():
        torch.cuda.synchronize()
        st = env.get_state(0, env.N, want_sub=True)
        return [np.asarray(x).tobytes() for x in st], int(lib.uavenv_tick(env._h)), ring.obs.clone(), ring.action.clone()

    s0 = snap()
    E = L.EINVAL
    obs = ring.current_obs()
    idx = torch.full((env.N,), -7, dtype=torch.int32, device="cuda")
    nets = [Net(fresh_flat(3, False, 5 + j), 3, False, "f32") for j in range(2)]

    def act(ns, n_nets=None, dtype=L.OBS_PACKED, n_envs=64, o=None):
        arr = (C.POINTER(L.UavDqnNet) * max(len(ns), 1))(*[None if n is None else C.pointer(n.net) for n in ns])
        return lib.uavenv_dqn_act_slots(arr, len(ns) if n_nets is None else n_nets, (obs if o is None else o).data_ptr(), dtype,
                                        n_envs, 0.1, 1, 2, idx.data_ptr(), None, stream())

    assert act(nets) == 0
    torch.cuda.synchronize()
    assert (idx >= 0).all()
    idx.fill_(-7)
    assert act(nets, n_nets=0) == E and act([nets[0]] * 9) == E                              # 1 .. 8 nets
    assert lib.uavenv_dqn_act_slots(None, 2, obs.data_ptr(), L.OBS_PACKED, 64, 0.1, 1, 2, idx.data_ptr(), None, stream()) == E
    assert act([nets[0], None]) == E                                                         # a NULL net
    assert act(nets, dtype=L.OBS_F32) == E and act(nets, dtype=L.OBS_F16) == E               # packed rows only
    assert act([nets[0], Net(fresh_flat(3, False, 1), 3, False, "f16")]) == E                # an f16-MFMA net
    assert act([nets[0], Net(fresh_flat(4, False, 1), 4, False, "f32")]) == E                # n_actions differ
    assert act([nets[0], Net(fresh_flat(3, True, 1), 3, True, "f32")]) == E                  # dueling differs
    for A, d in ((15, False), (14, True), (1, False)):                                       # heads uavenv_dqn_act refuses
        bad = Net(np.zeros(6464 + (A + d) * 65, dtype=np.float32), A, d, "f32")
        assert act([bad, bad]) == E
    off = Net(fresh_flat(3, False, 2), 3, False, "f32")
    off.net.local = off.net.local + 4                                                        # a misaligned `local`
    assert act([nets[0], off]) == E
    assert act(nets, n_envs=0) == E and act(nets, n_envs=-3) == E
    assert lib.uavenv_dqn_act_slots(net_array(nets), 2, obs.data_ptr(), L.OBS_PACKED, 64, 0.1, 1, 2, None, None, stream()) == E
    torch.cuda.synchronize()
    assert (idx == -7).all()                                                                 # nothing was enqueued

    out = torch.full((2 * 64 + 8, 2), -7, dtype=torch.int32, device="cuda")

    def draw(frames=9, n_envs=64, head=2, filled=3, batch=64, U=2, valid=None, tries=8, o=out):
        return lib.uavenv_replay_draw_slots(frames, n_envs, head, filled, batch, U, valid, tries, 1, 2,
                                            None if o is None else o.data_ptr(), stream())

    assert draw() == 0
    torch.cuda.synchronize()
    assert (out[:128] >= 0).all() and (out[128:] == -7).all()
    out.fill_(-7)
    for kw in (dict(frames=1), dict(n_envs=0), dict(head=-1), dict(head=9), dict(filled=0), dict(filled=9), dict(batch=0),
               dict(U=0), dict(o=None), dict(valid=ring.valid.data_ptr(), tries=0)):
        assert draw(**kw) == E, kw
    torch.cuda.synchronize()
    assert (out == -7).all()

    keep = []
    h = C.c_void_p()

    def create(mut):
        cfg = good_cfg(ring, Ls, 64, keep)
        mut(cfg)
        hh = C.c_void_p()
        rc = lib.uavenv_dqn_slots_loop_create(C.byref(cfg), C.byref(hh))
        if rc == 0:
            lib.uavenv_dqn_slots_loop_destroy(hh)
        return rc

    assert create(lambda c: None) == 0
    f16 = FusedDQNLearner(dict(PARAM, NetWork="Qnet2"), "dqn", device="cuda:0", mfma="f16")
    four = FusedDQNLearner(dict(PARAM, NetWork="Qnet2", output="4"), "dqn", device="cuda:0")
    muts = {
        "no env": lambda c: setattr(c, "env", None),
        "n_slots 0": lambda c: setattr(c, "n_slots", 0),
        "n_slots 9": lambda c: setattr(c, "n_slots", 9),
        "n_slots does not divide N": lambda c: setattr(c, "n_slots", 3),
        "f32 rows": lambda c: setattr(c.ring, "obs_dtype", L.OBS_F32),
        "continuous ring": lambda c: setattr(c.ring, "action_is_index", 0),
        "another N": lambda c: setattr(c.ring, "n_agents", 64),
        "two frames": lambda c: setattr(c.ring, "frames", 2),
        "batch 65": lambda c: setattr(c, "batch", 65),
        "no draws": lambda c: setattr(c, "draws_dev", None),
        "head": lambda c: setattr(c, "head", 9),
        "filled": lambda c: setattr(c, "filled", 9),
        "update_loop 0": lambda c: setattr(c, "update_loop", 0),
        "valid draws without a valid plane": lambda c: (setattr(c, "valid_draws", 1), setattr(c.ring, "valid", None)),
        "f16 MFMA": lambda c: setattr(c.slot[1], "net", f16.net),
        "another head": lambda c: setattr(c.slot[1], "net", four.net),
        "no target": lambda c: setattr(c.slot[0].net, "target", None),
        "no partials": lambda c: setattr(c.slot[1], "partials_dev", None),
        "one net twice": lambda c: setattr(c.slot[1], "net", c.slot[0].net),
        "negative epoch": lambda c: setattr(c.slot[0], "epoch", -1),
    }
    for name, mut in muts.items():
        assert create(mut) == E, name
    assert lib.uavenv_dqn_slots_loop_create(None, C.byref(h)) == E
    assert lib.uavenv_dqn_slots_loop_run(None, 1, stream()) == E and lib.uavenv_dqn_slots_loop_set_eps(None, 0.1) == E
    assert lib.uavenv_dqn_slots_loop_get(None, C.byref(L.UavDqnSlotsLoopCursor())) == E
    cfg = good_cfg(ring, Ls, 64, keep)
    assert lib.uavenv_dqn_slots_loop_create(C.byref(cfg), C.byref(h)) == 0
    assert lib.uavenv_dqn_slots_loop_run(h, -1, stream()) == E
    assert lib.uavenv_dqn_slots_loop_run(h, 0, stream()) == 0                                 # zero passes: nothing happens
    cur = L.UavDqnSlotsLoopCursor()
    assert lib.uavenv_dqn_slots_loop_get(h, C.byref(cur)) == 0
    assert (cur.head, cur.filled, cur.counter, list(cur.epoch)) == (ring.head, ring.filled, 0, [0] * 8)
    assert lib.uavenv_dqn_slots_loop_destroy(h) == 0 and lib.uavenv_dqn_slots_loop_destroy(None) == 0
    s1 = snap()
    assert s1[0] == s0[0] and s1[1] == s0[1] and torch.equal(s1[2], s0[2])
    env.close()


def test_rollout_only_learn_start_and_set_eps():
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    env, ring, Ls = build(128, 2, "Qnet2", "dqn", frames_cap=16)
    w0 = [L.flat.clone() for L in Ls]
    loop = DQNSlotsHotLoop(ring, Ls, 128, seed=3, eps=1.0, learn_start=5 * 128)
    loop.run(4)                                    # 4 x 128 transitions per slot < learn_start
    torch.cuda.synchronize()
    assert [L.epoch for L in Ls] == [0, 0] and all(torch.equal(L.flat, w) for L, w in zip(Ls, w0))
    loop.set_eps(0.0)
    t = ring.head
    loop.run(3)                                    # updates at filled = 5, 6, 7
    torch.cuda.synchronize()
    assert [L.epoch for L in Ls] == [3, 3] and not any(torch.equal(L.flat[0], w[0]) for L, w in zip(Ls, w0))
    q = [L.q_values(torch.tensor(np.zeros((1, 100), dtype=np.float32), device="cuda")) for L in Ls]
    assert all(torch.isfinite(x).all() for x in q)
    loop.close()
    roll = DQNSlotsHotLoop(ring, Ls, 0, seed=3)    # batch 0: rollout only
    w1 = [L.flat.clone() for L in Ls]
    roll.run(5)
    torch.cuda.synchronize()
    assert [L.epoch for L in Ls] == [3, 3] and all(torch.equal(L.flat, w) for L, w in zip(Ls, w1)) and ring.filled == 12
    assert t < ring.head
    roll.close()
    env.close()


# ---- the plugin --------------------------------------------------------------------------------------------------------------

def _config(tmp_path, fused_slots, **env_tags):
    from dqn_based_uav_3d_path_planer_amd import driver
    xml = driver.make_config_dir(str(tmp_path), "DQN", num_envs=256, num_uav=4)
    s = open(xml).read()
    tags = dict(env_tags)
    if fused_slots is not None:
        tags["fused_slots"] = fused_slots
    for k, v in tags.items():
        if re.search(rf"<{k}>[^<]*</{k}>", s):
            s = re.sub(rf"<{k}>[^<]*</{k}>", f"<{k}>{v}</{k}>", s)
        else:
            s = s.replace("<seed>42</seed>", f"<seed>42</seed>\n        <{k}>{v}</{k}>")
    open(xml, "w").write(s)
    return xml


def test_plugin_fused_slots_episode(tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver
    monkeypatch.chdir(tmp_path)
    env = driver.simulator(_config(tmp_path, 1)).env
    assert env is not None and env.fast_slots and not env.fast and not env.fast_sac and env.backend.packed
    e0 = [u.Trainer.epoch for u in env.Agents]
    res = env.run_eposide(0.5)
    assert env.Check_uav_Done() and res["lose"] + res["success"] >= 256 * 4
    assert env.steps_last_episode > 100 and 1 <= env.surplus_passes_last_episode <= env.done_check
    for u, e in zip(env.Agents, e0):
        assert u.Trainer.epoch > e + 100 and np.isfinite(float(u.Trainer.learner.loss))
        assert len(u.Trainer.replay_memory) > 0
    assert np.isfinite(float(res["loss"]))
    w = [u.Trainer.learner.flat[0] for u in env.Agents]
    assert all(not torch.equal(w[0], x) for x in w[1:])                      # one learner per slot, each on its own rows
    res2 = env.run_eposide(0.3)                                                # a second episode goes on from the first
    assert env.Check_uav_Done() and all(u.Trainer.epoch > e + 200 for u, e in zip(env.Agents, e0)) and np.isfinite(float(res2["loss"]))


def test_plugin_fused_slots_federated_merge(tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver
    monkeypatch.chdir(tmp_path)
    env = driver.simulator(_config(tmp_path, 1, Is_FL=1, FL_Loop=1, FL_Aggregate="mean")).env
    assert env is not None and env.fast_slots and env.Is_FL == 1 and env.FL_Loop == 1 and env.FL_Aggregate == "mean"
    env.run_eposide(0.5)
    w = [u.Trainer.learner.flat[0] for u in env.Agents]
    assert env.fl_merges == 1 and env.fl_merged_on == "device" and all(torch.equal(w[0], x) for x in w[1:])
    env.run_eposide(0.5)                                                       # the merged weights are what the next episode acts with
    assert env.fl_merges == 2 and env.Check_uav_Done()


def test_plugin_without_the_tag_is_the_general_path(tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver
    monkeypatch.chdir(tmp_path)
    xml = _config(tmp_path, None)
    s = open(xml).read().replace("<num_envs>256</num_envs>", "<num_envs>32</num_envs>")
    open(xml, "w").write(s)
    env = driver.simulator(xml).env
    assert env is not None and not env.fast_slots and not env.fast and not env.backend.packed and env._ring is None
    torch.manual_seed(0)
    res = env.run_eposide(0.5)
    assert env.Check_uav_Done() and res["lose"] + res["success"] >= 32 * 4
    assert all(u.Trainer.epoch > 100 for u in env.Agents)
    # asked for, but unqualified (a batch the fused kernels do not take): the general path, nothing fails later
    d2 = tmp_path / "b"
    d2.mkdir()
    monkeypatch.chdir(d2)
    xml = _config(d2, 1)
    s = open(xml).read().replace("<num_envs>256</num_envs>", "<num_envs>32</num_envs>")
    open(xml, "w").write(s)
    t = d2 / "config" / "Trainer.xml"
    ts, n = re.subn(r"<Batch_Size>64</Batch_Size>", "<Batch_Size>100</Batch_Size>", t.read_text())
    assert n == 1
    t.write_text(ts)
    env = driver.simulator(xml).env
    assert env is not None and not env.fast_slots and not env.backend.packed
    torch.manual_seed(0)
    env.run_eposide(0.5)
    assert env.Check_uav_Done() and all(u.Trainer.epoch > 100 for u in env.Agents)
