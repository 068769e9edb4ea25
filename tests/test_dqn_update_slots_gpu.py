"""Every UAV slot's DQN update in one gradient and one Adam launch (k_dqn_grad_slots, k_dqn_reduce_adam_slots of
csrc/learner.hip; uavenv_dqn_grad_slots, uavenv_dqn_reduce_adam_slots and their image forms; learner.update_slots; the
multi_update mode of loop.DQNSlotsHotLoop), held to the per-slot launches they replace:

 - the gradient, bit for bit: every row of partials[j] equals, as uint32, the row uavenv_dqn_grad_img writes with net j on slot
   j's pairs -- U in {1, 2, 4}, four heads, dqn / ddqn, both losses, fresh and trained ("stress") weights, with an image for
   every slot (LDS-DMA staging), for none and for some; batches 64 (one workgroup per slot), 128, and 64 x 258 (more tiles than
   workgroups: the persistent loop).  Pairs come from a hand ring with invalid rows.  Guard rows behind every partial buffer
   stay untouched; replacing net k changes partials[k] only;
 - the gradient against float64: each slot's raw bucket (uavenv_dqn_reduce of its rows) against oracle.dqn_grad_ref.dqn_grad_f64
   with the F32 constants and check_a of tests/test_dqn_grad_kernels_gpu.py, unchanged (the slots form has no |TD| output: the
   per-sample |TD error| that check also looks at comes from the single-net launch of the same inputs, whose rows the slots
   form equals bit for bit);
 - reduce + Adam, bit for bit against U calls of uavenv_dqn_reduce_adam_img: parameters, target, moments, loss, raw, images --
   update counts that differ per slot (hard copies in some slots only), the gate matching and not, 1 / 2 / 256 partial rows;
 - learner.update_slots against learn_from_ring per learner over three updates;
 - the loop with multi_update against the composition of the entry points (tests/test_dqn_slots_loop_gpu.py's compose), the
   setter toggled between runs, a federated merge between runs, and the gate with every agent finished."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_dqn_grad_kernels_gpu as G
from oracle.dqn_grad_ref import dqn_grad_f64
from test_dqn_act_kernels_gpu import Net, fresh_flat
from test_dqn_slots_loop_gpu import HEADS, build, compose, net_array, slot_flats, stream

pytestmark = pytest.mark.gpu

GUARD = 3                    # rows behind a partial buffer that must stay as they were
SENTINEL = 0x7FC0BEEF        # a NaN no kernel produces


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


@pytest.fixture(scope="module", autouse=True)
def _release_pool():
    """The row pool (shared with tests/test_dqn_grad_kernels_gpu.py, which has let go of it by now) lives for this module only."""
    yield
    if G._POOL is not None:
        G._POOL.env.close()
        G._POOL = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def make_nets(A, dueling, which, U):
    """U nets of one head shape whose q_target differs from q_local (a scaled copy: the TD target is not the net's own value)."""
    nets = [Net(f, A, dueling, "f32") for f in slot_flats(A, dueling, which, U)]
    for j, n in enumerate(nets):
        n.buf[1].mul_(1.0 + (j + 1) / 64.0)
    return nets


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def new_parts(net, batch, U):
    lib = _lib().load()
    rows, stride = lib.uavenv_dqn_partial_rows(batch), lib.uavenv_dqn_partial_stride(C.byref(net.net))
    out = [torch.full((rows + GUARD, stride), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32) for _ in range(U)]
    return out, rows


def bits(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def grad_slots(ring, nets, pairs, kind, huber, parts, images=None, expect=0):
    L = _lib()
    B = pairs.shape[1]
    rc = L.load().uavenv_dqn_grad_slots_img(C.byref(ring._c), ring.head, ring.filled, B, 0, 0, pairs.data_ptr(), net_array(nets),
                                            len(nets), kind, G.GAMMA, huber, ptrs(parts), None if images is None else ptrs(images),
                                            stream())
    assert rc == expect, rc


def grad_one(ring, net, pairs_j, kind, huber, part, image=None, abs_out=None):
    L = _lib()
    rc = L.load().uavenv_dqn_grad_img(C.byref(ring._c), ring.head, ring.filled, pairs_j.shape[0], 0, 0, pairs_j.data_ptr(),
                                      C.byref(net.net), kind, G.GAMMA, huber, None, None if abs_out is None else abs_out.data_ptr(),
                                      part.data_ptr(), None if image is None else image.data_ptr(), stream())
    assert rc == 0, rc


def hand_pairs(rng, ring, U, B):
    fa = (np.zeros((U, B), dtype=np.int64), rng.integers(0, ring.n, (U, B)))         # explicit, with repeats
    return fa, torch.tensor(np.stack(fa, 2).astype(np.int32), device="cuda").contiguous()


@pytest.fixture(scope="module")
def hand():
    """One small hand ring (two frames of 512 agents, a quarter of the rows invalid) per action count."""
    rings = {}

    def get(A):
        if A not in rings:
            rings[A] = G.make_hand("packed", 512, np.random.default_rng(40 + A), A, invalid_frac=0.25)
            assert (rings[A].host["valid"][0] == 0).any()
        return rings[A]
    return get


@pytest.mark.parametrize("A,dueling", HEADS, ids=lambda x: str(x))
@pytest.mark.parametrize("U", [1, 2, 4])
def test_grad_slots_equals_the_gradient_kernel_per_slot(hand, U, A, dueling):
    ring = hand(A)
    rng = np.random.default_rng([U, A, int(dueling)])
    for which, kind, huber in (("fresh", 0, 0), ("stress", 1, 1), ("fresh", 1, 0), ("stress", 0, 1)):
        nets = make_nets(A, dueling, which, U)
        images = [n.image() for n in nets]
        some = [im if j % 2 == 0 else None for j, im in enumerate(images)]
        for B in (64, 128):
            _, pairs = hand_pairs(rng, ring, U, B)
            want, rows = new_parts(nets[0], B, U)
            for j in range(U):
                grad_one(ring, nets[j], pairs[j], kind, huber, want[j], images[j])
            torch.cuda.synchronize()
            want = [bits(w) for w in want]
            P = nets[0].flat.size
            assert all(np.isfinite(w[:rows, :P + 2].view(np.float32)).all() and (w[rows:] == SENTINEL).all() for w in want)
            assert all(w[:rows, P + 1].view(np.float32).sum() < B for w in want)        # invalid rows among the pairs
            for imgs in (images, None, some):
                got, _ = new_parts(nets[0], B, U)
                grad_slots(ring, nets, pairs, kind, huber, got, imgs)
                torch.cuda.synchronize()
                for j in range(U):
                    assert np.array_equal(bits(got[j]), want[j]), (which, kind, huber, B, j, imgs is None)
            if U > 1 and B == 128:            # replacing net k changes partials[k] only
                k = int(rng.integers(0, U))
                other = list(nets)
                other[k] = Net(fresh_flat(A, dueling, 900 + k), A, dueling, "f32")
                got, _ = new_parts(nets[0], B, U)
                grad_slots(ring, other, pairs, kind, huber, got)
                torch.cuda.synchronize()
                for j in range(U):
                    assert np.array_equal(bits(got[j]), want[j]) == (j != k), (j, k)


@pytest.mark.parametrize("with_images", [True, False])
def test_grad_slots_persistent_workgroups(hand, with_images):
    """64 x 258 samples per slot: 258 tiles on uavenv_dqn_partial_rows' 256 workgroups, so workgroups 0 and 1 of every slot take a
    second tile (the tile loop and its barrier)."""
    U, A, B = 2, 3, 64 * 258
    ring = hand(A)
    nets = make_nets(A, False, "stress", U)
    images = [n.image() for n in nets] if with_images else None
    _, pairs = hand_pairs(np.random.default_rng(258), ring, U, B)
    want, rows = new_parts(nets[0], B, U)
    assert rows == 256
    for j in range(U):
        grad_one(ring, nets[j], pairs[j], 1, 0, want[j], None if images is None else images[j])
    got, _ = new_parts(nets[0], B, U)
    grad_slots(ring, nets, pairs, 1, 0, got, images)
    torch.cuda.synchronize()
    for j in range(U):
        w = bits(want[j])
        assert np.array_equal(bits(got[j]), w) and (w[rows:] == SENTINEL).all()
        cnt = w[:rows, nets[0].flat.size + 1].view(np.float32)
        assert cnt[:2].min() > 64 >= cnt[2:].max()                                   # two tiles in rows 0 and 1, one elsewhere


@pytest.mark.parametrize("A,dueling", HEADS, ids=lambda x: str(x))
def test_grad_slots_against_f64(hand, A, dueling):
    L = _lib()
    lib = L.load()
    U, B = 2, 128
    ring = hand(A)
    kind = 1 if dueling or A == 4 else 0
    kind_name = "dueling" if dueling else ("ddqn" if kind else "dqn")
    nets = make_nets(A, dueling, "stress" if A != 2 else "fresh", U)
    images = [n.image() for n in nets]
    fa, pairs = hand_pairs(np.random.default_rng([64, A, int(dueling)]), ring, U, B)
    parts, rows = new_parts(nets[0], B, U)
    grad_slots(ring, nets, pairs, kind, 0, parts, images)
    P = nets[0].flat.size
    for j in range(U):
        raw = torch.empty(P + 2, device="cuda")
        assert lib.uavenv_dqn_reduce(C.byref(nets[j].net), parts[j].data_ptr(), rows, raw.data_ptr(), stream()) == 0
        one, _ = new_parts(nets[0], B, 1)
        abs_td = torch.full((B,), -1.0, device="cuda")
        grad_one(ring, nets[j], pairs[j], kind, 0, one[0], images[j], abs_out=abs_td)
        torch.cuda.synchronize()
        assert np.array_equal(bits(one[0]), bits(parts[j]))
        raw, abs_td = raw.cpu().numpy(), abs_td.cpu().numpy()
        hb = G.host_batch(ring, (fa[0][j], fa[1][j]), None, False)
        fl = nets[j].buf[:2, :P].cpu().numpy().astype(np.float64)
        kw = dict(kind=kind_name, dueling=dueling, n_actions=A, gamma=float(np.float32(G.GAMMA)), huber=False,
                  relu_eps=G.F32["relu_eps"], tie_eps=G.F32["tie_eps"])
        args = (hb["s"], hb["s2"], hb["actions"], hb["rewards"], hb["dones"], hb["valid"], fl[0], fl[1])
        r = dqn_grad_f64(*args, is_weights=None, **kw)
        if r["near_tie"].any():               # (as run_case: a DDQN argmax within tie_eps is held to the kernel's own choice)
            alt = np.abs(abs_td - np.abs(r["delta_alt"])) < np.abs(abs_td - r["abs_td"])
            na = np.where(r["near_tie"], np.where(alt, r["a_alt"], r["a_next"]), -1)
            r = dqn_grad_f64(*args, is_weights=None, next_action=na, **kw)
        ok, worst = G.check_a(raw, abs_td, r, P, G.F32)
        print("slot", j, "worst ratio", round(worst, 4))
        assert ok, (A, dueling, j, worst, raw[P + 1], r["count"])
        assert 0 < r["count"] < B


def adam_state(nets, rng, rows, count):
    """Non-zero moments, a target that differs from the parameters, and random partial rows with `count` valid samples each."""
    P = nets[0].flat.size
    stride = _lib().load().uavenv_dqn_partial_stride(C.byref(nets[0].net))
    parts = []
    for n in nets:
        n.buf[2, :P] = torch.tensor(rng.normal(0, 1e-2, P).astype(np.float32), device="cuda")
        n.buf[3, :P] = torch.tensor(rng.uniform(1e-6, 1e-3, P).astype(np.float32), device="cuda")
        p = rng.normal(0, 1.0, (rows, stride)).astype(np.float32)
        p[:, P] = rng.uniform(10, 100, rows)
        p[:, P + 1] = count
        parts.append(torch.tensor(p, device="cuda"))
    return parts


@pytest.mark.parametrize("gate", ["none", "match", "miss"])
@pytest.mark.parametrize("U,A,dueling,rows", [(4, 3, False, 2), (2, 3, True, 256), (1, 2, False, 1), (4, 4, False, 256)])
def test_reduce_adam_slots_equals_the_per_slot_launch(U, A, dueling, rows, gate):
    L = _lib()
    lib = L.load()
    rng = np.random.default_rng([U, A, rows])
    steps = [1, 2, 3, 6][:U]                                   # update_loop 3: hard copies in slots 2 and 3 only
    hard = [1 if t % 3 == 0 else 0 for t in steps]
    word = torch.tensor([77], dtype=torch.int32, device="cuda")
    go, go_value = (None, 0) if gate == "none" else (word.data_ptr(), 77 if gate == "match" else 78)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    nets = make_nets(A, dueling, "stress", U)
    parts = adam_state(nets, rng, rows, 64.0)
    ref = [Net(n.flat, A, dueling, "f32") for n in nets]
    for n, r in zip(nets, ref):
        r.buf.copy_(n.buf)
    P = nets[0].flat.size
    images, ref_images = [n.image() for n in nets], [n.image() for n in ref]
    start = [n.buf.clone() for n in nets]
    loss = [torch.full((), -5.0, device="cuda") for _ in range(2 * U)]
    raw = [torch.full((P + 2,), -5.0, device="cuda") for _ in range(2 * U)]
    for j in range(U):
        assert lib.uavenv_dqn_reduce_adam_img(C.byref(ref[j].net), parts[j].data_ptr(), rows, lr, b1, b2, eps, steps[j], hard[j],
                                              loss[U + j].data_ptr(), raw[U + j].data_ptr(), go, go_value, ref_images[j].data_ptr(),
                                              stream()) == 0
    st, hd = (C.c_int32 * U)(*steps), (C.c_int32 * U)(*hard)
    assert lib.uavenv_dqn_reduce_adam_slots_img(net_array(nets), U, ptrs(parts), rows, lr, b1, b2, eps, st, hd, ptrs(loss[:U]),
                                                ptrs(raw[:U]), go, go_value, ptrs(images), stream()) == 0
    torch.cuda.synchronize()
    for j in range(U):
        assert np.array_equal(bits(nets[j].buf), bits(ref[j].buf)), j          # parameters, target, m, v
        assert np.array_equal(bits(loss[j]), bits(loss[U + j])) and np.array_equal(bits(raw[j]), bits(raw[U + j])), j
        assert np.array_equal(bits(images[j]), bits(ref_images[j])), j
        moved = not torch.equal(nets[j].buf, start[j])
        assert moved == (gate != "miss"), (j, gate)
        if gate == "miss":
            assert float(loss[j]) == -5.0 and float(raw[j][0]) == -5.0
        else:
            assert torch.equal(nets[j].buf[1, :P], nets[j].buf[0, :P]) == bool(hard[j]), j
    # the ABI entry: no images, no raw; loss cells nullable per entry
    again = [Net(n.flat, A, dueling, "f32") for n in nets]
    for n, s in zip(again, start):
        n.buf.copy_(s)
    cells = [torch.full((), -5.0, device="cuda") if j % 2 == 0 else None for j in range(U)]
    assert lib.uavenv_dqn_reduce_adam_slots(net_array(again), U, ptrs(parts), rows, lr, b1, b2, eps, st, hd, ptrs(cells), go, go_value,
                                            stream()) == 0
    torch.cuda.synchronize()
    for j in range(U):
        assert np.array_equal(bits(again[j].buf), bits(ref[j].buf)), j
        if cells[j] is not None:
            assert np.array_equal(bits(cells[j]), bits(loss[U + j]))


def fill(ring, passes, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for _ in range(passes):
        ring.current_action().copy_(torch.randint(0, 3, (ring.env.N,), generator=gen, device="cuda", dtype=torch.int32))
        ring.step_env(auto_reset=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("U,net,kind,with_images", [(4, "Qnet2", "dqn", False), (2, "VAnet2", "dueling", True)])
def test_update_slots_equals_learn_from_ring_per_learner(U, net, kind, with_images):
    from dqn_based_uav_3d_path_planer_amd.learner import update_slots
    B, n_envs = 128, 100
    env_a, ring_a, La = build(n_envs, U, net, kind)
    env_b, ring_b, Lb = build(n_envs, U, net, kind)
    fill(ring_a, 6, 3)
    fill(ring_b, 6, 3)
    assert torch.equal(ring_a.obs, ring_b.obs) and ring_a.filled == 6
    for j in range(U):
        La[j].epoch = Lb[j].epoch = j              # the slots' update counts differ: hard copies at different updates
    rng = np.random.default_rng(U)
    images = [L.split_image() for L in Lb] if with_images else None
    for step in range(3):
        f = (ring_a.head - 1 - rng.integers(0, ring_a.filled, (U, B))) % ring_a.frames
        agent = rng.integers(0, n_envs, (U, B)) * U + np.arange(U)[:, None]
        pairs = torch.tensor(np.stack([f, agent], 2).astype(np.int32), device="cuda").contiguous()
        for j in range(U):
            La[j].learn_from_ring(ring_a, B, 0, 0, explicit_idx=pairs[j])
        update_slots(Lb, ring_b, B, pairs, images=images)
        torch.cuda.synchronize()
        for j in range(U):
            assert torch.equal(La[j].flat, Lb[j].flat) and La[j].epoch == Lb[j].epoch == j + step + 1, (step, j)
            assert float(La[j].loss) == float(Lb[j].loss) and np.isfinite(float(Lb[j].loss)), (step, j)
            if with_images:
                assert torch.equal(images[j], Lb[j].split_image()), (step, j)      # the images followed the parameters
    assert any(torch.equal(L.flat[0], L.flat[1]) for L in Lb) and not all(torch.equal(L.flat[0], L.flat[1]) for L in Lb)
    env_a.close()
    env_b.close()


@pytest.mark.parametrize("U,batch,net,kind,mode", [(4, 64, "Qnet2", "dqn", "reset"), (2, 128, "VAnet2", "ddqn", "skip")])
def test_multi_update_loop_equals_the_composition(U, batch, net, kind, mode):
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    n_envs, passes, seed, eps = 200, 23, 9, 0.2
    kind = "dueling" if net == "VAnet2" else kind
    auto_reset, valid_draws, gate = (True, False, False) if mode == "reset" else (False, True, True)
    env_a, ring_a, La = build(n_envs, U, net, kind)
    assert ring_a.frames == 9
    compose(ring_a, La, passes, batch, seed, eps, auto_reset, True, valid_draws)
    env_b, ring_b, Lb = build(n_envs, U, net, kind)
    loop = DQNSlotsHotLoop(ring_b, Lb, batch, seed=seed, eps=eps, auto_reset=auto_reset, skip_done=True, gate_updates=gate,
                           valid_draws=valid_draws, multi_update=True)
    assert loop.multi_update
    loop.run(10)
    assert loop.in_sync(batch)
    loop.run(passes - 10)
    torch.cuda.synchronize()
    assert (ring_b.head, ring_b.filled, loop.counter) == (ring_a.head, ring_a.filled, passes)
    assert [x.epoch for x in Lb] == [x.epoch for x in La] and La[0].epoch == passes
    for name in ("obs", "action", "reward", "done", "valid"):
        assert torch.equal(getattr(ring_a, name), getattr(ring_b, name)), name
    for j, (a, b) in enumerate(zip(La, Lb)):
        assert torch.equal(a.flat, b.flat), j                                    # parameters, target, moments
        assert float(a.loss) == float(b.loss) and np.isfinite(float(b.loss)), j
    assert len({float(x.flat[0].sum()) for x in Lb}) == U
    loop.close()
    env_a.close()
    env_b.close()


def test_the_setter_toggled_between_runs():
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    out = []
    for plan in ((False, False, False), (True, False, True)):
        env, ring, Ls = build(200, 4, "Qnet2", "dqn")
        loop = DQNSlotsHotLoop(ring, Ls, 64, seed=5, eps=0.2, multi_update=plan[0])
        for k, on in enumerate(plan):
            if k:
                loop.set_multi_update(on)
            assert loop.multi_update == on
            loop.run(6)
        torch.cuda.synchronize()
        out.append(([L.flat.clone() for L in Ls], [float(L.loss) for L in Ls], [L.epoch for L in Ls], ring.obs.clone(), loop.counter))
        loop.close()
        env.close()
    a, b = out
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[1:3] == b[1:3] and torch.equal(a[3], b[3]) and a[4] == b[4] == 18
    assert a[2] == [18] * 4


def test_multi_update_refuses_heads_of_more_than_four_outputs():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
    from test_dqn_slots_loop_gpu import PARAM
    env = make_city26_env(64, obs_dtype="packed", uav_per_env=2)
    ring = DeviceReplayRing(env, 8 * env.N, discrete=True)
    ring.reset(seed=12)
    Ls = [FusedDQNLearner(dict(PARAM, NetWork="Qnet2", output="5"), "dqn", device="cuda:0") for _ in range(2)]
    with pytest.raises(L.UavEnvError):
        DQNSlotsHotLoop(ring, Ls, 64, seed=5, multi_update=True)
    loop = DQNSlotsHotLoop(ring, Ls, 64, seed=5)               # the per-slot form takes them
    with pytest.raises(L.UavEnvError):
        loop.set_multi_update(True)
    assert not loop.multi_update                               # left as it was
    loop.run(3)
    torch.cuda.synchronize()
    assert [x.epoch for x in Ls] == [3, 3]
    loop.close()
    env.close()


def test_a_federated_merge_between_two_multi_update_runs_reaches_the_next_pass():
    """As the per-slot loop's test: every run rebuilds the layer-1 images, so the pass after a merge acts AND learns with the
    merged weights -- against a per-slot loop that went through the same merge."""
    from dqn_based_uav_3d_path_planer_amd import federated
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop

    class T:
        fused = True

        def __init__(self, L):
            self.learner, self.q_local = L, L.q_local

    out = []
    for multi in (False, True):
        env, ring, Ls = build(200, 4, "Qnet2", "dqn")
        loop = DQNSlotsHotLoop(ring, Ls, 64, seed=4, eps=0.1, multi_update=multi)
        loop.run(6)
        torch.cuda.synchronize()
        before = Ls[1].flat[0].clone()
        assert federated.federated_learning_q([T(L) for L in Ls], "mean") == "device"
        torch.cuda.synchronize()
        assert all(torch.equal(L.flat[0], Ls[0].flat[0]) for L in Ls) and not torch.equal(Ls[1].flat[0], before)
        t = ring.head
        loop.run(2)
        torch.cuda.synchronize()
        out.append(([L.flat.clone() for L in Ls], ring.action[t].clone(), [float(L.loss) for L in Ls]))
        loop.close()
        env.close()
    a, b = out
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_gated_multi_update_with_every_agent_finished_leaves_the_learners():
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    env, ring, Ls = build(64, 2, "Qnet2", "dqn")
    loop = DQNSlotsHotLoop(ring, Ls, 64, seed=6, eps=0.3, auto_reset=False, skip_done=True, gate_updates=True, multi_update=True)
    w0 = [L.flat.clone() for L in Ls]
    for _ in range(60):                        # no restarts: the episode ends for every agent (success, crash or the step limit)
        loop.run(50)
        torch.cuda.synchronize()
        if not bool(ring.valid[(ring.head - 1) % ring.frames].any()):
            break
    assert not bool(ring.valid[(ring.head - 1) % ring.frames].any()), "the episode did not end"
    assert not any(torch.equal(L.flat, w) for L, w in zip(Ls, w0))
    loop.run(1)                                # (one more: the pass that found the last agent finished is behind us for certain)
    torch.cuda.synchronize()
    w1, l1, e1 = [L.flat.clone() for L in Ls], [float(L.loss) for L in Ls], [L.epoch for L in Ls]
    loop.run(7)
    torch.cuda.synchronize()
    assert all(torch.equal(L.flat, w) for L, w in zip(Ls, w1)) and [float(L.loss) for L in Ls] == l1
    assert [L.epoch for L in Ls] == [e + 7 for e in e1]        # (the host's counts go on, as in the per-slot form)
    loop.close()
    env.close()
