"""The paths of k_dqn_grad_packed8<true> (the bench / C-loop form, through uavenv_dqn_grad_img with a layer-1 image) that a change to
its instruction stream must not break, on a packed ring of 9 frames x 2 048 agents filled by real step launches:

 * the in-kernel draw against the same launch given uavenv_replay_draw's pairs explicitly, at 64, 128 and 16 512 samples -- one
   tile, two workgroups, and 258 tiles on 256 workgroups (the looped second copy of the tile runs; 16 512 > 8 x 2 048 stored
   transitions, so the draw wraps too): partial rows byte for byte;
 * is_w all ones against no is_w, |TD| requested against not requested: partial rows byte for byte, and the |TD| output against
   |delta| recomputed in float64 at the bound of tests/test_dqn_grad_kernels_gpu.py (tau_td q_abs, tau_td = 2^-16);
 * the option grid dqn / ddqn x MSE / Huber x Qnet2 / VAnet2 (three actions) at batch 128 against oracle/dqn_grad_ref.py's float64
   bucket with check (a) and the f32 bars of tests/test_dqn_grad_kernels_gpu.py, unchanged;
 * the row writer on a partials buffer pre-filled with a NaN pattern: every column below P + 2 of every written row finite,
   columns [P + 2, stride) and the rows at or beyond the grid untouched, dW1 columns 96..99 exact zeros.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_dqn_grad_kernels_gpu as T
from dqn_fixtures import unpack

pytestmark = pytest.mark.gpu

N, FRAMES = 2048, 9
NAN_BITS = 0x7FC0BEEF          # a quiet NaN with a payload no arithmetic produces


class Ring9:
    """What T.RealRing wraps (ring, obs, env): a packed ring of 9 frames that has wrapped."""

    def __init__(self):
        from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
        from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
        self.env = make_city26_env(N, obs_dtype="packed")
        self.ring = DeviceReplayRing(self.env, (FRAMES - 1) * N, discrete=True)
        assert self.ring.frames == FRAMES
        self.ring.reset(seed=9)
        gen = torch.Generator(device="cuda").manual_seed(2)
        for _ in range(12):                                      # 12 steps on 9 frames: wrapped
            self.ring.current_action().copy_(torch.randint(0, 3, (N,), generator=gen, device="cuda", dtype=torch.int32))
            self.ring.step_env(auto_reset=True)
        torch.cuda.synchronize()
        assert self.ring.filled == FRAMES - 1
        self.obs = unpack(self.ring.obs)


_S = {}


@pytest.fixture(scope="module")
def st():
    """One ring, its pairs and the learners of the grid, shared by every test of the module and left unchanged by them."""
    p = Ring9()
    _S.update(p=p, ring=T.RealRing(p), learners={})
    yield _S
    p.env.close()
    _S.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def learner(st, net, huber):
    key = (net, huber)
    if key not in st["learners"]:
        from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
        torch.manual_seed(31 + len(st["learners"]))
        L = FusedDQNLearner(dict(T.PARAM, NetWork=net, output="3"), "dueling" if net == "VAnet2" else "dqn", device="cuda:0",
                            loss="huber" if huber else "mse")
        with torch.no_grad():
            L.flat[1].copy_(L.flat[0] + 0.02 * torch.randn_like(L.flat[0]))
        st["learners"][key] = (L, L.split_image())
    return st["learners"][key]


def pairs(st, B, seed, counter):
    ring = st["ring"]
    out = torch.empty((B, 2), dtype=torch.int32, device="cuda")
    assert st["p"].env.lib.uavenv_replay_draw(ring.frames, N, ring.head, ring.filled, B, seed, counter, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return out


def filled_partials(L, B, extra_rows=2):
    """The partials buffer of a batch-B launch plus rows behind the grid, every dword the NaN pattern."""
    rows = L.lib.uavenv_dqn_partial_rows(B)
    stride = L.lib.uavenv_dqn_partial_stride(C.byref(L.net))
    t = torch.full((rows + extra_rows, stride), NAN_BITS, dtype=torch.int32, device="cuda")
    return t, rows, stride


def launch(L, img, ring, B, kind, idx, isw, abs_out, seed=11, counter=5, parts=None):
    """uavenv_dqn_grad_img with `kind` as given (0: max_a Q_target, 1: the double-DQN choice), whatever the learner's own is;
    returns the partials as int32 bits on the host."""
    if parts is None:
        parts = filled_partials(L, B)[0]
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = L.lib.uavenv_dqn_grad_img(C.byref(ring._c), ring.head, ring.filled, B, seed, counter, p(idx), C.byref(L.net), kind,
                                   T.GAMMA, L.huber, p(isw), p(abs_out), parts.data_ptr(), img.data_ptr(), L._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return parts.cpu().numpy()


@pytest.mark.parametrize("B", [64, 128, 16512])
def test_in_kernel_draw_equals_explicit_pairs(st, B):
    L, img = learner(st, "Qnet2", False)
    assert L.lib.uavenv_dqn_partial_rows(B) == min(B // 64, 256)
    drawn = launch(L, img, st["ring"], B, 0, None, None, None, seed=11, counter=B)
    given = launch(L, img, st["ring"], B, 0, pairs(st, B, 11, B), None, None, seed=11, counter=B)
    assert np.array_equal(drawn, given)
    P = L.P
    assert drawn.view(np.float32)[:min(B // 64, 256), P + 1].sum() > 0          # (valid samples were counted: the launch ran)


def test_unit_weights_and_abs_td_leave_rows_unchanged(st):
    B = 128
    L, img = learner(st, "Qnet2", False)
    ring = st["ring"]
    idx = pairs(st, B, 11, 3)
    plain = launch(L, img, ring, B, 0, idx, None, None)
    ones = launch(L, img, ring, B, 0, idx, torch.ones(B, device="cuda"), None)
    abs_out = torch.full((B,), -1.0, device="cuda")
    with_td = launch(L, img, ring, B, 0, idx, None, abs_out)
    assert np.array_equal(plain, ones)
    assert np.array_equal(plain, with_td)
    fa = idx.cpu().numpy().astype(np.int64)
    hb = T.host_batch(ring, (fa[:, 0], fa[:, 1]), None, False)
    local, target = T.ref_params(L, False)
    r = T.dqn_grad_f64(hb["s"], hb["s2"], hb["actions"], hb["rewards"], hb["dones"], hb["valid"], local, target, kind="dqn",
                       dueling=False, n_actions=3, gamma=float(np.float32(T.GAMMA)), huber=False, relu_eps=T.F32["relu_eps"],
                       tie_eps=T.F32["tie_eps"])
    err = np.abs(abs_out.cpu().numpy() - r["abs_td"])
    bar = T.F32["tau_td"] * r["q_abs"] + r["td_amb"] + 1e-30
    print("abs_td worst error / bar", float((err / bar).max()))
    assert np.all(err <= bar)


GRID = [(kind, huber, net) for kind in ("dqn", "ddqn") for huber in (False, True) for net in ("Qnet2", "VAnet2")]


@pytest.mark.parametrize("case", GRID, ids=lambda c: "%s-%s-%s" % (c[0], "huber" if c[1] else "mse", c[2]))
def test_option_grid_against_f64(st, case):
    kind, huber, net = case
    B = 128
    L, img = learner(st, net, huber)
    ring = st["ring"]
    seed = GRID.index(case)
    idx = pairs(st, B, 11, 100 + seed)
    abs_out = torch.full((B,), -1.0, device="cuda")
    parts, rows, _ = filled_partials(L, B)
    launch(L, img, ring, B, 0 if kind == "dqn" else 1, idx, None, abs_out, parts=parts)
    raw = torch.empty(L.P + 2, device="cuda")
    assert L.lib.uavenv_dqn_reduce(C.byref(L.net), parts.view(torch.float32).data_ptr(), rows, raw.data_ptr(), L._stream()) == 0
    torch.cuda.synchronize()
    raw, abs_td = raw.cpu().numpy(), abs_out.cpu().numpy()
    fa = idx.cpu().numpy().astype(np.int64)
    hb = T.host_batch(ring, (fa[:, 0], fa[:, 1]), None, False)
    local, target = T.ref_params(L, False)
    kw = dict(kind=kind, dueling=net == "VAnet2", n_actions=3, gamma=float(np.float32(T.GAMMA)), huber=huber,
              relu_eps=T.F32["relu_eps"], tie_eps=T.F32["tie_eps"])
    args = (hb["s"], hb["s2"], hb["actions"], hb["rewards"], hb["dones"], hb["valid"], local, target)
    r = T.dqn_grad_f64(*args, **kw)
    if r["near_tie"].any():        # (as run_case: a double-DQN argmax within tie_eps is held to the kernel's own choice)
        alt = np.abs(abs_td - np.abs(r["delta_alt"])) < np.abs(abs_td - r["abs_td"])
        na = np.where(r["near_tie"], np.where(alt, r["a_alt"], r["a_next"]), -1)
        r = T.dqn_grad_f64(*args, next_action=na, **kw)
    ok, worst = T.check_a(raw, abs_td, r, L.P, T.F32)
    print(case, "worst error / bar", round(worst, 4), "count", raw[L.P + 1], r["count"])
    assert ok, (case, worst, raw[L.P + 1], r["count"])


@pytest.mark.parametrize("B", [128, 16512])
def test_row_writer_touches_its_columns_only(st, B):
    L, img = learner(st, "Qnet2", False)
    P = L.P
    parts, rows, stride = filled_partials(L, B, extra_rows=2)
    out = launch(L, img, st["ring"], B, 0, None, None, None, counter=7, parts=parts)
    assert stride >= P + 2 and rows == min(B // 64, 256)
    assert np.isfinite(out[:rows, :P + 2].view(np.float32)).all()
    assert np.all(out[:rows, P + 2:] == np.int32(NAN_BITS))
    assert np.all(out[rows:] == np.int32(NAN_BITS))
    dW1 = out[:rows, :64 * 100].reshape(rows, 64, 100)
    assert np.all(dW1[:, :, 96:] == 0)                                         # +0.0, bit for bit
