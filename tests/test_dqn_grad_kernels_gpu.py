"""Every DQN gradient kernel form of csrc/learner.hip (the dispatch in uavenv_dqn_grad_img), held against the float64 bucket of
oracle/dqn_grad_ref.py at the RAW bucket -- gradient sums, loss sum, valid count and |TD error| -- before any Adam step, through
the C ABI (uavenv_dqn_grad_img + uavenv_dqn_reduce), so the weights never move between checks.  Then the fused reduction + Adam
(uavenv_dqn_reduce_adam) against adam_step_f64, and the padded FusedDQNLearner.learn() path.

Per case:
 (a) accuracy against f64, per parameter component p:
        |raw_p - g_p| <= tau M_p + K tau_td sqrt(N2_p) + Z_p
     M_p = sum_s |contribution_{s,p}| (|delta_s| widened by 2^-20 (|q_a| + |y|)); N2_p = sum_s (q_abs_s |d contribution_{s,p} /
     d delta_s|)^2 (q_abs_s: the |.|-forward behind delta_s); Z_p: the terms an arithmetic within its bound may decide the other
     way (a ReLU pre-activation within relu_eps of zero; a DDQN argmax within tie_eps is instead held to the kernel's own choice,
     read back from its |TD error|).  The loss sum the same way; the valid count exactly; abs_td_s to tau_td q_abs_s.
     And the error's projection on the gradient itself (its layer-2 block, which no ReLU decision moves), the direction a uniform
     scale error takes:
        |<raw - g, g>| <= K sqrt(sum_p (sig M_p g_p)^2 + sum_s (sig_td q_abs_s <|d c_s / d delta_s|, |g|>)^2) + 2 K 2^-24 max(.)
                          (with every (sample, unit) whose ReLU is within relu_eps a further independent term: its flip)
     (Bernstein: independent unbiased roundings, each at most 2^-24 times its scale; K = 6, 2 exp(-K^2 / 2) = 3e-8.)
     f32-accuracy forms (every f32-MFMA form, packed8 with its split two-term f16 layer-1 products included):
        forward: layer 1 sums 101 terms, layer 2 65, the dueling combine and the target a few more, each term rounded once at
        u = 2^-24: |err delta_s| <= 180 u q_abs_s < 2^-16 q_abs_s -> tau_td = relu_eps = tie_eps = 2^-16.  The deltas of
        different samples round independently, so their effect on a component is K root-sum-squares of that bound, not the sum;
        with round-to-nearest their standard deviation is at most sqrt(180 / 3) u q_abs_s < 2^-20 q_abs_s = sig_td q_abs_s;
        backward: every gradient term is a product of two or three f32 values, each within ~70 u of exact, summed over the
        batch in f32 (a random walk of ~300 roundings on partial sums <= M: ~2^-20 M): tau = 2^-17 per component; the partial
        sums reach M_p only in the last ~16 additions (the workgroup-row reduction), so the standard deviation of a
        component's summation error is below 4 u M_p < 2^-21 M_p = sig M_p.
     f16-MFMA forms (k_dqn_grad_h8): observations and fc1 weights are rounded to f16 by design, and the
     reference is fed exactly those rounded inputs; what remains is the rounding of the H, dH and dout operands of the gradient
     products (and of H into layer 2) to an 11-bit significand, 2^-11 relative each: a gradient term carries at most two such
     roundings, 2^-10, and delta at most 2^-11 q_abs from H plus the f32 terms: tau = 2^-10, tau_td = relu_eps = tie_eps = 2^-9,
     sig = 2^-13, sig_td = 2^-12.
 (b) tile-partition invariance: the same explicit list as one launch and as 64-sample one-workgroup launches summed in f64;
     only the order of the f32 summation differs, bounded as above by 2^-20 M_p (loss: 2^-20 M_loss); count exact; abs_td bit
     for bit (every form computes a sample's delta by the same instructions whatever its tile or workgroup).
 (c) for B >= 16 384, on the host only: the f64 side perturbed by one dropped or duplicated sample (gradient and loss; the
     valid sample of median |dq|), the gradient scaled by (1 + 1/B), and the count off by one.  For the f32-accuracy forms (a)
     ALONE must reject each: a bug common to every tile shows on both sides of (b), so (b) cannot stand in for (a).
     Resolving power: for the f16-MFMA forms (tau = 2^-10, 128 x the f32 bar) (a) cannot resolve one sample or a 1/B scale
     at B >= 16 384.  There (a) must reject only the count; a dropped or duplicated sample must be rejected by (a) or (b),
     which guards tile-local drops; NOTHING guards a drop common to all tiles or a uniform scale in those forms at that size
     -- the f32 forms, which share td_backward and the reductions with them, are the guard there.
Worst measured ratio (error / bar) per form over the cases below, (a) / (b), on an MI355X (printed with -s):
  packed8<false> 0.013 / 0.159      packed8<true> 0.023 / 0.147       h8<PACKED> 0.051 / 0.087     h8<F16> 0.194 / 0.117
  grad<float, 4> 0.006 / 0.119      grad<half, 4> 0.025 / 0.106       grad<float, NMAX> 0.025 / 0.123
  grad<half, NMAX> 0.008 / 0.133    grad_packed<NMAX> 0.113 / 0.095
  knob children: packed8<false> register-staged 0.006 / 0.088.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dqn_fixtures import Pool, unpack
from oracle.dqn_grad_ref import adam_step_f64, dqn_grad_f64, layout, sample_contribution

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM = {"w": "100", "hiden_dim": "64", "LEARNING_RATE": "0.001", "gamma": "0.99", "Update_loop": "3"}
GAMMA = 0.99
F32 = dict(tau=2.0 ** -17, tau_td=2.0 ** -16, relu_eps=2.0 ** -16, tie_eps=2.0 ** -16, sig=2.0 ** -21, sig_td=2.0 ** -20)
F16 = dict(tau=2.0 ** -10, tau_td=2.0 ** -9, relu_eps=2.0 ** -9, tie_eps=2.0 ** -9, sig=2.0 ** -13, sig_td=2.0 ** -12)
PART = 2.0 ** -20
K = 6.0                     # root-sum-square multiple: 2 exp(-K^2 / 2) = 3e-8 (Hoeffding)
# obs kind, MFMA, layer-1 image, outputs
FORMS = {
    "p8": ("packed", "f32", False, 3),      # k_dqn_grad_packed8<false>
    "p8i": ("packed", "f32", True, 3),      # k_dqn_grad_packed8<true>: the bench / C-loop form
    "h8p": ("packed", "f16", False, 3),     # k_dqn_grad_h8<PACKED>
    "h8f": ("f16", "f16", False, 3),        # k_dqn_grad_h8<F16>
    "g32": ("f32", "f32", False, 3),        # k_dqn_grad<float, 4>
    "g16": ("f16", "f32", False, 3),        # k_dqn_grad<__half, 4>
    "g32n": ("f32", "f32", False, 9),       # k_dqn_grad<float, NMAX>
    "g16n": ("f16", "f32", False, 9),       # k_dqn_grad<__half, NMAX>
    "pn": ("packed", "f32", False, 9),      # k_dqn_grad_packed<NMAX>
}
WORST = {}


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


_POOL = None


def pool():
    global _POOL
    if _POOL is None:
        _POOL = Pool()
    return _POOL


@pytest.fixture(scope="module", autouse=True)
def _release_pool():
    """The pool's environment and ring live for this module only: later modules time their own loops on the same device."""
    global _POOL
    yield
    if _POOL is not None:
        _POOL.env.close()
        _POOL = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class HandRing:
    """Two frames of n agents (frame 0 = s, frame 1 = s'), observation rows drawn from the pool, stored as `obs_kind`."""

    def __init__(self, obs_kind, rows0, rows1, action, reward, done, valid):
        L = _lib()
        self.obs_kind = obs_kind
        self.n = n = len(action)
        self.host = dict(obs=np.stack([rows0, rows1]).astype(np.float32), action=np.stack([action, np.zeros(n)]).astype(np.int32),
                         reward=np.stack([reward, np.zeros(n)]).astype(np.float32),
                         done=np.stack([done, np.zeros(n)]).astype(np.uint8), valid=np.stack([valid, np.ones(n)]).astype(np.uint8))
        self.upload()
        code = {"packed": L.OBS_PACKED, "f16": L.OBS_F16, "f32": L.OBS_F32}[obs_kind]
        self._c = L.UavReplayRing(self.obs.data_ptr(), self.action.data_ptr(), self.reward.data_ptr(), self.done.data_ptr(),
                                  self.valid.data_ptr(), 2, n, code, 1)
        self.head, self.filled, self.frames = 1, 1, 2

    def upload(self):
        h = self.host
        if self.obs_kind == "packed":
            ob = torch.tensor(np.stack([self._packrows(h["obs"][0]), self._packrows(h["obs"][1])]))
        elif self.obs_kind == "f16":
            ob = torch.tensor(h["obs"]).half()
        else:
            ob = torch.tensor(h["obs"])
        if hasattr(self, "obs"):                      # in place: the C ring keeps pointing at the same planes
            self.obs.copy_(ob.cuda())
            for k in ("action", "reward", "done", "valid"):
                getattr(self, k).copy_(torch.tensor(h[k]).cuda())
        else:
            self.obs = ob.cuda().contiguous()
            for k in ("action", "reward", "done", "valid"):
                setattr(self, k, torch.tensor(h[k]).cuda().contiguous())

    @staticmethod
    def _packrows(rows):
        from conftest import pack_obs_rows
        return pack_obs_rows(rows)

    def obs_f(self):
        """[frames, n, 100] as the kernels read them (f16 rings: the stored halves)."""
        o = self.host["obs"]
        return o.astype(np.float16).astype(np.float32) if self.obs_kind == "f16" else o

    def planes(self):
        h = self.host
        return self.obs_f(), h["action"], h["reward"], h["done"], h["valid"]


class RealRing:
    """The pool's wrapped packed ring as the kernels see it (with its 16-byte transition records)."""

    def __init__(self, p):
        self.p, self._c, self.head, self.filled, self.frames = p, p.ring._c, p.ring.head, p.ring.filled, p.ring.frames
        self.obs_kind = "packed"

    def planes(self):
        r = self.p.ring
        return (self.p.obs, r.action.cpu().numpy(), r.reward.cpu().numpy(), r.done.cpu().numpy(), r.valid.cpu().numpy())


def make_hand(obs_kind, n, rng, A, extreme=True, invalid_frac=0.0):
    rows = pool().rows
    r0 = rows[rng.integers(0, len(rows), n)]
    r1 = rows[rng.integers(0, len(rows), n)]
    # rewards centred off zero: in a batch whose TD errors cancel, the gradient is rounding-sized noise and no bar can see a 1/B
    # scale of it (the mutation check (c) requires (a) to)
    reward = rng.normal(-3.0, 5.0, n)
    if extreme:                                     # the reference's reward extremes (arrival / crash: +-200 scale)
        k = rng.random(n)
        reward = np.where(k < 0.05, 200.0, np.where(k < 0.10, -200.0, reward))
    done = (rng.random(n) < 0.2).astype(np.uint8)
    valid = (rng.random(n) >= invalid_frac).astype(np.uint8)
    return HandRing(obs_kind, r0, r1, rng.integers(0, A, n), reward, done, valid)


def make_learner(form, kind, huber, seed):
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    obs_kind, mfma, img, out = FORMS[form]
    torch.manual_seed(seed)
    net = "VAnet2" if kind == "dueling" else "Qnet2"
    L = FusedDQNLearner(dict(PARAM, NetWork=net, output=str(out)), kind, device="cuda:0", mfma=mfma,
                        loss="huber" if huber else "mse")
    with torch.no_grad():
        L.flat[1].copy_(L.flat[0] + 0.02 * torch.randn_like(L.flat[0]))
    return L


def make_tie(L):
    """Q_local(s') ties exactly between actions 0 and 1 (identical fc2 / fc_A rows and biases), the others far below; the target
    differs so that picking action 1 moves y by 0.99 * 5."""
    A, hid, w = L.n_actions, 64, 100
    n2 = A + (1 if L.dueling else 0)
    o_b1, o_w2, o_b2, _ = layout(w, hid, n2)
    with torch.no_grad():
        for blk in (0, 1):
            f = L.flat[blk]
            f[o_w2 + hid:o_w2 + 2 * hid] = f[o_w2:o_w2 + hid]
            f[o_b2 + 1] = f[o_b2]
        for a in range(2, A):
            L.flat[0][o_b2 + a] = L.flat[0][o_b2] - 30.0
        L.flat[1][o_b2 + 1] = L.flat[1][o_b2] + 5.0


def launch(L, ring, B, idx, isw, abs_out, img, parts, seed=0, counter=0, idx_off=0):
    lib = L.lib
    p = lambda t, off=0: None if t is None else t.data_ptr() + off  # noqa: E731
    kind = 0 if L.kind == "dqn" else 1
    rc = lib.uavenv_dqn_grad_img(C.byref(ring._c), ring.head, ring.filled, B, seed, counter, p(idx, 8 * idx_off), C.byref(L.net),
                                 kind, GAMMA, L.huber, p(isw, 4 * idx_off), p(abs_out, 4 * idx_off), parts, p(img), L._stream())
    assert rc == 0, rc


def run_whole(L, ring, B, idx, isw, img, seed=0, counter=0):
    nblk = L.lib.uavenv_dqn_partial_rows(B)
    parts = L.new_partials(B)
    abs_out = torch.full((B,), -1.0, device="cuda")
    launch(L, ring, B, idx, isw, abs_out, img, parts.data_ptr(), seed, counter)
    raw = torch.empty(L.P + 2, device="cuda")
    assert L.lib.uavenv_dqn_reduce(C.byref(L.net), parts.data_ptr(), nblk, raw.data_ptr(), L._stream()) == 0
    torch.cuda.synchronize()
    return raw.cpu().numpy(), abs_out.cpu().numpy(), parts, nblk


def run_tiles(L, ring, B, idx, isw, img):
    nt = B // 64
    stride = L.lib.uavenv_dqn_partial_stride(C.byref(L.net))
    parts = torch.empty((nt, stride), device="cuda")
    abs_out = torch.full((B,), -1.0, device="cuda")
    for t in range(nt):
        launch(L, ring, 64, idx, isw, abs_out, img, parts.data_ptr() + 4 * t * stride, idx_off=64 * t)
    torch.cuda.synchronize()
    return parts[:, :L.P + 2].double().sum(0).cpu().numpy(), abs_out.cpu().numpy()


def host_batch(ring, fa, isw, f16_obs):
    obs, act, rew, done, valid = ring.planes()
    f, a = fa
    fn = (f + 1) % obs.shape[0]
    s, s2 = obs[f, a], obs[fn, a]
    if f16_obs:
        s, s2 = s.astype(np.float16).astype(np.float32), s2.astype(np.float16).astype(np.float32)
    return dict(s=s, s2=s2, actions=act[f, a], rewards=rew[f, a], dones=done[f, a], valid=valid[f, a],
                is_weights=None if isw is None else isw.cpu().numpy())


def ref_params(L, f16):
    fl = L.flat[:2].cpu().numpy().astype(np.float64)
    if f16:
        fl[:, :6400] = fl[:, :6400].astype(np.float16).astype(np.float64)
    return fl[0], fl[1]


def check_a(raw, abs_td, r, P, bars):
    """(a): returns (ok, worst ratio).  Per component: tau M_p + K tau_td sqrt(N2_p) + Z_p; the loss sum alike; the count exactly;
    abs_td per sample; and the projection of the error on the gradient itself (a uniform scale error), against the
    root-sum-square of the same bars."""
    e = raw[:P].astype(np.float64) - r["grad"]
    g_bar = bars["tau"] * r["M"] + K * bars["tau_td"] * np.sqrt(r["N2"]) + r["Z"] + 1e-30
    rg = np.abs(e) / g_bar
    l_bar = bars["tau"] * r["M_loss"] + K * bars["tau_td"] * np.sqrt(r["N2_loss"]) + r["Z_loss"] + 1e-30
    rl = abs(float(raw[P]) - r["loss"]) / l_bar
    t_bar = bars["tau_td"] * r["q_abs"] + r["td_amb"] + 1e-30
    rt = np.abs(abs_td - r["abs_td"]) / t_bar
    # the direction: the gradient's layer-2 block (fc2 / fc_A, fc_V and their biases).  A uniform scale shows there as much as
    # anywhere, and no ReLU decision moves it: a flip within relu_eps changes H by at most relu_eps |.|-forward
    g = r["grad"].copy()
    g[:64 * 101] = 0.0
    sm, sd, zs = r["dir_sens"](g)
    var = np.sum((bars["sig"] * sm) ** 2) + np.sum((bars["sig_td"] * sd) ** 2)
    b_max = 2.0 ** -24 * max(sm.max(), sd.max())
    # each (sample, unit) whose ReLU is within relu_eps may flip, independently, by at most zs in <error, g>; near ties are
    # already held to the kernel's choice
    var += np.sum(zs ** 2)
    b_max = max(b_max, float(zs.max()) if zs.size else 0.0)
    s_bar = K * np.sqrt(var) + 2 * K * b_max + 1e-300
    rs = abs(float(e @ g)) / s_bar
    worst = max(rg.max(), rl, rt.max(), rs)
    return bool(worst <= 1.0 and raw[P + 1] == r["count"]), float(worst)


def check_b(whole, tiles, abs_w, abs_t, r, P):
    rb = max((np.abs(whole[:P] - tiles[:P]) / (PART * r["M"] + 1e-30)).max(),
             abs(whole[P] - tiles[P]) / (PART * r["M_loss"] + 1e-30))
    return bool(rb <= 1.0 and whole[P + 1] == tiles[P + 1] and np.array_equal(abs_w, abs_t)), float(rb)


def run_case(form, B, kind, huber, weighted, source, seed):
    obs_kind, mfma, use_img, A = FORMS[form]
    f16 = mfma == "f16"
    bars = dict(F16 if f16 else F32)
    rng = np.random.default_rng(seed)
    L = make_learner(form, kind, huber, seed)
    if source == "tie":
        make_tie(L)
        bars["tie_eps"] = 0.0                           # exact ties: the first maximum, no allowance
    if source == "draw":
        ring = RealRing(pool())
        assert obs_kind == "packed"
        from oracle.philox import replay_draws
        fa = replay_draws(B, 11, seed, ring.head, ring.filled, ring.frames, pool().env.N)
        assert (fa[0] == ring.frames - 1).any()        # some s' come from frame 0
    else:
        n = min(B, 4096)
        ring = make_hand(obs_kind, n, rng, A, invalid_frac=0.25 if source == "invalid" else 0.0)
        fa = (np.zeros(B, dtype=np.int64), rng.integers(0, n, B))     # explicit, with repeats
    idx = torch.tensor(np.stack(fa, 1).astype(np.int32), device="cuda").contiguous()
    isw = torch.tensor(rng.uniform(0.05, 1.0, B).astype(np.float32), device="cuda") if weighted else None
    img = L.split_image() if use_img else None
    hb = host_batch(ring, fa, isw, f16)
    local, target = ref_params(L, f16)
    kw = dict(kind=kind, dueling=kind == "dueling", n_actions=A, gamma=float(np.float32(GAMMA)), huber=huber,
              relu_eps=bars["relu_eps"], tie_eps=bars["tie_eps"])
    r = dqn_grad_f64(hb["s"], hb["s2"], hb["actions"], hb["rewards"], hb["dones"], hb["valid"], local, target,
                     is_weights=hb["is_weights"], **kw)
    P = L.P
    raw, abs_td, parts, nblk = run_whole(L, ring, B, None if source == "draw" else idx, isw, img, seed=11, counter=seed)
    if r["near_tie"].any():
        # a DDQN argmax within tie_eps may go either way: read the kernel's choice back from its |TD error| and hold it to that
        nt = r["near_tie"]
        alt = np.abs(abs_td - np.abs(r["delta_alt"])) < np.abs(abs_td - r["abs_td"])
        na = np.where(nt, np.where(alt, r["a_alt"], r["a_next"]), -1)
        r = dqn_grad_f64(hb["s"], hb["s2"], hb["actions"], hb["rewards"], hb["dones"], hb["valid"], local, target,
                         is_weights=hb["is_weights"], next_action=na, **kw)
        kw["next_action"] = na
    ok_a, ra = check_a(raw, abs_td, r, P, bars)
    assert ok_a, (form, B, kind, "a", ra, raw[P + 1], r["count"])
    if huber:
        assert (r["abs_td"] < 1).any() and (r["abs_td"] > 1).any()
    if source == "tie":
        assert kind != "dqn" and np.all(r["a_next"] == 0)
    tiles, abs_t = run_tiles(L, ring, B, idx, isw, img)
    ok_b, rb = check_b(raw.astype(np.float64), tiles, abs_td, abs_t, r, P)
    assert ok_b, (form, B, kind, "b", rb)
    WORST[form] = max(WORST.get(form, 0.0), ra)
    WORST[form + "/b"] = max(WORST.get(form + "/b", 0.0), rb)
    if source == "invalid":
        inv = np.flatnonzero(ring.host["valid"][0] == 0)
        assert len(inv) > 0
        h = ring.host
        rows = pool().rows
        h["obs"][0, inv] = rows[rng.integers(0, len(rows), len(inv))]
        h["obs"][1, inv] = rows[rng.integers(0, len(rows), len(inv))]
        h["action"][0, inv] = (h["action"][0, inv] + 1) % A
        h["reward"][0, inv] = -h["reward"][0, inv] + 17.0
        h["done"][0, inv] = 1 - h["done"][0, inv]
        ring.upload()
        raw2, abs2, _, _ = run_whole(L, ring, B, idx, isw, img)
        assert np.array_equal(raw2, raw), "invalid rows changed the bucket"
        vs = hb["valid"] != 0
        assert np.array_equal(abs2[vs], abs_td[vs])
    if B >= 16384:
        mutations(r, raw, abs_td, tiles, abs_t, hb, local, target, kw, bars, P, B, f16)
    return dict(L=L, parts=parts, nblk=nblk, raw=raw, r=r, f16=f16, bars=bars)


def mutations(r, raw, abs_td, tiles, abs_t, hb, local, target, kw, bars, P, B, f16):
    """(c): perturbations of the f64 side.  f32-accuracy forms: (a) ALONE must reject each -- one sample's gradient and loss
    dropped or duplicated (the count left as it is: the bug a kernel shares across all its tiles), the gradient scaled by
    (1 + 1/B), the count off by one.  f16 forms: tau = 2^-10 cannot resolve one sample or a 1/B scale at B >= 16 384; (a) must
    reject the count, and a dropped or duplicated sample must be rejected by (a) or (b) (a tile-local bug)."""
    # the sample: the valid one of median |dq| (a sample whose delta is near zero contributes nothing any check could see)
    vi = np.flatnonzero(hb["valid"] != 0)
    w = np.abs(r["abs_td"][vi] if not kw["huber"] else np.minimum(r["abs_td"][vi], 1.0))
    if hb["is_weights"] is not None:
        w = w * hb["is_weights"][vi]
    i = int(vi[np.argsort(w, kind="stable")[len(vi) // 2]])
    c = sample_contribution(hb, i, local=local, target=target, **kw)
    cvec = np.concatenate([c["grad"], [c["loss"], 0.0]])

    def with_(r, d):
        q = dict(r)
        q["grad"], q["loss"], q["count"] = r["grad"] + d[:P], r["loss"] + d[P], r["count"] + d[P + 1]
        return q
    scale = np.zeros(P + 2)
    scale[:P] = r["grad"] / B
    cnt = np.zeros(P + 2)
    cnt[P + 1] = 1.0
    for name, d in (("drop", -cvec), ("dup", cvec), ("scale", scale), ("count", cnt)):
        ok_a = check_a(raw, abs_td, with_(r, d), P, bars)[0]
        if not f16 or name == "count":
            assert not ok_a, ("(a) does not reject", name)
        elif name != "scale":
            assert not (ok_a and check_b(raw.astype(np.float64), tiles + d, abs_td, abs_t, r, P)[0]), ("not rejected", name)


# (form, B, kind, huber, weighted, source): every form sees every kind, both losses, with and without weights; the bench form
# (p8i, dqn, mse, 16 384, drawn) sees all of them
CASES = [
    ("p8", 64, "dqn", False, False, "hand"), ("p8", 128, "ddqn", True, True, "hand"), ("p8", 2368, "dueling", False, True, "hand"),
    ("p8", 16384, "dqn", True, False, "hand"), ("p8", 16448, "ddqn", False, True, "hand"),
    ("p8", 40960, "dueling", True, False, "hand"), ("p8", 65536, "dqn", False, True, "hand"),
    ("p8", 128, "dueling", False, False, "tie"), ("p8", 16448, "ddqn", True, True, "invalid"),
    ("p8i", 64, "ddqn", False, True, "hand"), ("p8i", 128, "dueling", True, False, "hand"), ("p8i", 2368, "dqn", True, True, "hand"),
    ("p8i", 16384, "dqn", False, False, "draw"), ("p8i", 16384, "dqn", False, True, "draw"),
    ("p8i", 16384, "dqn", True, False, "draw"), ("p8i", 16384, "ddqn", True, True, "draw"),
    ("p8i", 16384, "dueling", False, True, "draw"), ("p8i", 16448, "dqn", False, False, "hand"),
    ("p8i", 40960, "ddqn", True, True, "hand"), ("p8i", 65536, "dueling", False, False, "hand"),
    ("p8i", 2368, "ddqn", False, False, "tie"), ("p8i", 2368, "dqn", False, True, "invalid"),
    ("h8p", 64, "dqn", False, False, "hand"), ("h8p", 2368, "ddqn", True, True, "hand"), ("h8p", 16448, "dueling", False, True, "hand"),
    ("h8p", 65536, "dqn", True, False, "hand"), ("h8p", 2368, "dueling", True, False, "invalid"),
    ("h8f", 64, "dueling", True, True, "hand"), ("h8f", 2368, "dqn", False, False, "hand"), ("h8f", 16448, "ddqn", False, True, "hand"),
    ("h8f", 65536, "ddqn", True, False, "hand"), ("h8f", 2368, "ddqn", False, False, "tie"),
    ("g32", 64, "ddqn", True, False, "hand"), ("g32", 2368, "dueling", False, True, "hand"), ("g32", 16448, "dqn", True, True, "hand"),
    ("g16", 64, "dqn", False, True, "hand"), ("g16", 2368, "ddqn", True, False, "hand"), ("g16", 16448, "dueling", False, True, "hand"),
    ("g32n", 64, "dqn", False, False, "hand"), ("g32n", 2368, "dueling", True, True, "hand"), ("g32n", 16448, "ddqn", False, False, "hand"),
    ("g32n", 2368, "dueling", False, False, "tie"),
    ("g16n", 64, "dueling", False, True, "hand"), ("g16n", 2368, "dqn", True, False, "hand"), ("g16n", 16448, "ddqn", True, True, "hand"),
    ("g16n", 2368, "ddqn", False, False, "invalid"),
    ("pn", 64, "ddqn", False, True, "hand"), ("pn", 2368, "dqn", True, False, "hand"), ("pn", 16448, "dueling", False, True, "hand"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_raw_bucket_against_f64(case):
    form, B, kind, huber, weighted, source = case
    out = run_case(form, B, kind, huber, weighted, source, seed=CASES.index(case) + 1)
    print(case, "worst ratios", {k: round(v, 4) for k, v in WORST.items() if k.split("/")[0] == form})
    if B in (16384, 65536) and source in ("draw", "hand") and not out["f16"]:
        reduce_adam(out, hard=B == 65536)


def reduce_adam(out, hard):
    """(d): uavenv_dqn_reduce_adam with raw_out, from non-zero moments at epoch 5.  Its raw_out against uavenv_dqn_reduce's (the f32
    summation bound); loss_out = loss sum / count bit for bit; m, v, w against adam_step_f64 on raw / count -- the bucket (a)
    tied to f64, so only the step's own f32 rounding is allowed, and a divide by count +- 1 must be rejected."""
    L, r, raw, P = out["L"], out["r"], out["raw"], out["L"].P
    rng = np.random.default_rng(5)
    gbar = r["grad"] / r["count"]
    m0 = (gbar * rng.choice([-1.0, 1.0], P) * rng.uniform(0.5, 1.5, P)).astype(np.float32)
    v0 = (gbar * gbar * rng.uniform(0.5, 2.0, P)).astype(np.float32)
    with torch.no_grad():
        L.flat[2].copy_(torch.tensor(m0))
        L.flat[3].copy_(torch.tensor(v0))
        L.flat[1].copy_(L.flat[1] + 1.0)               # so that a hard copy is visible
    w0 = L.flat[0].cpu().numpy().astype(np.float64)
    t0 = L.flat[1].cpu().numpy()
    loss = torch.empty((), device="cuda")
    raw2 = torch.empty(P + 2, device="cuda")
    lr, betas, eps, t = 1e-3, (0.9, 0.999), 1e-8, 5
    assert L.lib.uavenv_dqn_reduce_adam(C.byref(L.net), out["parts"].data_ptr(), out["nblk"], lr, betas[0], betas[1], eps, t,
                                        1 if hard else 0, loss.data_ptr(), raw2.data_ptr(), L._stream()) == 0
    torch.cuda.synchronize()
    raw2 = raw2.cpu().numpy()
    assert np.all(np.abs(raw2[:P] - raw[:P]) <= PART * r["M"] + 1e-30) and raw2[P + 1] == raw[P + 1]
    assert abs(raw2[P] - raw[P]) <= PART * r["M_loss"]
    cnt = np.float32(raw2[P + 1])
    assert float(loss) == float(np.float32(raw2[P]) * (np.float32(1.0) / max(cnt, np.float32(1.0))))
    g_k = raw2[:P].astype(np.float64)
    n = float(raw2[P + 1])
    f = L.flat.cpu().numpy().astype(np.float64)
    ok, worst = check_adam(f, w0, m0, v0, g_k / n, 2.0 ** -23 * np.abs(g_k / n), t, lr, betas, eps, hard)
    assert ok, worst
    for dn in (-1.0, 1.0):                             # (c) for the divide: count off by one is rejected
        assert not check_adam(f, w0, m0, v0, g_k / (n + dn), 2.0 ** -23 * np.abs(g_k / n), t, lr, betas, eps, hard)[0], dn
    check_target(L, t0, hard)


def check_target(L, t0, hard):
    if hard:
        assert np.array_equal(L.flat[1].cpu().numpy().view(np.uint32), L.flat[0].cpu().numpy().view(np.uint32))
    else:
        assert np.array_equal(L.flat[1].cpu().numpy(), t0)


def check_adam(f, w0, m0, v0, gbar, gerr, t, lr, betas, eps, hard):
    """The kernels' m, v, w (rows 2, 3, 0 of f) after one step against adam_step_f64 on the mean gradient gbar, with the
    hyperparameters as the kernel receives them (f32).  Returns (ok, worst ratio).  Per component: gerr (the mean gradient's
    error bound) carried through the step to first order, plus f32 rounding -- of each stored value, and of the bias corrections:
    bc2 = 1 - powf(beta2, t) is 0.005 at t = 5, so the 2^-24 rounding of powf is 2^-24 / bc2 relative in bc2 and half that in
    the step.  And the projection of the error in m on the gradient (a scale error in the mean, e.g. a wrong count), against K
    root-sum-squares of the per-component bars: every component's step is separate arithmetic."""
    lr, betas, eps = float(np.float32(lr)), (float(np.float32(betas[0])), float(np.float32(betas[1]))), float(np.float32(eps))
    w1, m1, v1, _ = adam_step_f64(w0, m0, v0, gbar, t, lr, betas, eps, hard)
    m_bar = (1 - betas[0]) * gerr + 2.0 ** -21 * (np.abs(m0) + np.abs(gbar)) + 1e-38
    v_bar = 2 * (1 - betas[1]) * np.abs(gbar) * gerr + (1 - betas[1]) * gerr ** 2 + 2.0 ** -21 * (v0 + (1 - betas[1]) * gbar ** 2) + 1e-38
    bc1, bc2 = 1 - betas[0] ** t, 1 - betas[1] ** t
    den = np.sqrt(v1) / np.sqrt(bc2) + eps
    step = (lr / bc1) * np.abs(m1) / den
    rel = m_bar / np.maximum(np.abs(m1), 1e-38) + 0.5 * (v_bar / np.maximum(v1, 1e-38)) * (np.sqrt(v1) / np.sqrt(bc2)) / den + 2.0 ** -23 / bc2 + 2.0 ** -21
    w_bar = np.minimum(step * rel, (lr / bc1) * (np.abs(m1) + m_bar) / max(eps, 1e-38)) + 2.0 ** -23 * np.abs(w1) + 1e-38
    u = (1 - betas[0]) * gbar
    rs = abs(float((f[2] - m1) @ u)) / (K * float(np.sqrt(np.sum((m_bar * u) ** 2))) + 1e-300)
    worst = max((np.abs(f[2] - m1) / m_bar).max(), (np.abs(f[3] - v1) / v_bar).max(), (np.abs(f[0] - w1) / w_bar).max(), rs)
    return bool(worst <= 1.0), float(worst)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("b", [1, 63, 65, 1000])
def test_padded_learn_against_f64(b, weighted):
    """(e): FusedDQNLearner.learn / learn_weighted on b real samples, after a full call of the same padded size (so the pad rows
    hold stale data), from non-zero moments: the f64 bucket over the b samples + adam_step_f64, with (a)'s bar on the mean
    gradient; the mean over b - 1 or b + 1 samples must be rejected (b = 1: over 2 -- a count of 0 divides by 1)."""
    kind = ("dqn", "ddqn", "dueling")[b % 3]
    L = make_learner("g32", kind, b == 65, 100 + b)
    rng = np.random.default_rng(b)
    rows = pool().rows
    bp = (b + 63) // 64 * 64

    def batch(k):
        return dict(states=torch.tensor(rows[rng.integers(0, len(rows), k)]).cuda(),
                    next_states=torch.tensor(rows[rng.integers(0, len(rows), k)]).cuda(),
                    actions=torch.tensor(rng.integers(0, 3, k)).cuda(),
                    rewards=torch.tensor(rng.normal(0, 50, k).astype(np.float32)).cuda(),
                    dones=torch.tensor((rng.random(k) < 0.2).astype(np.float32)).cuda())
    first = batch(bp)
    if weighted:
        L.learn_weighted(first, torch.rand(bp, device="cuda"))
    else:
        L.learn(first)
    bt = batch(b)
    isw = torch.tensor(rng.uniform(0.1, 1.0, b).astype(np.float32)).cuda() if weighted else None
    local, target = ref_params(L, False)
    r = dqn_grad_f64(bt["states"].cpu().numpy(), bt["next_states"].cpu().numpy(), bt["actions"].cpu().numpy(),
                     bt["rewards"].cpu().numpy(), bt["dones"].cpu().numpy(), np.ones(b), local, target,
                     is_weights=None if isw is None else isw.cpu().numpy(), kind=kind, dueling=kind == "dueling", n_actions=3,
                     gamma=float(np.float32(GAMMA)), huber=b == 65, relu_eps=F32["relu_eps"], tie_eps=F32["tie_eps"])
    gbar = r["grad"] / r["count"]
    m0 = (gbar * rng.choice([-1.0, 1.0], L.P) * rng.uniform(0.5, 1.5, L.P)).astype(np.float32)
    v0 = (gbar * gbar * rng.uniform(0.5, 2.0, L.P)).astype(np.float32)
    with torch.no_grad():
        L.flat[2].copy_(torch.tensor(m0))
        L.flat[3].copy_(torch.tensor(v0))
    L.epoch = 4 if b != 1000 else 5                    # step 5 (no copy) or 6 (hard copy)
    t = L.epoch + 1
    w0, t0 = L.flat[0].cpu().numpy().astype(np.float64), L.flat[1].cpu().numpy()
    if weighted:
        loss, abs_err = L.learn_weighted(bt, isw)
        assert np.all(np.abs(abs_err.cpu().numpy() - r["abs_td"]) <= F32["tau_td"] * r["q_abs"] + r["td_amb"])
    else:
        loss = L.learn(bt)
    torch.cuda.synchronize()
    l_bar = F32["tau"] * r["M_loss"] + K * F32["tau_td"] * np.sqrt(r["N2_loss"]) + r["Z_loss"]
    assert abs(float(loss) - r["loss"] / b) <= l_bar / b + 2.0 ** -22 * abs(float(loss))
    gerr = (F32["tau"] * r["M"] + K * F32["tau_td"] * np.sqrt(r["N2"]) + r["Z"]) / r["count"] + 2.0 ** -23 * np.abs(gbar)
    f = L.flat.cpu().numpy().astype(np.float64)
    ok, worst = check_adam(f, w0, m0, v0, gbar, gerr, t, L.lr, L.betas, L.eps, t % 3 == 0)
    assert ok, worst
    for n in ((2,) if b == 1 else (b - 1, b + 1)):
        assert not check_adam(f, w0, m0, v0, r["grad"] / n, gerr, t, L.lr, L.betas, L.eps, t % 3 == 0)[0], n
    check_target(L, t0, t % 3 == 0)


# --- A/B knob forms: read once per process, so each runs in a fresh child, one after another, under its own time limit -------
KNOBS = [
    ("UAVENV_STAGE_VGPR", "1", [("p8i", 128, "ddqn", True, True, "hand"), ("p8i", 16448, "dqn", False, False, "hand")]),
]

CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
torch.cuda.set_device(0)
import test_dqn_grad_kernels_gpu as T
for k, case in enumerate(eval(sys.argv[2])):
    T.run_case(*case, seed=1000 + k)
print("knob worst ratios", T.WORST)
"""


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: k[0])
def test_knob_forms_against_f64(knob):
    name, val, cases = knob
    env = {k: v for k, v in os.environ.items() if not k.startswith("UAVENV_")}
    env[name] = val
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, ROOT, repr(cases)], env=env, check=True,
                   timeout=330)
