"""The fused SAC update kernels of csrc/sac.hip -- k_sac_td, k_sac_critic_grad, k_sac_actor_grad, k_sac_reduce_adam, k_sac_act -- held
against the float64 statement of oracle/sac_grad_ref.py at the RAW partial-row bucket, through the C ABI (FusedSACLearner.critic_grad
/ actor_grad, uavenv_sac_reduce, uavenv_sac_*_adam, the *_multi entry points), so the weights never move between checks.

Nets per case: freshly initialised (targets and critics decorrelated), or a STRESS actor (oracle.sac_grad_ref.stress_actor, tuned on
the pool's rows): asserted on the host before the launch, over (sample, action dimension) pairs, >= 5 % with fc_std(x) > 20 and
>= 5 % of the same dimension below 20, >= 5 % with sd < 0.01, >= 5 % with 0.01 <= sd < 0.9, >= 5 % with |fc_mu(x)| > 3, none with
fc_std(x) < -12 (below that f32 sd^2 heads for underflow and the reference's formula is undefined too: out of scope).

Per case:
 (a) accuracy against f64, per component p of the summed rows (gradients, loss columns, sum log pi alike):
        |raw_p - g_p| <= tau M_p + K tau_td sqrt(N2_p) + Z_p + tau_split T_p + tau_c C_p
     and the TD targets (UavSacBatch.td_scratch, read back) and abs_td per sample to tau_td times their scale, the valid fraction
     (see below), and the projection of the error on the gradient's last-layer block (the direction of a uniform scale error):
        |<raw - g, g>| <= K sqrt(sum_p (sig M_p g_p)^2 + sum_s (sig_td sens_s)^2 + sum_s zs_s^2) + 2 K max(2^-24 max(.), max zs)
     Derivation, u = 2^-24, every term rounded once (as tests/test_dqn_grad_kernels_gpu.py):
       forward: layer 1 sums 103 terms (the split two-term f16 form is exact per product: fc1 as hi + mid carries 22 bits, 2^-22 =
       4 u relative to the row's largest weight, the flags are exact), the 64 -> 64 layer 65, the head 65, the target a few:
       |err q| <= 240 u q_abs < 2^-16 q_abs -> tau_td = relu_eps = tie_eps = 2^-16 for Q, for y (y_abs adds |r| and alpha lp_abs) and
       for the actor's head pre-activations; their standard deviation under round-to-nearest <= sqrt(240 / 3) u < 2^-20 = sig_td.
       log pi: tanhf, expf, log1pf, logf are within ~2 ulp each: 16 u of the magnitude of its terms (weight 2^-4 in lp_abs); ns - mu
       amplifies the one rounding of ns by |eps| / sd (weight 2^-7); the pre-activations' errors at full weight through d lp / d(m, s).
       backward: a gradient term is a product of three or four f32 values each within ~70 u of exact, summed over the batch in f32
       (a random walk of ~300 roundings on partial sums <= M): tau = 2^-17; standard deviation < 4 u M = 2^-21 M = sig.
       split dW1 (wgrad_x_split): dH1 as hi + mid 2^-11 of dH1 2^S with 2^S from the TILE's largest |dH1|: each flag-column product
       is exact to 2^-22 of that maximum: tau_split = 2^-22 on T_p = sum over tiles of (tile max |dH1|) x (samples with the flag).
       1 - tanh^2 of a saturated tanh (|fc_mu| > 3, sd -> 1) has an absolute error of ~4 u of the 1 (tanhf's 2 ulp, doubled by the
       square): tau_c = 2^-21 on C_p = M_p with every 1 - x^2 replaced by 1 + x^2 (actor phase only).
     Valid fraction: the kernel sums fl(count_wg * fl(1 / B)) over the workgroups in f32.  For B a power of two every partial sum is
     exact: asserted EXACTLY.  Otherwise fl(1 / B) is inexact and the sums round: |err| <= (rows / 4 + 4) u (the reduction's four
     row groups) -- a finding of this module: "exact" cannot hold for 2 368 or 16 448, and the bound stays far below 1 / B.
 (b) partition invariance: the same batch with tiles_per_wg = 1, 3, 8 (ragged last workgroup; k_sac_td's halves walk odd and single
     tile counts): partial rows summed in f64 differ by f32 summation order only (2^-20 M_p; the valid fraction as above), TD
     targets and abs_td bit for bit.
 (c) B >= 16 384, host only: the f64 side with one sample dropped / duplicated (the valid sample of median |contribution|), the
     gradient scaled by 1 + 1/B, the valid count off by one: (a) ALONE must reject each, in both phases.  On the stress cases also
     the oracle with one switch flipped (a1 := a0 in the target critics, max for min, log pi without - log sd, one tanh in the
     correction): (a) must reject each in every phase it reaches (a1 := a0: the critic phase only).
     Z never decides a mutation: these batches are SETTLED on the host before the launch (settle()): every sample the oracle marks
     ambiguous is drawn again until none is left, so Z = 0 there.  (With three nets of 64-unit layers per phase ~4 % of the samples
     hold some ReLU within relu_eps and ~1 % a |Q1 - Q2| within tie_eps; each such sample's share may flow another way, and that
     allowance is 100 to 1 000 times the rounding bars -- measured on the host: with it no 1 / B scale error is visible in the actor
     phase.)  The smaller cases keep their ambiguous samples and their Z.
 (d) k_sac_reduce_adam from non-zero moments at step 5 against sac_adam_f64 (check_adam's bars): both critics, the soft update with
     tau = 0.05 on targets offset beforehand, the actor, log_alpha, alpha_mv; a valid fraction off by one sample is rejected.
     25 % invalid rows, one whole 64-sample tile invalid (split_scale(0)), and an all-invalid batch (nothing non-finite).
 (e) invalid rows are inert (rewritten with other finite values: partial rows bit-identical).
 (f) records vs planes on a real ring with attach_action1: bit-identical partial rows in both phases.
 (g) *_grad_multi with 4 slots of different batch sizes and pins (grids 1, 13, 8, 1: three slots take the early return), different
     nets per slot: bit-identical to the single-slot launches, rows beyond a slot's grid untouched; *_adam_multi bit-identical to
     the single calls.
 (h) k_sac_act on the stress actor (ragged count, strided rows) against actor_head_f64; its bar is oracle.sac_grad_ref.act_bar, which
     tests/test_sac_act_kernels_gpu.py holds the batched launch to at every slot count and tile trip.
 (i) UAVENV_SAC_FUSED_TD=1 in-process against f64; UAVENV_SAC_WGS in a fresh child.
Ambiguity cap, asserted on the host before the launch (the batch's seed is the first that meets it): ReLU pre-activations within
relu_eps of zero at most 1 % of (sample, unit) pairs, |Q1 - Q2| within tie_eps at most 1 % of (sample, output column) pairs.  (Not "1 %
of the samples with any ambiguous unit": at the derived relu_eps that is ~4 % for ANY batch of these nets, no seed changes it.)
Worst measured error / bar on an MI355X over the cases below (printed with -s; the module takes 35 s):
  k_sac_td 0.30 (TD targets; stress actors -- fresh ones 0.002)      abs_td 0.003
  k_sac_critic_grad (a) 0.15, direction 0.03, (b) 0.42               with UAVENV_SAC_FUSED_TD=1: 0.03 / 0.02
  k_sac_actor_grad  (a) 0.39, direction 0.03, (b) 0.48               k_sac_act 0.10          k_sac_reduce_adam 0.50
  UAVENV_SAC_WGS children: critic 0.08, TD 0.10, actor 0.014, (b) 0.07 / 0.13            the real ring (f): 0.02 / 0.30 / 0.004
Mutations (c), error / bar (critic phase, actor phase), smallest over the eight batches of 16 384 .. 65 536 (unmutated: above):
  drop 2.15, 2.17   duplicate 2.15, 2.16   scale 3.67, 2.19   count: ~15 at B = 16 448 (1 / B against 68 u), infinite at a power of two
  a1 := a0 27.4 (critic)   max for min 8 412, 744   no - log sd 1 541, 559 579   one tanh 292, 2 417
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.sac_grad_ref import (MUTS, PA, PC, act_bar, actor_forward, assert_stress, sac_actor_bucket_f64, sac_adam_f64,
                                 sac_critic_bucket_f64, sample_contribution, stress_actor)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM = {"actor": {"NetWork": "PolicyNetContinuous_SAC", "w": "100", "action_bound": "1", "hiden_dim": "64", "output": "2", "lr": "0.0001"},
         "critic": {"NetWork": "QValueNetContinuous_SAC", "w": "100", "hiden_dim": "64", "action_dim": "2", "lr": "0.001"},
         "SAC_param": {"IS_Continuous": "1", "alpha_lr": "0.0001", "target_entropy": "1", "gamma": "0.99", "tau": "0.05"}}
GAMMA = float(np.float32(0.99))
BARS = dict(tau=2.0 ** -17, tau_td=2.0 ** -16, relu_eps=2.0 ** -16, tie_eps=2.0 ** -16, sig=2.0 ** -21, sig_td=2.0 ** -20,
            tau_split=2.0 ** -22, tau_c=2.0 ** -21)
PART = 2.0 ** -20
K = 6.0
U = 2.0 ** -24
WORST = {}
FC, FA = 2 * PC + 2, PA + 2          # the valid-fraction columns


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


def note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


class Pool:
    """A real continuous-action ring (2 UAVs per env, packed rows, attach_action1) that has wrapped: the source of every observation
    row, and the ring of (f)."""

    def __init__(self):
        from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
        from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
        self.env = env = make_city26_env(1024, uav_per_env=2, obs_dtype="packed")
        self.ring = ring = DeviceReplayRing(env, 4 * env.N, discrete=False)
        assert ring.frames == 5
        ring.reset(seed=4)
        self.a1 = torch.zeros((ring.frames, env.N), dtype=torch.float32, device="cuda")
        ring.attach_action1(self.a1)
        gen = torch.Generator(device="cuda").manual_seed(1)
        for _ in range(8):
            ring.current_action().copy_(torch.rand(env.N, generator=gen, device="cuda") * 2 - 1)
            self.a1[ring.head].copy_(torch.rand(env.N, generator=gen, device="cuda") * 2 - 1)
            ring.step_env(auto_reset=True)
        torch.cuda.synchronize()
        assert ring.filled == 4
        self.packed = ring.obs.view(-1, ring.obs.shape[-1])
        L = _lib()
        out = torch.empty((self.packed.shape[0], 100), dtype=torch.float32, device="cuda")
        assert L.load().uavenv_obs_unpack(self.packed.data_ptr(), self.packed.shape[0], out.data_ptr(), L.OBS_F32,
                                          torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        self.rows = out.cpu().numpy()


_POOL = None


def pool():
    global _POOL
    if _POOL is None:
        _POOL = Pool()
    return _POOL


@pytest.fixture(scope="module", autouse=True)
def _release_pool():
    global _POOL
    yield
    print("SAC kernels, worst error / bar:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    if _POOL is not None:
        _POOL.env.close()
        _POOL = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class Hand:
    """F frames of n agents: packed observation rows copied from the pool, hand-made action / reward / done / valid planes and the
    16-byte records {a1, a0, reward, done | valid << 8} that describe the same transitions."""

    def __init__(self, n, rng, invalid=0.0, F=3):
        p = pool()
        self.n, self.F = n, F
        R = F * n
        self.src = rng.integers(0, len(p.rows), R)
        k = rng.random(R)
        reward = np.where(k < 0.05, 194.0, np.where(k < 0.10, -200.0, rng.normal(-3.0, 5.0, R)))
        self.h = dict(obs=p.rows[self.src].copy(), act0=rng.uniform(-1, 1, R).astype(np.float32), act1=rng.uniform(-1, 1, R).astype(np.float32),
                      reward=reward.astype(np.float32), done=(rng.random(R) < 0.2).astype(np.uint8),
                      valid=(rng.random(R) >= invalid).astype(np.uint8))
        self.obs = p.packed[torch.tensor(self.src, device="cuda")].contiguous()
        self.t = {}
        self.upload()

    def upload(self):
        h = self.h
        for k in ("act0", "act1", "reward", "done", "valid"):
            v = torch.tensor(h[k]).cuda()
            if k in self.t:
                self.t[k].copy_(v)
            else:
                self.t[k] = v.contiguous()
        m = np.stack([h["act1"].view(np.int32), h["act0"].view(np.int32), h["reward"].view(np.int32),
                      h["done"].astype(np.int32) | (h["valid"].astype(np.int32) << 8)], 1)
        if "meta" in self.t:
            self.t["meta"].copy_(torch.tensor(m).cuda())
        else:
            self.t["meta"] = torch.tensor(m).cuda().contiguous()

    def set_obs(self, rows_idx, src_idx):
        p = pool()
        self.h["obs"][rows_idx] = p.rows[src_idx]
        self.obs[torch.tensor(rows_idx, device="cuda")] = p.packed[torch.tensor(src_idx, device="cuda")]


def make_learner(seed, stress, log_alpha):
    from dqn_based_uav_3d_path_planer_amd.sac import FusedSACLearner
    torch.manual_seed(seed)
    L = FusedSACLearner(PARAM)
    with torch.no_grad():
        for blk in (2, 3):
            L._cblocks[blk, :PC].add_(0.01 * torch.randn(PC, device="cuda"))
        if stress:
            f = stress_actor(L._blocks[0].cpu().numpy(), pool().rows)
            L._blocks[0, :PA].copy_(torch.tensor(f.astype(np.float32)).cuda())
        L.log_alpha.fill_(float(log_alpha))
    return L


def params_of(L):
    a = L._blocks[0].cpu().numpy().astype(np.float64)
    c = L._cblocks[:4].cpu().numpy().astype(np.float64)
    return a, [c[0], c[1]], [c[2], c[3]], float(L.log_alpha.cpu().numpy().astype(np.float64))


class Case:
    """One batch on a Hand ring (or the pool's real ring), its device description and its host copy."""

    def __init__(self, L, B, rng, form, weighted, ring=None, invalid=0.0, use_meta=False, uav=2):
        self.L, self.B, self.form = L, B, form
        real = ring is not None
        if not real:
            n = max(256, min(B, 4096))
            ring = Hand(n, rng, invalid)
        self.ring = ring
        if real:
            p = pool()
            r = p.ring
            F, n = r.frames, p.env.N
            planes = dict(act0=r.action.view(-1), act1=p.a1.view(-1), reward=r.reward.view(-1), done=r.done.view(-1), valid=r.valid.view(-1),
                          meta=r.meta.view(-1, 4))
            obs_dev, obs_host = p.packed, p.rows
            host = {k: planes[k].cpu().numpy() for k in ("act0", "act1", "reward", "done", "valid")}
            back = (r.head - 1 - rng.integers(0, r.filled, B)) % F          # complete transitions only
            f = back
        else:
            F, n = ring.F, ring.n
            planes, obs_dev, obs_host, host = ring.t, ring.obs, ring.h["obs"], ring.h
            f = rng.integers(0, F, B)
        self.planes, self.obs_dev = planes, obs_dev
        self.F, self.n, self.uav, self.real = F, n, uav, real
        self.obs_host, self.planes_host = obs_host, host
        if form == "draws":
            self.slot = int(rng.integers(0, uav))
            e = rng.integers(0, n // uav, B)
            self.fe = np.stack([f, e], 1).astype(np.int32)
            assert (f == F - 1).any() or real                                # some s' wrap to frame 0
            self.draws = torch.tensor(self.fe).cuda().contiguous()
            kw = dict(draws=self.draws, n_agents=n, uav_per_env=uav, slot=self.slot, frames=F)
        else:
            self.ix = np.stack([rng.integers(0, n, B), rng.integers(n, F * n, B)], 1).astype(np.int32)   # s from frame 0, s' from the others
            self.idx_s, self.idx_n = (torch.tensor(self.ix[:, k].copy()).cuda().contiguous() for k in (0, 1))
            kw = dict(idx_s=self.idx_s, idx_n=self.idx_n)
        self._rows()
        self.isw = torch.tensor(rng.uniform(0.05, 1.0, B).astype(np.float32)).cuda() if weighted else None
        self.abs_td = torch.full((B,), -1.0, device="cuda")
        eps = rng.normal(size=(2, B, 2)).astype(np.float32)
        self.eps = [torch.tensor(eps[0]).cuda().contiguous(), torch.tensor(eps[1]).cuda().contiguous()]
        self.kw = dict(kw, valid=planes["valid"], is_weights=self.isw, abs_td_out=self.abs_td)
        self.use_meta = use_meta
        self.b = self.batch(use_meta)
        self.host = dict(eps_next=eps[0], eps_cur=eps[1], is_weights=None if self.isw is None else self.isw.cpu().numpy())
        self.rehost()

    def _rows(self):
        if self.form == "draws":
            f, e = self.fe[:, 0].astype(np.int64), self.fe[:, 1].astype(np.int64)
            self.rs, self.rn = f * self.n + e * self.uav + self.slot, ((f + 1) % self.F) * self.n + e * self.uav + self.slot
        else:
            self.rs, self.rn = self.ix[:, 0].astype(np.int64), self.ix[:, 1].astype(np.int64)

    def redraw(self, mask, rng):
        """Other transitions and other rsample() draws for the samples of `mask` (host and device)."""
        k = int(mask.sum())
        if self.form == "draws":
            f = self.fe[mask, 0] if self.real else rng.integers(0, self.F, k)
            self.fe[mask] = np.stack([f, rng.integers(0, self.n // self.uav, k)], 1)
            self.draws.copy_(torch.tensor(self.fe).cuda())
        else:
            self.ix[mask] = np.stack([rng.integers(0, self.n, k), rng.integers(self.n, self.F * self.n, k)], 1)
            self.idx_s.copy_(torch.tensor(self.ix[:, 0].copy()).cuda())
            self.idx_n.copy_(torch.tensor(self.ix[:, 1].copy()).cuda())
        for j in (0, 1):
            key = ("eps_next", "eps_cur")[j]
            self.host[key][mask] = rng.normal(size=(k, 2)).astype(np.float32)
            self.eps[j].copy_(torch.tensor(self.host[key]).cuda())
        self._rows()
        self.rehost()

    def batch(self, use_meta, tiles_per_wg=0):
        p = self.planes
        return self.L.make_batch(self.obs_dev, p["act0"], p["act1"], p["reward"], p["done"], meta=p["meta"].view(-1) if use_meta else None,
                                 tiles_per_wg=tiles_per_wg, **self.kw)

    def rehost(self):
        h, o = (self.ring.h, self.ring.h["obs"]) if not self.real else (self.planes_host, self.obs_host)
        self.host.update(s=o[self.rs], s2=o[self.rn], actions=np.stack([h["act0"][self.rs], h["act1"][self.rs]], 1),
                         rewards=h["reward"][self.rs], dones=h["done"][self.rs], valid=h["valid"][self.rs])


def run_phase(L, b, eps, critic):
    """-> (column sums by uavenv_sac_reduce [stride] f32, partial rows [rows, stride] clone, td [B, 2] or None, abs_td or None)"""
    parts = L.critic_grad(b, eps) if critic else L.actor_grad(b, eps)
    rows = L._rows_launched
    stride = parts.shape[1]
    raw = torch.empty(stride, device="cuda")
    assert L.lib.uavenv_sac_reduce(parts.data_ptr(), rows, stride, raw.data_ptr(), L._stream()) == 0
    torch.cuda.synchronize()
    return raw.cpu().numpy(), parts[:rows].clone(), rows


def frac_ratio(got, count, B, rows):
    """The valid-fraction column as error / bound: B a power of two -> exact (any difference is infinitely far out)."""
    want = count / B
    if B & (B - 1) == 0:
        return 0.0 if got == np.float32(want) else float("inf")
    return abs(float(got) - want) / ((rows / 4 + 4) * U * want + 1e-38)


def proj_ratio(e, g, sens):
    sm, sd = sens[0], sens[1]
    var = np.sum((BARS["sig"] * sm) ** 2) + np.sum((BARS["sig_td"] * sd) ** 2)
    b_max = U * max(float(sm.max()), float(sd.max()))
    if len(sens) > 2:
        var += np.sum(sens[2] ** 2)
        b_max = max(b_max, float(sens[2].max()))
    return abs(float(e @ g)) / (K * np.sqrt(var) + 2 * K * b_max + 1e-300)


def bar_of(r):
    b = BARS["tau"] * r["M"] + K * BARS["tau_td"] * np.sqrt(r["N2"]) + r["Z"] + BARS["tau_split"] * r["T"] + 1e-30
    return b + BARS["tau_c"] * r["C"] if "C" in r else b


def check_critic(raw, td, abs_td, r, B, rows):
    """(a) for the critic phase -> (ok, dict of ratios)."""
    e = raw.astype(np.float64) - r["row"]
    rg = np.abs(e[:FC]) / bar_of(r)[:FC]
    rt = np.abs(td - r["y"]) / (BARS["tau_td"] * r["y_abs"] + 1e-30)
    ra = np.abs(abs_td - r["abs_td"]) / (BARS["tau_td"] * r["abs_td_scale"] + 1e-30)
    g = np.zeros(2 * PC + 4)
    for k in range(2):
        g[k * PC + PC - 130:(k + 1) * PC] = r["row"][k * PC + PC - 130:(k + 1) * PC]
    rs = proj_ratio(e, g, r["dir_sens"](g))
    out = dict(critic=float(rg.max()), td=float(rt.max()), abs_td=float(ra.max()), critic_dir=float(rs),
               critic_frac=frac_ratio(raw[FC], r["row"][FC] * B, B, rows))
    fin = bool(np.isfinite(raw).all() and np.isfinite(td).all() and np.isfinite(abs_td).all())
    return bool(fin and max(out.values()) <= 1.0), out


def check_actor(raw, r, B, rows):
    e = raw.astype(np.float64) - r["row"]
    rg = np.abs(e[:FA]) / bar_of(r)[:FA]
    g = np.zeros(PA + 4)
    g[64 * 101:PA] = r["row"][64 * 101:PA]
    rs = proj_ratio(e, g, r["dir_sens"](g))
    out = dict(actor=float(rg.max()), actor_dir=float(rs), actor_frac=frac_ratio(raw[FA], r["row"][FA] * B, B, rows))
    return bool(np.isfinite(raw).all() and max(out.values()) <= 1.0), out


def oracle(case, prm, mut=None):
    actor, critics, targets, la = prm
    kw = dict(relu_eps=BARS["relu_eps"], mut=mut)
    c = sac_critic_bucket_f64(case.host, actor, critics, targets, la, GAMMA, **kw)
    a = sac_actor_bucket_f64(case.host, actor, critics, la, tie_eps=BARS["tie_eps"], **kw)
    return c, a


def settle(case, prm, rng, rc, ra):
    """For the batches the mutations (c) run on: every sample the oracle marks ambiguous in either phase (a ReLU pre-activation of
    any net within relu_eps of zero, |Q1 - Q2| within tie_eps) is drawn again -- its transition and its rsample() draws -- on the
    host, before any launch, until none is left (Z = 0).  Such a sample's share may legitimately flow another way; at a few per cent of
    a large batch that allowance, not the rounding bars, would decide whether one sample or a 1 / B scale is seen, and (c) requires
    the rounding bars to.  The smaller cases keep their ambiguous samples and their Z (exact ties go to critic 1 in kernel and oracle
    alike)."""
    for _ in range(16):
        amb = rc["amb_rows"] | ra["amb_rows"]
        if not amb.any():
            break
        case.redraw(amb, rng)
        rc, ra = oracle(case, prm)
    assert not (rc["amb_rows"] | ra["amb_rows"]).any() and not rc["Z"].any() and not ra["Z"].any()
    return rc, ra


def with_row(r, row):
    q = dict(r)
    q["row"] = row
    return q


def mutations(case, prm, rc, ra, got, stress):
    """(c) -> {name: (critic ratio, actor ratio)}; asserts that (a) rejects each."""
    B, host = case.B, case.host
    actor, critics, targets, la = prm
    raw_c, td, abs_td, rows_c, raw_a, rows_a = got
    vi = np.flatnonzero(host["valid"] != 0)
    wt = np.abs(rc["q"][0] - rc["y"]).sum(1)[vi] * (1.0 if host["is_weights"] is None else host["is_weights"][vi])
    i = int(vi[np.argsort(wt, kind="stable")[len(vi) // 2]])
    cc = sample_contribution(sac_critic_bucket_f64, host, i, actor, critics, targets, la, GAMMA)
    ca = sample_contribution(sac_actor_bucket_f64, host, i, actor, critics, la)
    cc[FC], ca[FA] = 0.0, 0.0                        # (the count is its own mutation)
    sc, sa = np.zeros_like(cc), np.zeros_like(ca)
    sc[:2 * PC], sa[:PA] = rc["row"][:2 * PC] / B, ra["row"][:PA] / B
    nc, na = np.zeros_like(cc), np.zeros_like(ca)
    nc[FC], na[FA] = 1.0 / B, 1.0 / B
    res = {}
    for name, dc, da in (("drop", -cc, -ca), ("dup", cc, ca), ("scale", sc, sa), ("count", nc, na)):
        okc, oc = check_critic(raw_c, td, abs_td, with_row(rc, rc["row"] + dc), B, rows_c)
        oka, oa = check_actor(raw_a, with_row(ra, ra["row"] + da), B, rows_a)
        res[name] = (max(oc.values()), max(oa.values()))
        assert not okc and not oka, ("(a) does not reject", name, okc, oka, oc, oa)
    if stress:
        for mut in MUTS:
            mc, ma = oracle(case, prm, mut)
            okc, oc = check_critic(raw_c, td, abs_td, mc, B, rows_c)
            oka, oa = check_actor(raw_a, ma, B, rows_a)
            res[mut] = (max(oc.values()), max(oa.values()))
            assert not okc, ("(a) does not reject in the critic phase", mut, oc)
            assert mut == "a1_is_a0" or not oka, ("(a) does not reject in the actor phase", mut, oa)
    return res


def launch_both(case, b):
    L = case.L
    raw_c, parts_c, rows_c = run_phase(L, b, case.eps[0], True)
    td = b._keep[-1].cpu().numpy().reshape(-1, 2).astype(np.float64)
    abs_td = case.abs_td.cpu().numpy().astype(np.float64)
    raw_a, parts_a, rows_a = run_phase(L, b, case.eps[1], False)
    return (raw_c, td, abs_td, rows_c, raw_a, rows_a), parts_c, parts_a


def run_case(B, stress, weighted, form, log_alpha, seed, invalid=0.0, special=None, uav=2, use_meta=False, fused_td=False,
             partitions=(1, 3, 8), tag="", settle_all=False):
    L = make_learner(seed, stress, log_alpha)
    prm = params_of(L)
    for attempt in range(32):
        # the batch's seed is chosen on the host, with the oracle alone, before any launch: the first for which the ambiguity cap
        # holds -- ReLU pre-activations within relu_eps at most 1 % of (sample, unit) pairs, |Q1 - Q2| within tie_eps at most 1 % of
        # (sample, output column) pairs
        rng = np.random.default_rng(seed + 1000 * attempt)
        case = Case(L, B, rng, form, weighted, invalid=invalid, use_meta=use_meta, uav=uav)
        rc, ra = oracle(case, prm)
        if B >= 16384 or settle_all:
            rc, ra = settle(case, prm, rng, rc, ra)
        if special == "tile":                             # every sample of tile 3 invalid
            case.ring.h["valid"][case.rs[192:256]] = 0
        elif special == "all":
            case.ring.h["valid"][:] = 0
        if special:
            case.ring.upload()
            case.rehost()
            rc, ra = oracle(case, prm)
        if rc["amb_units"] <= 0.01 * B * 256 and ra["amb_units"] <= 0.01 * B * 320 and ra["near_tie"].sum() <= 0.01 * 2 * B:
            break
    assert rc["amb_units"] <= 0.01 * B * 256 and ra["amb_units"] <= 0.01 * B * 320, (rc["amb_units"], ra["amb_units"])
    assert ra["near_tie"].sum() <= 0.01 * 2 * B, int(ra["near_tie"].sum())
    if stress:
        assert_stress(rc["head"])
        assert_stress(ra["head"])
    if fused_td:
        os.environ["UAVENV_SAC_FUSED_TD"] = "1"
    try:
        got, parts_c, parts_a = launch_both(case, case.b)
    finally:
        os.environ.pop("UAVENV_SAC_FUSED_TD", None)
    if fused_td:                                      # the fused form leaves the targets in LDS: only the rows and abs_td are seen
        got = (got[0], rc["y"], got[2]) + got[3:]
    okc, oc = check_critic(got[0], got[1], got[2], rc, B, got[3])
    oka, oa = check_actor(got[4], ra, B, got[5])
    for k, v in {**oc, **oa}.items():
        note(k + tag, v)
    print((B, stress, weighted, form, special, fused_td), {k: round(v, 4) for k, v in {**oc, **oa}.items()})
    assert okc, ("critic (a)", oc, got[0][FC], rc["row"][FC])
    assert oka, ("actor (a)", oa, got[4][FA], ra["row"][FA])
    out = dict(case=case, prm=prm, rc=rc, ra=ra, got=got, parts_c=parts_c, parts_a=parts_a)
    if fused_td:
        return out
    # (b)
    sums = {}
    for tpw in partitions:
        b = case.batch(use_meta, tpw)
        g2, pc, pa = launch_both(case, b)
        sums[tpw] = (pc.double().sum(0).cpu().numpy(), pa.double().sum(0).cpu().numpy(), g2[1], g2[2], pc.shape[0], pa.shape[0])
        assert tpw == 0 or pc.shape[0] == (B // 64 + tpw - 1) // tpw
    t0 = partitions[0]
    for tpw in partitions[1:]:
        for ph, r, fcol in ((0, rc, FC), (1, ra, FA)):
            d = np.abs(sums[tpw][ph] - sums[t0][ph])
            rb = float((d[:fcol] / (PART * r["M"][:fcol] + 1e-30)).max())
            note(("critic/b" if ph == 0 else "actor/b") + tag, rb)
            assert rb <= 1.0, ("(b)", ph, tpw, rb)
            fr = sums[t0][ph][fcol]
            assert d[fcol] == 0.0 if B & (B - 1) == 0 else d[fcol] <= 4 * U * fr, ("(b) valid fraction", ph, tpw, d[fcol])
        assert np.array_equal(sums[tpw][2], sums[t0][2]) and np.array_equal(sums[tpw][3], sums[t0][3]), ("(b) td / abs_td bits", tpw)
    if B >= 16384:
        res = mutations(case, prm, rc, ra, got, stress)
        print("   mutations (critic, actor) error / bar:", {k: (round(v[0], 2), round(v[1], 2)) for k, v in res.items()})
    return out


# B, stress, weighted, form, log_alpha, extras
LA = float(np.log(0.01))
CASES = [
    (64, False, False, "idx", LA, {}), (64, True, True, "draws", 0.0, dict(uav=4, use_meta=True)),
    (128, True, False, "idx", LA, {}), (128, False, True, "draws", LA, dict(uav=2, use_meta=True)),
    (2368, True, False, "draws", 0.0, dict(uav=4)), (2368, False, True, "idx", LA, dict(use_meta=True)),
    (16448, False, True, "draws", LA, dict(uav=2, use_meta=True)), (16448, True, False, "idx", 0.0, {}),
    (32768, False, False, "idx", LA, {}), (32768, True, True, "draws", 0.0, dict(uav=4, use_meta=True)),
    (32768, False, True, "draws", LA, dict(uav=2)), (32768, True, False, "idx", LA, dict(use_meta=True)),
    (65536, True, True, "idx", 0.0, {}),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:4]) + ("-a1" if c[4] == 0.0 else ""))
def test_raw_rows_against_f64(case):
    B, stress, weighted, form, la, extra = case
    run_case(B, stress, weighted, form, la, seed=CASES.index(case) + 1, **extra)


@pytest.mark.parametrize("B,stress,form", [(128, True, "idx"), (2368, False, "draws"), (16448, True, "idx")])
def test_fused_td_against_f64(B, stress, form):
    """(i) UAVENV_SAC_FUSED_TD=1 (read per call): k_sac_critic_grad computes the TD targets itself -- against f64, not against the
    split form."""
    run_case(B, stress, True, form, 0.0 if stress else LA, seed=50 + B % 7, fused_td=True, tag="/fused_td")


def adam_header(L, lr, tau, t):
    return _lib().UavSacAdam(lr, L.beta1, L.beta2, L.adam_eps, 1.0 - L.beta1 ** t, float(np.sqrt(1.0 - L.beta2 ** t)), tau, 0.0, None,
                             None, 0, 0)


def seed_moments(L, rc, ra, rng, offset_targets=True):
    fc, fa = max(rc["row"][FC], 1e-9), max(ra["row"][FA], 1e-9)
    gc = (np.abs(rc["row"][:2 * PC]) + BARS["tau"] * rc["M"][:2 * PC] + 1e-12) / fc
    ga = (np.abs(ra["row"][:PA]) + BARS["tau"] * ra["M"][:PA] + 1e-12) / fa
    with torch.no_grad():
        for k in range(2):
            g = gc[k * PC:(k + 1) * PC]
            L._cblocks[4 + 2 * k, :PC].copy_(torch.tensor((g * rng.choice([-1.0, 1.0], PC) * rng.uniform(0.5, 1.5, PC)).astype(np.float32)))
            L._cblocks[5 + 2 * k, :PC].copy_(torch.tensor((g * g * rng.uniform(0.5, 2.0, PC)).astype(np.float32)))
        L._blocks[1, :PA].copy_(torch.tensor((ga * rng.choice([-1.0, 1.0], PA) * rng.uniform(0.5, 1.5, PA)).astype(np.float32)))
        L._blocks[2, :PA].copy_(torch.tensor((ga * ga * rng.uniform(0.5, 2.0, PA)).astype(np.float32)))
        L._alpha_mv.copy_(torch.tensor([0.3, 0.2]))
        if offset_targets:
            L._cblocks[2:4].add_(1.0)


@pytest.mark.parametrize("special,invalid", [(None, 0.25), ("tile", 0.0), ("all", 0.0)])
def test_reduce_adam_against_f64(special, invalid):
    """(d) and (e).  The batches are settled (no ambiguous sample, Z = 0: see settle) so that the f64 bucket pins the mean gradient to
    the rounding bars and a valid fraction off by ONE sample of 2 368 shows."""
    from test_dqn_grad_kernels_gpu import check_adam
    B, t, tau = 2368, 5, float(np.float32(0.05))
    out = run_case(B, special != "tile", True, "idx", 0.0 if special != "tile" else LA, seed=70 + len(special or ""), invalid=invalid,
                   special=special, tag="/adam_case", settle_all=True)
    case, L, rc, ra, got = out["case"], out["case"].L, out["rc"], out["ra"], out["got"]
    if special == "all":
        assert got[0][FC] == 0.0 and got[4][FA] == 0.0 and not got[0][:2 * PC].any() and not got[4][:PA].any()
    if special == "tile":
        assert not case.host["valid"][192:256].any() and case.host["valid"].sum() > B // 2
    if special is None:
        # (e): every valid = 0 row of frame 0 rewritten (observations, actions, reward, done): bit-identical partial rows
        ring = case.ring
        inv = np.flatnonzero(ring.h["valid"][:ring.n] == 0)
        assert len(inv) > 0.1 * ring.n and (case.host["valid"] == 0).sum() > 0.1 * B
        rng = np.random.default_rng(9)
        ring.set_obs(inv, rng.integers(0, len(pool().rows), len(inv)))
        ring.h["act0"][inv] = -ring.h["act0"][inv]
        ring.h["act1"][inv] = 0.5 * ring.h["act1"][inv] + 0.1
        ring.h["reward"][inv] = -ring.h["reward"][inv] + 17.0
        ring.h["done"][inv] = 1 - ring.h["done"][inv]
        ring.upload()
        _, pc2, pa2 = launch_both(case, case.b)
        assert torch.equal(pc2, out["parts_c"]) and torch.equal(pa2, out["parts_a"]), "(e) invalid rows changed the partial rows"
    # (d)
    rng = np.random.default_rng(5)
    seed_moments(L, rc, ra, rng)
    cb0 = L._cblocks.cpu().numpy().astype(np.float64)
    ab0 = L._blocks.cpu().numpy().astype(np.float64)
    la0, amv0 = float(L.log_alpha), L._alpha_mv.cpu().numpy().astype(np.float64)
    pc, pa = out["parts_c"], out["parts_a"]
    sc = torch.zeros(8, device="cuda")
    hc, ha = adam_header(L, L.critic_lr, tau, t), adam_header(L, L.actor_lr, 0.0, t)
    cb = L._cblocks
    assert L.lib.uavenv_sac_critic_adam(C.byref(L._nets), pc.data_ptr(), pc.shape[0], cb[4].data_ptr(), cb[5].data_ptr(), cb[6].data_ptr(),
                                        cb[7].data_ptr(), C.byref(hc), sc.data_ptr(), L._stream()) == 0
    assert L.lib.uavenv_sac_actor_adam(C.byref(L._nets), pa.data_ptr(), pa.shape[0], B, L._blocks[1].data_ptr(), L._blocks[2].data_ptr(),
                                       L._alpha_mv.data_ptr(), C.byref(ha), L.alpha_lr, L.target_entropy, sc[4:].data_ptr(),
                                       L._stream()) == 0
    torch.cuda.synchronize()
    cb1, ab1 = L._cblocks.cpu().numpy().astype(np.float64), L._blocks.cpu().numpy().astype(np.float64)
    assert np.isfinite(cb1).all() and np.isfinite(ab1).all() and np.isfinite(float(L.log_alpha)) and torch.isfinite(L._alpha_mv).all()
    lr_c, lr_a, lr_al = (float(np.float32(x)) for x in (L.critic_lr, L.actor_lr, L.alpha_lr))
    betas, eps = (L.beta1, L.beta2), L.adam_eps
    fc, fa = rc["row"][FC], ra["row"][FA]
    bc, ba = bar_of(rc), bar_of(ra)
    oc = sac_adam_f64("critic", rc["row"], dict(w1=cb0[0], w2=cb0[1], t1=cb0[2], t2=cb0[3], m1=cb0[4], v1=cb0[5], m2=cb0[6], v2=cb0[7]),
                      t, lr_c, tau=tau)
    oa = sac_adam_f64("actor", ra["row"], dict(w=ab0[0], m=ab0[1], v=ab0[2], log_alpha=la0, alpha_mv=amv0), t, lr_a, alpha_lr=lr_al,
                      target_entropy=L.target_entropy, batch=B)
    norm_c, norm_a = (1.0 / fc if fc > 0 else 0.0), (1.0 / fa if fa > 0 else 0.0)
    worst = 0.0
    for k in range(2):
        f = np.stack([cb1[k, :PC], np.zeros(PC), cb1[4 + 2 * k, :PC], cb1[5 + 2 * k, :PC]])
        g = oc[f"g{k + 1}"]
        gerr = bc[k * PC:(k + 1) * PC] * norm_c + 2.0 ** -22 * np.abs(g)
        ok, w = check_adam(f, cb0[k, :PC], cb0[4 + 2 * k, :PC], cb0[5 + 2 * k, :PC], g, gerr, t, lr_c, betas, eps, False)
        worst = max(worst, w)
        assert ok, ("critic adam", k, w)
        # the soft update: t' = t (1 - tau) + w' tau on the kernel's own w'
        tgt = cb0[2 + k, :PC] * (1.0 - tau) + cb1[k, :PC] * tau
        assert np.all(np.abs(cb1[2 + k, :PC] - tgt) <= 2.0 ** -22 * (np.abs(cb0[2 + k, :PC]) + np.abs(cb1[k, :PC])) + 1e-30), ("soft update", k)
        assert np.abs(cb1[2 + k, :PC] - cb0[2 + k, :PC]).max() > 0.01                        # (visible: the targets were offset by 1)
        if fc > 0:
            for dn in (-1.0, 1.0):
                g2 = rc["row"][k * PC:(k + 1) * PC] / (fc + dn / B)
                assert not check_adam(f, cb0[k, :PC], cb0[4 + 2 * k, :PC], cb0[5 + 2 * k, :PC], g2, gerr, t, lr_c, betas, eps, False)[0], dn
    f = np.stack([ab1[0, :PA], np.zeros(PA), ab1[1, :PA], ab1[2, :PA]])
    gerr = ba[:PA] * norm_a + 2.0 ** -22 * np.abs(oa["g"])
    ok, w = check_adam(f, ab0[0, :PA], ab0[1, :PA], ab0[2, :PA], oa["g"], gerr, t, lr_a, betas, eps, False)
    worst = max(worst, w)
    assert ok, ("actor adam", w)
    if fa > 0:
        for dn in (-1.0, 1.0):
            assert not check_adam(f, ab0[0, :PA], ab0[1, :PA], ab0[2, :PA], ra["row"][:PA] / (fa + dn / B), gerr, t, lr_a, betas, eps, False)[0], dn
    # log_alpha: Adam on one component
    la1, amv1 = float(L.log_alpha), L._alpha_mv.cpu().numpy().astype(np.float64)
    gl = oa["g_alpha"]
    glerr = np.exp(la0) * ba[PA + 1] * (0.5 / B) * norm_a + 2.0 ** -21 * (abs(gl) + np.exp(la0) * L.target_entropy)
    f1 = np.array([[la1], [0.0], [amv1[0]], [amv1[1]]])
    ok, w = check_adam(f1, np.array([la0]), amv0[:1], amv0[1:], np.array([gl]), np.array([glerr]), t, lr_al, betas, eps, False)
    worst = max(worst, w)
    assert ok, ("log_alpha adam", w, la1, oa["log_alpha"])
    # the losses the launch reports: the row's loss columns over the valid fraction
    s = sc.cpu().numpy().astype(np.float64)
    for k in range(2):
        assert abs(s[k] - oc["losses"][k]) <= bc[2 * PC + k] * norm_c + 2.0 ** -21 * abs(oc["losses"][k]) + 1e-30
    assert abs(s[4] - oa["loss"]) <= ba[PA] * norm_a + 2.0 ** -21 * abs(oa["loss"]) + 1e-30
    if special == "all":                          # the moments only decay (check_adam on a zero gradient); the weights move by momentum
        assert np.abs(cb1[0, :PC] - cb0[0, :PC]).max() > 0 and np.abs(ab1[0, :PA] - ab0[0, :PA]).max() > 0
    note("adam", worst)
    print("reduce_adam", special, "worst error / bar", round(worst, 4))


def test_records_equal_planes():
    """(f) on the pool's real ring (records written by the step launches, attach_action1), draws form, s' wrapping."""
    p = pool()
    rng = np.random.default_rng(21)
    L = make_learner(21, True, 0.0)
    case = Case(L, 2368, rng, "draws", True, ring=p.ring, uav=2)
    f = case.draws[:, 0].cpu().numpy()
    assert (f == p.ring.frames - 1).any()                                    # some s' wrap to frame 0
    assert (case.host["valid"] == 0).any() or True
    res = []
    for use_meta in (False, True):
        b = case.batch(use_meta, 3)
        _, pc, pa = launch_both(case, b)
        res.append((pc, pa, b._keep[-1].clone(), case.abs_td.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][1]).all()
    # and the real ring's batch against f64 too (the records' planes, valid = 0 rows of waiting agents included)
    prm = params_of(L)
    rc, ra = oracle(case, prm)
    got, _, _ = launch_both(case, case.batch(True, 3))
    okc, oc = check_critic(got[0], got[1], got[2], rc, case.B, got[3])
    oka, oa = check_actor(got[4], ra, case.B, got[5])
    for k, v in {**oc, **oa}.items():
        note(k + "/real_ring", v)
    assert okc and oka, (oc, oa)


def test_several_trainers_per_launch():
    """(g)"""
    Lb = _lib()
    spec = [(64, 1), (2368, 3), (4096, 8), (128, 2)]
    rng = np.random.default_rng(31)
    cases = [Case(make_learner(40 + j, j % 2 == 1, 0.0 if j % 2 else LA), B, rng, "idx" if j % 2 else "draws", j < 2, uav=4,
                  use_meta=j >= 2) for j, (B, _) in enumerate(spec)]
    n = len(spec)
    lib = cases[0].L.lib
    stream = cases[0].L._stream()
    grids = [lib.uavenv_sac_partial_rows_n(B, n, tpw) for B, tpw in spec]
    assert grids == [1, 13, 8, 1]
    single = []
    for cs, (B, tpw) in zip(cases, spec):
        b = cs.batch(cs.use_meta, tpw)
        _, pc, pa = launch_both(cs, b)
        single.append((pc, pa, b._keep[-1].clone(), cs.abs_td.clone()))
        cs.abs_td.fill_(-1.0)
    SENT = 12345.0
    for critic in (True, False):
        nets = (Lb.UavSacNets * n)()
        bs = (Lb.UavSacBatch * n)()
        parts = (C.c_void_p * n)()
        bufs, keep = [], []
        for j, (cs, (B, tpw)) in enumerate(zip(cases, spec)):
            b = cs.batch(cs.use_meta, tpw)
            b.eps = cs.eps[0 if critic else 1].data_ptr()
            keep.append(b)
            nets[j], bs[j] = cs.L._nets, b
            buf = torch.full((B // 64, Lb.SAC_CRITIC_STRIDE if critic else Lb.SAC_ACTOR_STRIDE), SENT, device="cuda")
            bufs.append(buf)
            parts[j] = buf.data_ptr()
        if critic:
            rc_ = lib.uavenv_sac_critic_grad_multi(C.addressof(nets), C.addressof(bs), n, GAMMA, 1.0, C.addressof(parts), stream)
        else:
            rc_ = lib.uavenv_sac_actor_grad_multi(C.addressof(nets), C.addressof(bs), n, 1.0, C.addressof(parts), stream)
        assert rc_ == 0, lib.uavenv_sac_last_error()
        torch.cuda.synchronize()
        for j, cs in enumerate(cases):
            want = single[j][0 if critic else 1]
            g = grids[j]
            assert want.shape[0] == g
            assert torch.equal(bufs[j][:g], want), ("slot", j, "critic" if critic else "actor")
            assert bool((bufs[j][g:] == SENT).all()), ("rows beyond the slot's grid written", j)
            if critic:
                assert torch.equal(keep[j]._keep[-1], single[j][2]) and torch.equal(cs.abs_td, single[j][3]), ("td / abs_td", j)
        if critic:
            cbufs = bufs
        else:
            abufs = bufs
    # *_adam_multi: every slot's rows reduced to ONE row (the entry points share `rows`), then the multi launch against single calls
    t, tau, B0 = 5, float(np.float32(0.05)), 128
    raws_c, raws_a = [], []
    for j, cs in enumerate(cases):
        L = cs.L
        seed_moments(L, dict(row=np.ones(2 * PC + 4), M=np.ones(2 * PC + 4)), dict(row=np.ones(PA + 4), M=np.ones(PA + 4)),
                     np.random.default_rng(j))
        rcw = torch.empty(Lb.SAC_CRITIC_STRIDE, device="cuda")
        raw = torch.empty(Lb.SAC_ACTOR_STRIDE, device="cuda")
        assert lib.uavenv_sac_reduce(cbufs[j].data_ptr(), grids[j], Lb.SAC_CRITIC_STRIDE, rcw.data_ptr(), stream) == 0
        assert lib.uavenv_sac_reduce(abufs[j].data_ptr(), grids[j], Lb.SAC_ACTOR_STRIDE, raw.data_ptr(), stream) == 0
        raws_c.append(rcw)
        raws_a.append(raw)
    torch.cuda.synchronize()
    state0 = [(cs.L._blocks.clone(), cs.L._cblocks.clone(), cs.L.log_alpha.clone(), cs.L._alpha_mv.clone()) for cs in cases]

    def restore():
        for cs, st in zip(cases, state0):
            cs.L._blocks.copy_(st[0]); cs.L._cblocks.copy_(st[1]); cs.L.log_alpha.copy_(st[2]); cs.L._alpha_mv.copy_(st[3])   # noqa: E702

    def snapshot(scal):
        torch.cuda.synchronize()
        return [(cs.L._blocks.clone(), cs.L._cblocks.clone(), cs.L.log_alpha.clone(), cs.L._alpha_mv.clone(), s.clone())
                for cs, s in zip(cases, scal)]
    arr = lambda xs: (C.c_void_p * n)(*[x.data_ptr() for x in xs])      # noqa: E731
    hs_c = (Lb.UavSacAdam * n)(*[adam_header(cs.L, cs.L.critic_lr, tau, t) for cs in cases])
    hs_a = (Lb.UavSacAdam * n)(*[adam_header(cs.L, cs.L.actor_lr, 0.0, t) for cs in cases])
    nets = (Lb.UavSacNets * n)(*[cs.L._nets for cs in cases])
    scal = [torch.zeros(8, device="cuda") for _ in cases]
    L0 = cases[0].L
    ptrs = [arr(raws_c), arr([cs.L._cblocks[4] for cs in cases]), arr([cs.L._cblocks[5] for cs in cases]),
            arr([cs.L._cblocks[6] for cs in cases]), arr([cs.L._cblocks[7] for cs in cases]), arr(scal),
            arr(raws_a), arr([cs.L._blocks[1] for cs in cases]), arr([cs.L._blocks[2] for cs in cases]),
            arr([cs.L._alpha_mv for cs in cases]), arr([s[4:] for s in scal])]             # (kept alive across the calls)
    ad = [C.addressof(x) for x in ptrs]
    assert lib.uavenv_sac_critic_adam_multi(C.addressof(nets), ad[0], 1, ad[1], ad[2], ad[3], ad[4], C.addressof(hs_c), ad[5], n, stream) == 0
    assert lib.uavenv_sac_actor_adam_multi(C.addressof(nets), ad[6], 1, B0, ad[7], ad[8], ad[9], C.addressof(hs_a), L0.alpha_lr,
                                           L0.target_entropy, ad[10], n, stream) == 0
    multi = snapshot(scal)
    restore()
    for s in scal:
        s.zero_()
    for j, cs in enumerate(cases):
        L = cs.L
        cb = L._cblocks
        assert lib.uavenv_sac_critic_adam(C.byref(L._nets), raws_c[j].data_ptr(), 1, cb[4].data_ptr(), cb[5].data_ptr(), cb[6].data_ptr(),
                                          cb[7].data_ptr(), C.byref(hs_c[j]), scal[j].data_ptr(), stream) == 0
        assert lib.uavenv_sac_actor_adam(C.byref(L._nets), raws_a[j].data_ptr(), 1, B0, L._blocks[1].data_ptr(), L._blocks[2].data_ptr(),
                                         L._alpha_mv.data_ptr(), C.byref(hs_a[j]), L.alpha_lr, L.target_entropy, scal[j][4:].data_ptr(),
                                         stream) == 0
    one = snapshot(scal)
    for j in range(n):
        for x, y in zip(multi[j], one[j]):
            assert torch.equal(x, y), ("adam_multi differs from the single call", j)
        assert not torch.equal(multi[j][1], state0[j][1]) and torch.isfinite(multi[j][0]).all() and torch.isfinite(multi[j][1]).all()


def test_act_on_the_stress_actor():
    """(h) k_sac_act, ragged count and strided rows.  Bar: the head pre-activations within tau_td of their |.|-forward, carried to
    the action to first order, plus 8 u for the four tanhf / expf / log1pf calls and the product sd eps on values of size <= 1 + |eps|."""
    p = pool()
    L = make_learner(61, True, 0.0)
    prm = params_of(L)
    n_rows = p.packed.shape[0]
    N = p.env.N
    worst = 0.0
    for slot, count in ((0, N // 2), (1, 333)):
        a0 = torch.full((n_rows,), 7.0, device="cuda")
        a1 = torch.full((n_rows,), 7.0, device="cuda")
        eps = torch.randn((count, 2), device="cuda")
        first = 2 * N + slot
        L.act_rows(p.packed, first, 2, count, a0, a1, eps)
        torch.cuda.synchronize()
        rows = first + 2 * np.arange(count)
        hd = actor_forward(p.rows[rows], prm[0], eps.cpu().numpy())
        if count > 1000:
            assert_stress(hd)
        got = np.stack([a0.cpu().numpy()[rows], a1.cpu().numpy()[rows]], 1).astype(np.float64)
        bar = act_bar(hd, BARS["tau_td"], U)
        assert np.isfinite(got).all()
        worst = max(worst, float((np.abs(got - hd["act"]) / bar).max()))
        un = np.ones(n_rows, dtype=bool)
        un[rows] = False
        assert bool((a0.cpu().numpy()[un] == 7.0).all()) and bool((a1.cpu().numpy()[un] == 7.0).all())
    note("act", worst)
    print("k_sac_act worst error / bar", round(worst, 4))
    assert worst <= 1.0, worst


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
torch.cuda.set_device(0)
import test_sac_grad_kernels_gpu as T
T.run_case(2368, True, True, "idx", 0.0, seed=91, partitions=(0, 1), tag="/wgs")
T.run_case(16448, False, False, "draws", T.LA, seed=92, uav=4, partitions=(0, 1), tag="/wgs")
print("knob worst ratios", T.WORST)
"""


@pytest.mark.parametrize("wgs", ["16", "64"])
def test_wgs_knob_against_f64(wgs):
    """(i) UAVENV_SAC_WGS (read once per process: a fresh child under its own time limit): the default partition becomes several
    tiles per workgroup at these sizes (16: 3 and 8; 64: 1 and 5) -- against f64 and against the one-tile partition."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("UAVENV_")}
    env["UAVENV_SAC_WGS"] = wgs
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, ROOT], env=env, check=True, timeout=330)
