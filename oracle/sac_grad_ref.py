"""Float64 statement of one fused SAC update (continuous actions) on the reference's nets -- what csrc/sac.hip's k_sac_td,
k_sac_critic_grad, k_sac_actor_grad, k_sac_act and k_sac_reduce_adam compute, written from the mathematics so that the kernels can
be held against it at the raw partial-row bucket.  CPU only (numpy); test infrastructure, not product code.

Nets (nets.py; the flat layouts of FusedSACLearner._bind):
  actor  100-64-(2+2): fc1.w 64x100 | fc1.b 64 | fc_mu.w 2x64 | fc_std.w 2x64 | fc_mu.b 2 | fc_std.b 2            (6 724)
  critic 102-64-64-2 : fc1.w 64x102 | fc1.b 64 | fc2.w 64x64 | fc2.b 64 | fc_out.w 2x64 | fc_out.b 2            (10 882)
Head (BaseCNN.py:470-483, quirks kept): mu = tanh(m), sd = tanh(softplus(s)) (threshold 20), ns = mu + sd eps, act = tanh(ns),
  log pi = -(ns - mu)^2 / (2 sd^2) - log sd - log sqrt(2 pi) - log(1 - tanh(act)^2 + 1e-7)            per action dimension, [B, 2]
The quadratic term is eps^2 / 2 exactly, whatever the parameters: it carries no gradient (autograd and f32 arithmetic both form it
from ns - mu and cancel terms of size |ns| |eps| / sd; the error scale lp_abs below carries that amplification).
Out of scope: fc_std pre-activations below -12, where sd^2 heads for f32 underflow and the reference's formula is undefined too.

Every critic output column d pairs with action dimension d in the TD target (the reference's [B, 2] broadcasting):
  y[:, d] = r + gamma (min(Qt1, Qt2)(s', a')[:, d] - alpha log pi(a' | s')[:, d]) (1 - done)

`mut` (tests only) evaluates the statement with one switch flipped, to show that an input reaches a branch with enough weight:
  "a1_is_a0"   the target critics see (a0, a0) instead of (a0, a1)          "max_q"  the maximum of the two critics, not the minimum
  "no_log_sd"  log pi without its - log sd term                             "one_tanh"  1 - tanh(ns)^2 (one tanh) in the correction
"""
from __future__ import annotations

import numpy as np

from oracle.dqn_grad_ref import adam_step_f64

W, HID, NA = 100, 64, 2
PA = HID * W + HID + 4 * HID + 4            # 6 724
PC = HID * (W + NA) + HID + HID * HID + HID + NA * HID + NA   # 10 882
LOG_SQRT_2PI = 0.9189385332046727
TD_FLOOR = 2.0 ** -20
TILE = 64
FLAG_COLS = np.r_[11:86, 90:95]             # the 0 / 1 columns of a packed observation row (include/uavenv.h)
MUTS = ("a1_is_a0", "max_q", "no_log_sd", "one_tanh")


def unflatten_actor(flat):
    f = np.asarray(flat, dtype=np.float64).reshape(-1)[:PA]
    o = HID * W
    return (f[:o].reshape(HID, W), f[o:o + HID], f[o + HID:o + HID + 4 * HID].reshape(4, HID), f[o + HID + 4 * HID:PA])


def unflatten_critic(flat):
    f = np.asarray(flat, dtype=np.float64).reshape(-1)[:PC]
    a = HID * (W + NA)
    b = a + HID
    c = b + HID * HID
    d = c + HID
    e = d + NA * HID
    return (f[:a].reshape(HID, W + NA), f[a:b], f[b:c].reshape(HID, HID), f[c:d], f[d:e].reshape(NA, HID), f[e:PC])


def actor_head_f64(m, s, eps, mut=None) -> dict:
    """The head after fc_mu / fc_std, [B, 2] each.  Returns mu, sd, sig (d softplus), ns, act, th, u, lp, dlp_dact."""
    m, s, eps = (np.asarray(x, dtype=np.float64) for x in (m, s, eps))
    mu = np.tanh(m)
    with np.errstate(over="ignore"):
        sp = np.where(s > 20.0, s, np.log1p(np.exp(np.minimum(s, 50.0))))
        sig = np.where(s > 20.0, 1.0, 1.0 / (1.0 + np.exp(-s)))
    sd = np.tanh(sp)
    ns = mu + sd * eps
    act = np.tanh(ns)
    if mut == "one_tanh":
        th, dth = act, np.ones_like(act)
    else:
        th, dth = np.tanh(act), 1.0 - np.tanh(act) ** 2
    u = 1.0 - th * th + 1e-7
    log_sd = np.zeros_like(sd) if mut == "no_log_sd" else np.log(sd)
    lp = -0.5 * eps * eps - log_sd - LOG_SQRT_2PI - np.log(u)
    return dict(mu=mu, sd=sd, sig=sig, ns=ns, act=act, th=th, u=u, lp=lp, dlp_dact=2.0 * th * dth / u, log_sd=log_sd)


def _actor_fwd(X, actor, eps, mut=None):
    W1, b1, Wh, bh = unflatten_actor(actor)
    pre = X @ W1.T + b1
    H = np.maximum(pre, 0.0)
    o = H @ Wh.T + bh
    habs = np.abs(X) @ np.abs(W1).T + np.abs(b1)
    oabs = habs @ np.abs(Wh).T + np.abs(bh)
    hd = actor_head_f64(o[:, :2], o[:, 2:], eps, mut)
    hd.update(pre=pre, H=H, o=o, habs=habs, m_abs=oabs[:, :2], s_abs=oabs[:, 2:], eps=np.asarray(eps, dtype=np.float64))
    # |d log pi / d m|, |d log pi / d s|: how an error in the head's pre-activations reaches log pi
    dns_dm = 1.0 - hd["mu"] ** 2
    dsd_ds = (1.0 - hd["sd"] ** 2) * hd["sig"]
    dlp_dns = hd["dlp_dact"] * (1.0 - hd["act"] ** 2)
    g_sd = 0.0 if mut == "no_log_sd" else 1.0 / hd["sd"]
    # the scale of log pi's error, in units of the pre-activations' relative error (tau_td ~ 2^-16, some 200 roundings): the
    # pre-activations' own share at full weight; the direct terms -- four transcendental calls of a few ulp each, 16 u = 2^-4 of
    # that unit; ns - mu, where ONE rounding of ns (u |ns|, twice for a product that is not fused) is amplified by |eps| / sd: 2^-7
    hd["lp_abs"] = (2.0 ** -4 * (0.5 * hd["eps"] ** 2 + np.abs(hd["log_sd"]) + LOG_SQRT_2PI + np.abs(np.log(hd["u"]))) +
                    2.0 ** -7 * np.abs(hd["ns"]) * np.abs(hd["eps"]) / hd["sd"] + np.abs(dlp_dns) * dns_dm * hd["m_abs"] +
                    (np.abs(dlp_dns * hd["eps"]) + g_sd) * dsd_ds * hd["s_abs"])
    return hd


def _critic_fwd(X, A, critic):
    W1, b1, W2, b2, Wo, bo = unflatten_critic(critic)
    XA = np.concatenate([X, A], axis=1)
    pre1 = XA @ W1.T + b1
    H1 = np.maximum(pre1, 0.0)
    pre2 = H1 @ W2.T + b2
    H2 = np.maximum(pre2, 0.0)
    q = H2 @ Wo.T + bo
    h1abs = np.abs(XA) @ np.abs(W1).T + np.abs(b1)
    h2abs = h1abs @ np.abs(W2).T + np.abs(b2)
    qabs = h2abs @ np.abs(Wo).T + np.abs(bo)
    return dict(XA=XA, pre1=pre1, H1=H1, pre2=pre2, H2=H2, q=q, h1abs=h1abs, h2abs=h2abs, q_abs=qabs, net=(W1, b1, W2, b2, Wo, bo))


def _masks(F, relu_eps):
    """(widened mask, ambiguous) of both hidden layers: a unit within relu_eps of its |.|-forward of zero may go either way."""
    out = []
    for pre, habs in ((F["pre1"], F["h1abs"]), (F["pre2"], F["h2abs"])):
        amb = (np.abs(pre) <= relu_eps * habs) if relu_eps > 0.0 else np.zeros(pre.shape, dtype=bool)
        out.append((((pre > 0.0) | amb).astype(np.float64), amb))
    return out


def _critic_bwd(F, dout):
    W1, b1, W2, b2, Wo, bo = F["net"]
    dH2 = (dout @ Wo) * (F["pre2"] > 0.0)
    dH1 = (dH2 @ W2) * (F["pre1"] > 0.0)
    return dH1, dH2


def _critic_flat(F, dout, dH1, dH2, A_=None, B_=None, sq=False):
    """The flat gradient from dout / dH2 / dH1 and the forward's H2 / H1 / XA (or, with sq, the sums of squares)."""
    XA, H1, H2 = (F["XA"] if A_ is None else A_), F["H1"], F["H2"]
    if sq:
        XA, H1, H2, dout, dH1, dH2 = XA ** 2, H1 ** 2, H2 ** 2, dout ** 2, dH1 ** 2, dH2 ** 2
    return np.concatenate([(dH1.T @ XA).ravel(), dH1.sum(0), (dH2.T @ H1).ravel(), dH2.sum(0), (dout.T @ H2).ravel(), dout.sum(0)])


def _critic_abs_bwd(F, ao, m2, m1):
    W1, b1, W2, b2, Wo, bo = F["net"]
    adh2 = (ao @ np.abs(Wo)) * m2
    adh1 = (adh2 @ np.abs(W2)) * m1
    return adh1, adh2


def _tile_scale(dH1, X, n_in):
    """The split dW1's scale: per 64-sample tile, the tile's largest |dH1| times how many of its samples have the flag column set
    (every hidden unit alike) -- the kernel's flag-column sums are accurate to 2^-22 of this.  [64 * n_in] (zero off the flags)."""
    B = dH1.shape[0]
    nt = (B + TILE - 1) // TILE
    pad = nt * TILE - B
    a = np.abs(dH1).max(axis=1)
    f = X[:, FLAG_COLS]
    if pad:
        a = np.concatenate([a, np.zeros(pad)])
        f = np.concatenate([f, np.zeros((pad, f.shape[1]))])
    amax = a.reshape(nt, TILE).max(axis=1)
    cnt = f.reshape(nt, TILE, -1).sum(axis=1)
    col = np.zeros(n_in)
    col[FLAG_COLS] = amax @ cnt
    return np.tile(col, HID)


def sac_td_f64(s2, rewards, dones, eps_next, actor, target1, target2, log_alpha, gamma, bound=1.0, mut=None) -> dict:
    """y [B, 2] and y_abs [B, 2] (the sum of the magnitudes of the terms behind y: the scale of its rounding error)."""
    X2 = np.asarray(s2, dtype=np.float64)
    r = np.asarray(rewards, dtype=np.float64).reshape(-1, 1)
    nd = 1.0 - np.asarray(dones, dtype=np.float64).reshape(-1, 1)
    alpha = float(np.exp(np.float64(log_alpha)))
    hd = _actor_fwd(X2, actor, eps_next, mut)
    a = hd["act"] * bound
    if mut == "a1_is_a0":
        a = np.stack([a[:, 0], a[:, 0]], axis=1)
    F1, F2 = _critic_fwd(X2, a, target1), _critic_fwd(X2, a, target2)
    pick = np.maximum if mut == "max_q" else np.minimum
    y = r + gamma * (pick(F1["q"], F2["q"]) - alpha * hd["lp"]) * nd
    y_abs = np.abs(r) + gamma * nd * (np.maximum(F1["q_abs"], F2["q_abs"]) + alpha * hd["lp_abs"])
    return dict(y=y, y_abs=y_abs, head=hd)


def sac_critic_bucket_f64(batch: dict, actor, critics, targets, log_alpha, gamma, bound=1.0, *, denom=None, relu_eps=0.0,
                          td_floor=TD_FLOOR, mut=None) -> dict:
    """The raw row k_sac_critic_grad writes, summed over the workgroups, as the kernel defines it.
    batch: s, s2 [B, 100], actions [B, 2], rewards, dones, valid [B], eps_next [B, 2], is_weights [B] or None.
    Per critic k the gradient of sum_s w_s |q_k(s, a) - y|^2 / (2 B), w = valid x is_weight, B = denom (default: the rows given).
    Returns row [2 PC + 4] = grad 1 | grad 2 | loss 1, loss 2, valid fraction, 0; abs_td [B]; y, y_abs, q_abs [2][B, 2]; and, in the
    row's layout, M (sum of |contributions|, |q - y| widened by td_floor (|q| + |y|)), N2 (sum of squares of what a forward error
    of its scale q_abs + y_abs in q - y moves the component by), Z (what ReLU units of either hidden layer within relu_eps of
    zero may move), T (the split dW1's per-tile scale, flag columns of fc1 only); dir_sens(u); amb_units, amb_rows [B]."""
    X = np.asarray(batch["s"], dtype=np.float64)
    B = X.shape[0]
    D = float(B if denom is None else denom)
    A = np.asarray(batch["actions"], dtype=np.float64).reshape(B, 2)
    val = np.asarray(batch["valid"], dtype=np.float64).reshape(-1)
    isw = np.ones(B) if batch.get("is_weights") is None else np.asarray(batch["is_weights"], dtype=np.float64).reshape(-1)
    w = (val * isw)[:, None]
    td = sac_td_f64(batch["s2"], batch["rewards"], batch["dones"], batch["eps_next"], actor, targets[0], targets[1], log_alpha,
                    gamma, bound, mut)
    y, y_abs = td["y"], td["y_abs"]
    row, M, N2, Z, T = (np.zeros(2 * PC + 4) for _ in range(5))
    qs, qabs, parts = [], [], []
    amb_units = 0
    amb_rows = np.zeros(B, dtype=bool)
    for k, c in enumerate(critics):
        F = _critic_fwd(X, A, c)
        (m1, a1), (m2, a2) = _masks(F, relu_eps)
        e = F["q"] - y
        dout = w * e / D
        dH1, dH2 = _critic_bwd(F, dout)
        sl = slice(k * PC, (k + 1) * PC)
        row[sl] = _critic_flat(F, dout, dH1, dH2)
        row[2 * PC + k] = float(np.sum(w * e * e)) * 0.5 / D
        wide = np.abs(e) + td_floor * (np.abs(F["q"]) + np.abs(y))
        ao = np.abs(w) * wide / D
        adh1, adh2 = _critic_abs_bwd(F, ao, m2, m1)
        M[sl] = _critic_flat(F, ao, adh1, adh2, A_=np.abs(F["XA"]))
        M[2 * PC + k] = float(np.sum(np.abs(w) * wide * wide)) * 0.5 / D
        sens = np.abs(w) * (F["q_abs"] + y_abs) / D
        sdh1, sdh2 = _critic_abs_bwd(F, sens, m2, m1)
        N2[sl] = _critic_flat(F, sens, sdh1, sdh2, sq=True)
        N2[2 * PC + k] = float(np.sum((np.abs(w) * wide * (F["q_abs"] + y_abs) / D) ** 2))
        if a1.any() or a2.any():
            full = np.abs(dout)
            z1, _ = _critic_abs_bwd(F, full, m2, a1.astype(np.float64))            # a layer-1 unit flips: its whole dH1 terms
            zz1, zz2 = _critic_abs_bwd(F, full, a2.astype(np.float64), m1)         # a layer-2 unit flips: dH2 and all below it
            zero = np.zeros_like(dout)
            Z[sl] = _critic_flat(F, zero, z1 + zz1, zz2, A_=np.abs(F["XA"]))
        T[sl][:HID * (W + NA)] = _tile_scale(dH1, F["XA"], W + NA)
        amb_units += int(a1.sum() + a2.sum())
        amb_rows |= a1.any(1) | a2.any(1)
        qs.append(F["q"])
        qabs.append(F["q_abs"])
        parts.append((F, sens, sdh1, sdh2))
    row[2 * PC + 2] = float(val.sum()) / D
    pick = np.maximum if mut == "max_q" else np.minimum
    abs_td = np.abs(pick(qs[0], qs[1])[:, 0] - y[:, 0])
    abs_td_scale = np.maximum(qabs[0], qabs[1])[:, 0] + y_abs[:, 0]

    def dir_sens(u):
        """For a direction u in the row's layout, non-zero in the fc_out blocks only (no ReLU decision moves them beyond the
        forward error): (M_p |u_p| [row], per sample the scale of what its forward error moves <row, u> by [B])."""
        u = np.abs(np.asarray(u, dtype=np.float64))
        per = np.zeros(B)
        for k, (F, sens, sdh1, sdh2) in enumerate(parts):
            uo = u[k * PC + PC - NA * HID - NA:(k + 1) * PC]
            per += (sens * (F["H2"] @ uo[:NA * HID].reshape(NA, HID).T + uo[NA * HID:])).sum(1)
        return M * u, per
    return dict(row=row, M=M, N2=N2, Z=Z, T=T, abs_td=abs_td, abs_td_scale=abs_td_scale, y=y, y_abs=y_abs, q=qs, q_abs=qabs,
                count=float(val.sum()), dir_sens=dir_sens, amb_units=amb_units, amb_rows=amb_rows, head=td["head"])


def sac_actor_bucket_f64(batch: dict, actor, critics, log_alpha, bound=1.0, *, denom=None, relu_eps=0.0, tie_eps=0.0,
                         mut=None) -> dict:
    """The raw row k_sac_actor_grad writes, summed over the workgroups: the gradient of
        sum_s valid_s (alpha sum_d log pi_d - sum_d min(Q1, Q2)_d) / (2 B)
    through, per (sample, output column), the critic that holds the minimum -- exact ties go to critic 1, the kernel's rule
    (torch.minimum splits the gradient of an exact tie evenly between the two); then the loss, sum_s valid sum_d log pi, the valid
    fraction, 0.  batch: s [B, 100], valid [B], eps_cur [B, 2].
    Returns row [PA + 4] and, in its layout, M, N2 (what an error of its scale in the head's pre-activations moves a component
    by), C (M with every 1 - tanh^2 factor of the head's backward replaced by 1 + tanh^2: a saturated tanh leaves 1 - x^2 with an
    ABSOLUTE error of a few ulp of 1, which no multiple of M covers), Z (critic ReLU units within relu_eps and |Q1 - Q2| within tie_eps: the gradient may flow the other way; the actor's own
    layer-1 units within relu_eps), T (split dW1 tile scale); lp, lp_abs, q_abs; dir_sens(u); amb_units, amb_rows [B] (near ties included), near_tie [B, 2]."""
    X = np.asarray(batch["s"], dtype=np.float64)
    B = X.shape[0]
    D = float(B if denom is None else denom)
    val = np.asarray(batch["valid"], dtype=np.float64).reshape(-1)
    v = val[:, None]
    alpha = float(np.exp(np.float64(log_alpha)))
    W1, b1, Wh, bh = unflatten_actor(actor)
    hd = _actor_fwd(X, actor, batch["eps_cur"], mut)
    a = hd["act"] * bound
    F = [_critic_fwd(X, a, c) for c in critics]
    q1, q2 = F[0]["q"], F[1]["q"]
    take2 = (q2 > q1) if mut == "max_q" else (q2 < q1)
    qsel = np.where(take2, q2, q1)
    qsel_abs = np.where(take2, F[1]["q_abs"], F[0]["q_abs"])
    near = (np.abs(q1 - q2) <= tie_eps * (F[0]["q_abs"] + F[1]["q_abs"])) if tie_eps > 0.0 else np.zeros(q1.shape, dtype=bool)
    g_q = v / (2.0 * D)
    g_lp = alpha * v / (2.0 * D)
    da = np.zeros((B, 2))
    da_abs = np.zeros((B, 2))
    da_amb = np.zeros((B, 2))
    amb_units = 0
    amb_rows = near.any(1)
    for k in range(2):
        sel = take2 if k == 1 else ~take2
        dH1, _ = _critic_bwd(F[k], -g_q * sel)
        Wa = F[k]["net"][0][:, W:]
        da += dH1 @ Wa
        (m1, a1), (m2, a2) = _masks(F[k], relu_eps)
        adh1, _ = _critic_abs_bwd(F[k], g_q * (sel | near), m2, m1)
        da_abs += adh1 @ np.abs(Wa)
        # what may go the other way: the whole share of a near-tie output through this critic; the terms of ambiguous units
        t1, _ = _critic_abs_bwd(F[k], g_q * near, m2, m1)
        da_amb += t1 @ np.abs(Wa)
        if a1.any() or a2.any():
            full = g_q * (sel | near)
            z1, _ = _critic_abs_bwd(F[k], full, m2, a1.astype(np.float64))
            z2, _ = _critic_abs_bwd(F[k], full, a2.astype(np.float64), m1)
            da_amb += (z1 + z2) @ np.abs(Wa)
            amb_units += int(a1.sum() + a2.sum())
            amb_rows = amb_rows | a1.any(1) | a2.any(1)
    one_act = 1.0 - hd["act"] ** 2
    one_mu = 1.0 - hd["mu"] ** 2
    dsd_ds = (1.0 - hd["sd"] ** 2) * hd["sig"]
    g_sd = np.zeros_like(hd["sd"]) if mut == "no_log_sd" else g_lp / hd["sd"]

    def head_bwd(dact, with_sd):
        dns = dact * one_act
        return np.concatenate([dns * one_mu, (dns * hd["eps"] - (g_sd if with_sd else 0.0)) * dsd_ds], axis=1)

    def head_abs(dact_abs, with_sd, cancel=False):
        # cancel: every 1 - x^2 (x a tanh) by the magnitude of its terms, 1 + x^2 -- what an absolute error of the 1 is relative to
        oa, om, ds = (1.0 + hd["act"] ** 2, 1.0 + hd["mu"] ** 2, (1.0 + hd["sd"] ** 2) * hd["sig"]) if cancel else (one_act, one_mu, dsd_ds)
        dns = dact_abs * oa
        return np.concatenate([dns * om, (dns * np.abs(hd["eps"]) + (g_sd if with_sd else 0.0)) * ds], axis=1)
    dout = head_bwd(g_lp * hd["dlp_dact"] + bound * da, True)
    amb = (np.abs(hd["pre"]) <= relu_eps * hd["habs"]) if relu_eps > 0.0 else np.zeros(hd["pre"].shape, dtype=bool)
    mask_w = ((hd["pre"] > 0.0) | amb).astype(np.float64)
    dH = (dout @ Wh) * (hd["pre"] > 0.0)

    def flat(do, dh, Xm, Hm):
        return np.concatenate([(dh.T @ Xm).ravel(), dh.sum(0), (do.T @ Hm).ravel(), do.sum(0)])
    row, M, N2, Z, T = (np.zeros(PA + 4) for _ in range(5))
    row[:PA] = flat(dout, dH, X, hd["H"])
    lp_s = hd["lp"].sum(1)
    row[PA] = float(np.sum(val * (alpha * lp_s - qsel.sum(1)))) / (2.0 * D)
    row[PA + 1] = float(np.sum(val * lp_s))
    row[PA + 2] = float(val.sum()) / D
    ao = head_abs(g_lp * np.abs(hd["dlp_dact"]) + bound * da_abs, True)
    adh = (ao @ np.abs(Wh)) * mask_w
    M[:PA] = flat(ao, adh, np.abs(X), hd["H"])
    co = head_abs(g_lp * np.abs(hd["dlp_dact"]) + bound * da_abs, True, cancel=True)
    Cc = np.zeros(PA + 4)
    Cc[:PA] = flat(co, (co @ np.abs(Wh)) * mask_w, np.abs(X), hd["H"])
    M[PA] = float(np.sum(val * (alpha * np.abs(hd["lp"]).sum(1) + np.abs(qsel).sum(1)))) / (2.0 * D)
    M[PA + 1] = float(np.sum(val * (np.abs(hd["lp"]).sum(1) + 0.5 * (hd["eps"] ** 2).sum(1))))
    # what an error in the head's pre-activations (m, s), of scale (m_abs, s_abs), moves the head's backward by, to first order:
    # central differences of (d_mu, d_sd) in m and in s with everything else held (dQ / da is piecewise constant in a)
    def head_at(dm, ds):
        h2 = actor_head_f64(hd["o"][:, :2] + dm, hd["o"][:, 2:] + ds, hd["eps"], mut)
        dns = (g_lp * h2["dlp_dact"] + bound * da) * (1.0 - h2["act"] ** 2)
        gs = np.zeros_like(h2["sd"]) if mut == "no_log_sd" else g_lp / h2["sd"]
        return np.concatenate([dns * (1.0 - h2["mu"] ** 2), (dns * hd["eps"] - gs) * (1.0 - h2["sd"] ** 2) * h2["sig"]], axis=1)
    hstep = 2.0 ** -20
    j_m = np.abs(head_at(hstep, 0.0) - head_at(-hstep, 0.0)) / (2.0 * hstep)
    j_s = np.abs(head_at(0.0, hstep) - head_at(0.0, -hstep)) / (2.0 * hstep)
    so = j_m * np.concatenate([hd["m_abs"], hd["m_abs"]], axis=1) + j_s * np.concatenate([hd["s_abs"], hd["s_abs"]], axis=1)
    sdh = (so @ np.abs(Wh)) * mask_w
    N2[:PA] = flat(so ** 2, sdh ** 2, X ** 2, hd["H"] ** 2)
    N2[PA] = float(np.sum((val * (alpha * hd["lp_abs"].sum(1) + qsel_abs.sum(1)) / (2.0 * D)) ** 2))
    N2[PA + 1] = float(np.sum((val * hd["lp_abs"].sum(1)) ** 2))
    zo = head_abs(bound * da_amb, False)
    zdh = (zo @ np.abs(Wh)) * mask_w
    Z[:PA] = flat(zo, zdh, np.abs(X), hd["H"])
    if amb.any():
        zf = ((np.abs(dout) + zo) @ np.abs(Wh)) * amb
        Z[:HID * W + HID] += np.concatenate([(zf.T @ np.abs(X)).ravel(), zf.sum(0)])
    T[:HID * W] = _tile_scale(dH, X, W)

    def dir_sens(u):
        """u non-zero in the head blocks (fc_mu, fc_std and their biases) only: (M_p |u_p|, per sample what its head error moves
        <row, u> by, per sample what its ambiguous critic decisions may move it by)."""
        u = np.abs(np.asarray(u, dtype=np.float64))
        Uh, ub = u[HID * W + HID:HID * W + HID + 4 * HID].reshape(4, HID), u[PA - 4:PA]
        reach = hd["H"] @ Uh.T + ub
        return M * u, (so * reach).sum(1), (zo * reach).sum(1)
    return dict(row=row, M=M, N2=N2, Z=Z, T=T, C=Cc, lp=hd["lp"], lp_abs=hd["lp_abs"], q_abs=qsel_abs, count=float(val.sum()), head=hd,
                dir_sens=dir_sens, amb_units=amb_units + int(amb.sum()), amb_rows=amb_rows | amb.any(1), near_tie=near,
                act=a, q=(q1, q2))


def sample_contribution(fn, batch: dict, i: int, *args, **kw) -> np.ndarray:
    """The f64 row of sample i alone in a bucket of the same size (fn = sac_critic_bucket_f64 / sac_actor_bucket_f64): dropping or
    duplicating a sample is subtracting or adding this."""
    n = len(np.asarray(batch["valid"]).reshape(-1))
    one = {k: (None if v is None else np.asarray(v)[i:i + 1]) for k, v in batch.items()}
    return fn(one, *args, denom=n, **kw)["row"]


def sac_adam_f64(phase: str, raw, state: dict, t: int, lr: float, *, tau: float = 0.0, alpha_lr: float = 0.0,
                 target_entropy: float = 0.0, batch: int = 0, betas=(0.9, 0.999), eps: float = 1e-8) -> dict:
    """One k_sac_reduce_adam launch on the column sums `raw` of a phase's partial rows.  Every column is divided by the valid
    fraction (a fraction of 0 makes every gradient 0), then torch.optim.Adam.
    phase "critic": raw [2 PC + 4]; state w1, m1, v1, w2, m2, v2, t1, t2 -> the same keys after the step, the targets soft-updated
      (t' = t (1 - tau) + w' tau), losses [2].
    phase "actor": raw [PA + 4]; state w, m, v, log_alpha, alpha_mv [2] -> after the step; loss; the log_alpha step is Adam on
      d/d log_alpha of mean((-log pi - target_entropy) exp(log_alpha)) = exp(log_alpha) (-sum log pi / (2 B frac) - target_entropy)."""
    raw = np.asarray(raw, dtype=np.float64)
    out = {}
    if phase == "critic":
        frac = raw[2 * PC + 2]
        norm = 1.0 / frac if frac > 0.0 else 0.0
        for k in (1, 2):
            g = raw[(k - 1) * PC:k * PC] * norm
            w, m, v, _ = adam_step_f64(state[f"w{k}"][:PC], state[f"m{k}"][:PC], state[f"v{k}"][:PC], g, t, lr, betas, eps)
            out[f"w{k}"], out[f"m{k}"], out[f"v{k}"] = w, m, v
            out[f"t{k}"] = np.asarray(state[f"t{k}"][:PC], dtype=np.float64) * (1.0 - tau) + w * tau
            out[f"g{k}"] = g
        out["losses"] = raw[2 * PC:2 * PC + 2] * norm
        return out
    frac = raw[PA + 2]
    norm = 1.0 / frac if frac > 0.0 else 0.0
    g = raw[:PA] * norm
    out["w"], out["m"], out["v"], _ = adam_step_f64(state["w"][:PA], state["m"][:PA], state["v"][:PA], g, t, lr, betas, eps)
    out["g"] = g
    out["loss"] = raw[PA] * norm
    la = float(state["log_alpha"])
    gl = np.exp(la) * (-raw[PA + 1] * (0.5 / batch) * norm - target_entropy)
    nla, ma, va, _ = adam_step_f64(np.array([la]), state["alpha_mv"][:1], state["alpha_mv"][1:2], np.array([gl]), t, alpha_lr,
                                   betas, eps)
    out["log_alpha"], out["alpha_mv"], out["g_alpha"] = float(nla[0]), np.array([ma[0], va[0]]), float(gl)
    return out


def stress_actor(actor_flat, X, *, std_anchor=(((0.0, 16.0), (0.5, 20.0)), ((0.0, -11.0), (0.6, -4.7))), mu_span=8.0):
    """A stress actor from `actor_flat`, tuned on the rows X (every row a batch will ever hold): the two fc_std rows rescaled and
    shifted so that quantile q of dimension d's pre-activations lands on the anchored value -- dimension 0: minimum 16, median 20
    (both sides of the softplus threshold); dimension 1: minimum -11 (sd ~ 2e-5, never below -12), 60 % below log 0.01 -- and the
    fc_mu rows rescaled to a span of +-mu_span in opposite directions.  Returns the new flat block."""
    f = np.array(actor_flat, dtype=np.float64).reshape(-1)[:PA].copy()
    W1, b1, Wh, bh = unflatten_actor(f)
    H = np.maximum(np.asarray(X, dtype=np.float64) @ W1.T + b1, 0.0)
    o = H @ Wh.T + bh
    oW, ob = HID * W + HID, PA - 4
    for d in range(2):
        s = o[:, 2 + d]
        (q0, v0), (q1, v1) = std_anchor[d]
        s0, s1 = np.quantile(s, q0), np.quantile(s, q1)
        k = (v1 - v0) / (s1 - s0)
        f[oW + (2 + d) * HID:oW + (3 + d) * HID] *= k
        f[ob + 2 + d] = k * bh[2 + d] + (v0 - k * s0)
        m = o[:, d]
        k = (1.0 if d == 0 else -1.0) * 2.0 * mu_span / (m.max() - m.min())
        f[oW + d * HID:oW + (d + 1) * HID] *= k
        f[ob + d] = k * (bh[d] - 0.5 * (m.max() + m.min()))
    return f


def stress_coverage(hd: dict) -> dict:
    """Fractions of (sample, action dimension) pairs in each branch of the head, from _actor_fwd's / sac_*'s `head`."""
    s, sd, m = hd["o"][:, 2:], hd["sd"], hd["o"][:, :2]
    n = float(s.size)
    both = max(min(float((s[:, d] > 20).sum()), float((s[:, d] < 20).sum())) for d in range(2)) / n
    return dict(above20=float((s > 20).sum()) / n, below20_same_dim=both, small_sd=float((sd < 0.01).sum()) / n,
                mid_sd=float(((sd >= 0.01) & (sd < 0.9)).sum()) / n, big_mu=float((np.abs(m) > 3).sum()) / n, min_s=float(s.min()))


def assert_stress(hd: dict):
    c = stress_coverage(hd)
    assert c["above20"] >= 0.05 and c["below20_same_dim"] >= 0.05 and c["small_sd"] >= 0.05 and c["mid_sd"] >= 0.05 and \
        c["big_mu"] >= 0.05 and c["min_s"] >= -12.0, c
    return c


def actor_forward(X, actor, eps, mut=None) -> dict:
    """The actor's forward (head included) on rows X with draws eps: see actor_head_f64; plus o, m_abs, s_abs, lp_abs."""
    return _actor_fwd(np.asarray(X, dtype=np.float64), actor, eps, mut)


def act_bar(hd: dict, tau_td: float, u: float):
    """The acting bar on |action - act| per (row, action dimension), hd from actor_forward: the head's pre-activations within tau_td
    of their |.|-forward, carried to the action to first order, plus 8 u for the four tanhf / expf / log1pf calls and the product
    sd eps on values of size <= 1 + |eps| (derived in tests/test_sac_grad_kernels_gpu.py::test_act_on_the_stress_actor)."""
    one_act, one_mu = 1 - hd["act"] ** 2, 1 - hd["mu"] ** 2
    dsd = (1 - hd["sd"] ** 2) * hd["sig"]
    return tau_td * one_act * (one_mu * hd["m_abs"] + np.abs(hd["eps"]) * dsd * hd["s_abs"]) + 8 * u * (1 + np.abs(hd["eps"]))


def act_launch_map(n_slots: int, count: int, budget: int = 512) -> dict:
    """How uavenv_sac_act_multi spreads one slot's `count` agents: max(1, budget / n_slots) workgroups per slot (budget =
    UAVENV_SAC_ACT_WGS, 512 unless set), 64 agents per tile, tile t to workgroup t mod gx on trip t div gx.
    -> gx, tiles, trips, trip [tiles], wg [tiles], last (rows of the last tile), late (workgroups that take the last trip)."""
    gx = max(1, budget // n_slots)
    tiles = (count + TILE - 1) // TILE
    t = np.arange(tiles)
    trip, wg = t // gx, t % gx
    return dict(gx=gx, tiles=tiles, trips=int(trip.max()) + 1, trip=trip, wg=wg, last=count - (tiles - 1) * TILE,
                late=int((trip == trip.max()).sum()))
