"""Float64 statement of one DQN-family gradient bucket and one Adam step -- the operation csrc/learner.hip's gradient kernels
(k_dqn_grad*, td_backward) followed by k_dqn_reduce / k_dqn_reduce_adam compute, written from the mathematics so that every
kernel form can be held against it.  CPU only (numpy); test infrastructure, not product code.

Network (nets.py, the flat layout of FusedDQNLearner._bind): H = relu(X W1^T + b1), out = H W2^T + b2 with
  Qnet2:  Q = out (n2 = n_actions rows of W2)
  VAnet2: rows 0..A-1 of W2 are fc_A, row A is fc_V; Q = V + A - mean(A)
TD target y = r + gamma * (1 - done) * Q_target(s', a') with a' = argmax_a Q_target(s', a) (kind "dqn") or
a' = argmax_a Q_local(s', a), first maximum on ties (kind "ddqn" / "dueling", DDQN_Trainer.py:94).
delta = Q_local(s, a) - y; per-sample loss delta^2 (MSE, dq = 2 delta) or smooth-L1 with threshold 1 (Huber, dq = clamp(delta,
-1, 1)); dq and the loss are multiplied by valid and by the importance-sampling weight.
"""
from __future__ import annotations

import numpy as np

TD_FLOOR = 2.0 ** -20      # |delta| is widened by this times (|q_a| + |y|) in the absolute sums M (a fitted batch keeps a bound)


def layout(w: int, hid: int, n2: int):
    """Offsets of W1, b1, W2, b2 in the flat parameter block; total P."""
    o_b1 = hid * w
    o_w2 = o_b1 + hid
    o_b2 = o_w2 + n2 * hid
    return o_b1, o_w2, o_b2, o_b2 + n2


def unflatten(flat, w: int, hid: int, n2: int):
    flat = np.asarray(flat, dtype=np.float64).reshape(-1)
    o_b1, o_w2, o_b2, P = layout(w, hid, n2)
    assert flat.size == P, (flat.size, P)
    return flat[:o_b1].reshape(hid, w), flat[o_b1:o_w2], flat[o_w2:o_b2].reshape(n2, hid), flat[o_b2:P]


def forward_f64(X, W1, b1, W2, b2, dueling: bool, A: int):
    pre = X @ W1.T + b1
    H = np.maximum(pre, 0.0)
    out = H @ W2.T + b2
    if dueling:
        adv = out[:, :A]
        Q = out[:, A:A + 1] + adv - adv.mean(axis=1, keepdims=True)
    else:
        Q = out[:, :A]
    return pre, H, Q


def q_abs_f64(X, W1, b1, W2, b2, dueling: bool, A: int):
    """|.|-propagated forward: a bound on the magnitude of every term a forward pass of Q sums, per sample and action."""
    habs = np.abs(X) @ np.abs(W1).T + np.abs(b1)
    oabs = habs @ np.abs(W2).T + np.abs(b2)
    if dueling:
        aabs = oabs[:, :A]
        return oabs[:, A:A + 1] + aabs + aabs.mean(axis=1, keepdims=True)
    return oabs[:, :A]


def dqn_grad_f64(s, s2, actions, rewards, dones, valid, local, target, *, kind: str, dueling: bool, n_actions: int,
                 gamma: float, huber: bool, is_weights=None, w: int = 100, hid: int = 64, td_floor: float = TD_FLOOR,
                 relu_eps: float = 0.0, tie_eps: float = 0.0, next_action=None, per_sample: bool = False) -> dict:
    """One gradient bucket in float64.

    s, s2 [B, w]: observation rows of s and s'; actions (ints), rewards, dones, valid (0 / 1) and optional is_weights [B];
    local / target: the flat parameter blocks (FusedDQNLearner._bind layout).  Returns a dict:
      grad   [P]  sum_s d(w_s valid_s loss_s)/d theta, in the flat layout (what the kernels put in raw[:P])
      loss   sum_s w_s valid_s loss_s (raw[P]);  count = sum_s valid_s (raw[P + 1])
      abs_td [B]  |delta_s| (written for every row, valid or not)
      q_a, y [B]  Q_local(s, a_s) and the TD target
      q_abs  [B]  sum of the magnitudes of the terms behind delta_s: |.|-forward of Q_local(s, a_s) plus |r| plus
                  gamma (1 - done) times that of the bootstrap value (the scale of a rounding error in delta_s)
      M      [P]  sum_s |contribution_{s,p}| with |delta_s| widened to |delta_s| + td_floor (|q_a| + |y|), ReLU masks widened to
                  units whose pre-activation is within 2^-16 of their |.|-forward of zero
      N      [P]  sum_s q_abs_s |d contribution_{s,p} / d delta_s|: the sensitivity of component p to errors in the deltas
      Z      [P]  the terms an arithmetic within its error bound may legitimately decide the other way: for every hidden unit
                  whose pre-activation is within relu_eps of its |.|-forward of zero, the whole |dH x| and |dH| terms (the ReLU
                  mask may flip); for every ddqn / dueling sample whose two best Q_local(s') are within tie_eps of their
                  |.|-forward, the |.|-backward of the change in dq if the second were picked.  Zero with both eps at 0.
      td_amb [B]  |delta_alt - delta| of those near-tie samples (0 elsewhere)
      N2     [P]  sum_s (q_abs_s |d contribution_{s,p} / d delta_s|)^2: with errors in the deltas independent between samples,
                  their effect on component p is of root-sum-square size sqrt(N2_p), not N_p
      dir_sens(u)  for a direction u [P]: (M_p |u_p| [P], q_abs_s <|d contribution_s / d delta_s|, |u|> [B], the |.| of what
                  each ReLU within relu_eps moves <error, u> by if it flips [number of such (sample, unit) pairs]) -- the scales of
                  what component p's roundings, sample s's delta error and one flipped unit contribute to <error, u>
      M_loss, N_loss, N2_loss, Z_loss  the same sums for the loss sum
      a_next, a_alt, near_tie  the bootstrap action used, the runner-up, and which samples are within tie_eps
    next_action (ddqn / dueling, optional [B] ints, -1 = argmax): the bootstrap action of a near-tie sample as the arithmetic under
    test decided it (read back from its |TD error|); such a sample is then no longer ambiguous.
      per_sample_grad [B, P]  (per_sample=True only) each sample's contribution to grad, so that sum(axis=0) == grad
    """
    if kind not in ("dqn", "ddqn", "dueling"):
        raise ValueError(kind)
    A = int(n_actions)
    n2 = A + (1 if dueling else 0)
    X = np.asarray(s, dtype=np.float64)
    X2 = np.asarray(s2, dtype=np.float64)
    B = X.shape[0]
    act = np.asarray(actions).astype(np.int64).reshape(-1)
    rew = np.asarray(rewards, dtype=np.float64).reshape(-1)
    done = np.asarray(dones, dtype=np.float64).reshape(-1)
    val = np.asarray(valid, dtype=np.float64).reshape(-1)
    isw = np.ones(B) if is_weights is None else np.asarray(is_weights, dtype=np.float64).reshape(-1)
    if np.any((act < 0) | (act >= A)):
        raise ValueError("action out of range")
    Wl = unflatten(local, w, hid, n2)
    Wt = unflatten(target, w, hid, n2)
    rows = np.arange(B)

    pre, H, Q = forward_f64(X, *Wl, dueling, A)
    _, _, Qt2 = forward_f64(X2, *Wt, dueling, A)
    qabs_l = q_abs_f64(X, *Wl, dueling, A)
    qabs_t = q_abs_f64(X2, *Wt, dueling, A)
    near = np.zeros(B, dtype=bool)
    if kind == "dqn":
        a_next = np.argmax(Qt2, axis=1)          # the value is the max whichever maximum is taken
        a_alt = a_next
    else:
        _, _, Ql2 = forward_f64(X2, *Wl, dueling, A)
        a_next = np.argmax(Ql2, axis=1)          # first maximum, as torch.max
        order = np.argsort(-Ql2, axis=1, kind="stable")
        a_alt = order[:, 1]
        qabs_l2 = q_abs_f64(X2, *Wl, dueling, A)
        gap = Ql2[rows, a_next] - Ql2[rows, a_alt]
        near = gap <= tie_eps * (qabs_l2[rows, a_next] + qabs_l2[rows, a_alt])
        if tie_eps == 0.0:
            near[:] = False
        if next_action is not None:
            na = np.asarray(next_action).astype(np.int64).reshape(-1)
            given = near & (na >= 0)
            a_next = np.where(given, na, a_next)
            a_alt = np.where(given & (na == a_alt), order[:, 0], a_alt)
            near = near & ~given
    q_next = Qt2[rows, a_next]
    q_a = Q[rows, act]
    y = rew + gamma * q_next * (1.0 - done)
    delta = q_a - y
    ad = np.abs(delta)
    wide = ad + td_floor * (np.abs(q_a) + np.abs(y))
    scale = val * isw
    if huber:
        per = np.where(ad < 1.0, 0.5 * delta * delta, ad - 0.5)
        dq = np.clip(delta, -1.0, 1.0)
        dq_sens = np.ones(B)                    # dq is 1-Lipschitz in delta, on either side of the threshold
        adw = np.minimum(wide, 1.0)
        per_w = np.where(wide < 1.0, 0.5 * wide * wide, wide - 0.5)
        dper_sens = np.minimum(wide, 1.0)       # |d per / d delta|
    else:
        per = delta * delta
        dq = 2.0 * delta
        dq_sens = np.full(B, 2.0)
        adw = 2.0 * wide
        per_w = wide * wide
        dper_sens = 2.0 * wide
    # the bootstrap value of a near-tie sample if the other action were picked
    delta_alt = q_a - (rew + gamma * Qt2[rows, a_alt] * (1.0 - done))
    td_amb = np.where(near, np.abs(delta_alt - delta), 0.0)
    if huber:
        dq_alt = np.clip(delta_alt, -1.0, 1.0)
        per_alt = np.where(np.abs(delta_alt) < 1.0, 0.5 * delta_alt ** 2, np.abs(delta_alt) - 0.5)
    else:
        dq_alt, per_alt = 2.0 * delta_alt, delta_alt ** 2
    dq_amb = np.where(near, np.abs(dq_alt - dq), 0.0)
    per_amb = np.where(near, np.abs(per_alt - per), 0.0)
    dq = dq * scale
    q_abs = qabs_l[rows, act] + np.abs(rew) + gamma * (1.0 - done) * qabs_t[rows, a_next]

    # dL/d out: coefficient of dq per output column
    coef = np.zeros((B, n2))
    if dueling:
        coef[:, :A] = -1.0 / A
        coef[rows, act] += 1.0
        coef[:, A] = 1.0
    else:
        coef[rows, act] = 1.0
    W1, b1, W2, b2 = Wl
    dout = dq[:, None] * coef
    dH = (dout @ W2) * (pre > 0.0)
    g_W2 = dout.T @ H
    g_b2 = dout.sum(axis=0)
    g_W1 = dH.T @ X
    g_b1 = dH.sum(axis=0)
    grad = np.concatenate([g_W1.ravel(), g_b1, g_W2.ravel(), g_b2])

    # absolute sums: the same backward on magnitudes
    habs = np.abs(X) @ np.abs(W1).T + np.abs(b1)
    amb = np.abs(pre) <= relu_eps * habs
    if relu_eps == 0.0:
        amb[:] = False
    mask_w = ((pre > 0.0) | amb).astype(np.float64)

    def abs_backward(d, mask):                  # d [B]: magnitude of dq (or of its sensitivity), already >= 0
        ao = d[:, None] * np.abs(coef)
        adh = (ao @ np.abs(W2)) * mask
        return np.concatenate([(adh.T @ np.abs(X)).ravel(), adh.sum(axis=0), (ao.T @ H).ravel(), ao.sum(axis=0)])
    M = abs_backward(adw * np.abs(scale), mask_w)
    N = abs_backward(q_abs * dq_sens * np.abs(scale), mask_w)
    Z = abs_backward(dq_amb * np.abs(scale), mask_w)
    sens = q_abs * dq_sens * np.abs(scale)
    ao2 = sens[:, None] * np.abs(coef)
    adh2 = (ao2 @ np.abs(W2)) * mask_w
    N2 = np.concatenate([((adh2 ** 2).T @ (X ** 2)).ravel(), (adh2 ** 2).sum(axis=0), ((ao2 ** 2).T @ (H ** 2)).ravel(),
                         (ao2 ** 2).sum(axis=0)])
    nW1, nb1, nW2 = W1.size, b1.size, W2.size

    def dir_sens(u):
        u = np.abs(np.asarray(u, dtype=np.float64))
        U1 = u[:nW1].reshape(W1.shape)
        ub1 = u[nW1:nW1 + nb1]
        U2 = u[nW1 + nb1:nW1 + nb1 + nW2].reshape(W2.shape)
        ub2 = u[nW1 + nb1 + nW2:]
        per_s = (adh2 * (np.abs(X) @ U1.T + ub1)).sum(axis=1) + (ao2 * (H @ U2.T + ub2)).sum(axis=1)
        zs = (np.abs(X) @ U1.T + ub1) * flip_dh
        return M * u, per_s, zs[amb]
    flip_dh = (np.maximum(np.abs(dq), dq_amb * np.abs(scale))[:, None] * np.abs(coef)) @ np.abs(W2)
    if amb.any():                               # a flipped ReLU mask moves the whole dH x term, not a rounding of it
        zf = abs_backward(np.maximum(np.abs(dq), dq_amb * np.abs(scale)), amb.astype(np.float64))
        Z[:W1.size + b1.size] += zf[:W1.size + b1.size]

    out = dict(grad=grad, loss=float(np.sum(per * scale)), count=float(np.sum(val)), abs_td=ad, q_a=q_a, y=y, q_abs=q_abs,
               M=M, N=N, M_loss=float(np.sum(per_w * np.abs(scale))),
               N_loss=float(np.sum(q_abs * dper_sens * np.abs(scale))), Z=Z, Z_loss=float(np.sum(per_amb * np.abs(scale))),
               N2=N2, N2_loss=float(np.sum((q_abs * dper_sens * np.abs(scale)) ** 2)), dir_sens=dir_sens,
               td_amb=td_amb, delta_alt=delta_alt, a_next=a_next, a_alt=a_alt, near_tie=near)
    if per_sample:
        ps = np.empty((B, grad.size))
        for i in range(B):
            ps[i] = np.concatenate([np.outer(dH[i], X[i]).ravel(), dH[i], np.outer(dout[i], H[i]).ravel(), dout[i]])
        out["per_sample_grad"] = ps
    return out


def sample_contribution(batch: dict, i: int, **kw) -> dict:
    """The f64 contribution of sample i alone (grad, loss, count) -- for the mutation self-checks: dropping or duplicating a
    sample of the bucket is subtracting or adding this."""
    one = {k: (None if v is None else np.asarray(v)[i:i + 1]) for k, v in batch.items()}
    if kw.get("next_action") is not None:
        kw = dict(kw, next_action=np.asarray(kw["next_action"])[i:i + 1])
    return dqn_grad_f64(one["s"], one["s2"], one["actions"], one["rewards"], one["dones"], one["valid"], **kw,
                        is_weights=one.get("is_weights"))


def adam_step_f64(w, m, v, mean_grad, t: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, hard: bool = False,
                  target=None):
    """torch.optim.Adam (amsgrad off, no weight decay), the formula of k_dqn_adam / k_dqn_reduce_adam, in float64:
    m' = m + (g - m)(1 - b1), v' = b2 v + (1 - b2) g^2, w' = w - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps).
    Returns (w', m', v', target') with target' = w' when hard, else the given target (or None)."""
    b1, b2 = betas
    g = np.asarray(mean_grad, dtype=np.float64)
    m1 = np.asarray(m, dtype=np.float64) + (g - np.asarray(m, dtype=np.float64)) * (1.0 - b1)
    v1 = np.asarray(v, dtype=np.float64) * b2 + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    w1 = np.asarray(w, dtype=np.float64) - (lr / bc1) * (m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps))
    t1 = w1.copy() if hard else (None if target is None else np.asarray(target, dtype=np.float64))
    return w1, m1, v1, t1
