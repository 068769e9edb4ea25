"""Float64 statement of the DQN acting step -- Q(s) of q_local followed by the epsilon-greedy choice of
Trainer/DuelingDQN_Trainer.py:86-97 -- which every acting form of the device computes (csrc/learner.hip: k_dqn_act*,
csrc/replay.hip: k_select_actions, the policy prologues of csrc/uavenv.hip), written from the mathematics and from
oracle/philox.py's stream so that each form can be held against it.  CPU only (numpy); test infrastructure, not product code.

Only tests/ may import this module.

The forward and its |.|-propagated twin are oracle/dqn_grad_ref.py's (forward_f64, q_abs_f64): the network, its flat layout and
the dueling combine are stated once.  The draw of row i of call (seed, counter) is act_draws' u_i and rnd_i, keyed by the ROW
INDEX, both halves of seed and of counter: greedy iff float32(u_i) > float32(eps), the FIRST maximum on ties (torch.max), else
rnd_i = floor(word1 * A / 2^32).  steer = -1 + 2 a / (A - 1) in f64, rounded to f32.

f16-MFMA forms (k_dqn_act_h, polh_wave): the observation rows, fc1 AND b1 (column 100 of the staged fc1 tile, against a ones
column) are rounded to f16 by xh_commit / wh_commit; products of two f16 values are exact in f32, the sums are f32, and layer 2
runs in f32 on the unrounded H.  f16_operands() rounds exactly those and nothing else.

MUTATIONS: deliberate errors of the f64 side, for the tests' self-checks (a check that cannot tell the kernel from a mutant of
the reference is no check).  Forward: "flag_f16" (fc1's flag columns rounded to f16: the split layer 1 without its mid * 2^-11
term), "flag_col" (the fc1 column of the given flag zeroed), "b1" / "b2" (the bias of the given unit / output dropped),
"mean_a1" (the dueling mean over A + 1).  Decision: "last_max", "ge", "rnd_from_u" (floor(u A)), "counter_lo", "seed_lo".
"""
from __future__ import annotations

import numpy as np

from oracle.dqn_grad_ref import forward_f64, q_abs_f64, unflatten
from oracle.philox import act_draws

W, HID = 100, 64
FLAG_COLS = np.array(list(range(11, 86)) + list(range(90, 95)))      # the 80 0 / 1 columns of state_PathPlan (Agents/UAV.py:533-566)
FORWARD_MUTATIONS = ("flag_f16", "flag_col", "b1", "b2", "mean_a1")
DECISION_MUTATIONS = ("last_max", "ge", "rnd_from_u", "counter_lo", "seed_lo")


def f16_round(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def f16_operands(X, flat_params):
    """(X, flat) as the f16-MFMA forms see them: rows, fc1 and b1 rounded to f16 (layer 2 untouched)."""
    fl = np.asarray(flat_params, dtype=np.float64).copy()
    n1 = HID * W + HID
    fl[:n1] = f16_round(fl[:n1])
    return f16_round(X), fl


def steer_of(a, n_actions: int):
    return (-1.0 + 2.0 * np.asarray(a, dtype=np.float64) / float(n_actions - 1)).astype(np.float32)


def first_argmax(q):
    """torch.max(1)[1] / the kernels' `q[k] > best` scan: the lowest index among equal maxima (+-inf compare like numbers)."""
    return np.argmax(np.asarray(q), axis=1).astype(np.int64)


def last_argmax(q):
    q = np.asarray(q)
    return (q.shape[1] - 1 - np.argmax(q[:, ::-1], axis=1)).astype(np.int64)


def draws(n: int, seed: int, counter: int, n_actions: int, first_row: int = 0, mut=None):
    """u [n] f32, rnd [n] of rows first_row .. first_row + n - 1 of call (seed, counter)."""
    if mut == "counter_lo":
        counter &= 0xFFFFFFFF
    if mut == "seed_lo":
        seed &= 0xFFFFFFFF
    u, rnd = act_draws(first_row + n, seed, counter, n_actions)
    u, rnd = u[first_row:], rnd[first_row:]
    if mut == "rnd_from_u":
        rnd = np.floor(u.astype(np.float64) * n_actions).astype(np.int64)
    return u, rnd


def decide(q, u, rnd, eps, mut=None):
    """The action of every row of a [n, A] table: greedy (first maximum) where float32(u) > float32(eps), else rnd."""
    e = np.float32(eps)
    greedy = (u.astype(np.float32) >= e) if mut == "ge" else (u.astype(np.float32) > e)
    best = last_argmax(q) if mut == "last_max" else first_argmax(q)
    return np.where(greedy, best, rnd).astype(np.int64)


def act_f64(X, flat_params, *, n_actions: int, dueling: bool, eps: float, seed: int, counter: int, first_row: int = 0,
            f16: bool = False, mut=None, mut_arg: int = 0) -> dict:
    """X [n, 100] observation rows, flat_params: q_local's flat block (FusedDQNLearner._bind layout).  Returns a dict:
      Q      [n, A]  f64 Q values;  q_abs [n, A]  the |.|-propagated forward (the scale of a rounding error in Q)
      u, rnd [n]     the epsilon-greedy stream of rows first_row ..;  greedy [n]: float32(u) > float32(eps)
      decide(q)      the action of every row for ANY [n, A] table (the kernels' own Q values): greedy -> first maximum, else rnd
      index, steer   decide(Q) and its steer
      steer_of(a)    -1 + 2 a / (A - 1), f64 rounded to f32
    f16: the operands of the f16-MFMA forms (f16_operands).  mut / mut_arg: one of the module's MUTATIONS."""
    A = int(n_actions)
    n2 = A + (1 if dueling else 0)
    X = np.asarray(X, dtype=np.float64)
    fl = np.asarray(flat_params, dtype=np.float64).reshape(-1)
    if f16:
        X, fl = f16_operands(X, fl)
    W1, b1, W2, b2 = (p.copy() for p in unflatten(fl, W, HID, n2))
    if mut == "flag_f16":
        W1[:, FLAG_COLS] = f16_round(W1[:, FLAG_COLS])
    elif mut == "flag_col":
        W1[:, mut_arg] = 0.0
    elif mut == "b1":
        b1[mut_arg] = 0.0
    elif mut == "b2":
        b2[mut_arg] = 0.0
    elif mut is not None and mut not in FORWARD_MUTATIONS + DECISION_MUTATIONS:
        raise ValueError(mut)
    _, _, Q = forward_f64(X, W1, b1, W2, b2, dueling, A)
    if mut == "mean_a1":
        if not dueling:
            raise ValueError("mean_a1 mutates the dueling combine")
        out = np.maximum(X @ W1.T + b1, 0.0) @ W2.T + b2
        Q = out[:, A:A + 1] + out[:, :A] - out[:, :A].sum(axis=1, keepdims=True) / (A + 1)
    qa = q_abs_f64(X, *unflatten(fl, W, HID, n2), dueling, A)
    n = X.shape[0]
    u, rnd = draws(n, seed, counter, A, first_row, mut)

    def _decide(q):
        q = np.asarray(q)
        assert q.shape == (n, A), q.shape
        return decide(q, u, rnd, eps, mut)
    index = _decide(Q)
    return dict(Q=Q, q_abs=qa, u=u, rnd=rnd, greedy=u > np.float32(eps), decide=_decide, index=index,
                steer=steer_of(index, A), steer_of=lambda a: steer_of(a, A))
