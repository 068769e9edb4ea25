"""Host model of the reset bank's three row movements, written from include/uavenv.h (not from the kernels):

  * fix_up   uavenv_plan_scenarios: "Scenarios whose planner gave up or whose path does not fit K take the next valid
             scenario's start / goal / path" -- next = cyclically, valid = as the planner left it;
  * commit   uavenv_replan_commit: "a row takes its new start / goal / sub-goal list unless an agent currently flies it or
             the new plan is unusable; such rows keep their old plan", force: "every usable plan is taken";
  * flown_rows  which bank row every agent holds: uavenv_reset_all / the step's auto-reset draw "scenario ~ U{0..M-1} from a
             counter-based Philox stream keyed by (seed, agent)" at the tick of the launch (oracle.philox.reset_draws).

Everything is integer and byte movement: the model predicts the bank bit for bit.  Pure numpy; a bank (and a staged slice)
is the tuple (start_goal [m, 6] f64, sub_goals [m, K, 3] f64, n_sub [m] int32) that VecPathPlanEnv.bank_read returns."""
from __future__ import annotations

import numpy as np

from . import philox


def usable(n_sub, K: int):
    """A plan the env can fly: at least start and goal, and it fits the K slots (the planner reports 1 = gave up,
    -n = needs n > K slots)."""
    n = np.asarray(n_sub)
    return (n >= 2) & (n <= K)


def same_bank(a, b) -> bool:
    """The comparison every bank test uses: start/goal, all K x 3 slots of every list and n_sub, bit for bit."""
    return len(a) == 3 and len(b) == 3 and all(np.asarray(x).shape == np.asarray(y).shape and np.array_equal(x, y)
                                               for x, y in zip(a, b))


def fix_up(sg, sub, n_sub, K: int):
    """-> (sg', sub', n_sub', replaced).  Every unusable row i takes row (i + d) % m for the smallest d >= 1 whose ORIGINAL
    n_sub is usable: all three arrays from that one row, sources never rows patched here.  replaced counts the unusable rows
    (also when there is no usable row to take: then nothing moves and the caller refuses the bank)."""
    sg, sub, n_sub = np.array(sg, dtype=np.float64), np.array(sub, dtype=np.float64), np.array(n_sub, dtype=np.int32)
    m = len(n_sub)
    good = usable(n_sub, K)
    src = np.arange(m)
    if good.any():
        for i in np.nonzero(~good)[0]:
            src[i] = next((i + d) % m for d in range(1, m) if good[(i + d) % m])
    return sg[src], sub[src], n_sub[src], int((~good).sum())


def commit(bank, staged, first: int, in_use, K: int, force: bool):
    """-> (bank', (committed, skipped_in_use, skipped_no_plan)).  Bank row first + r takes staged row r if the staged row is
    usable and (the bank row is not in use, or force); every other row of the bank is unchanged.  in_use: bool [m] over the
    BANK's rows.  A skipped row is counted once: in use (which force never is) before no plan."""
    sg, sub, ns = (np.array(x) for x in bank)
    s_sg, s_sub, s_ns = (np.asarray(x) for x in staged)
    count = len(s_ns)
    rows = first + np.arange(count)
    held = np.zeros(count, bool) if force else np.asarray(in_use, dtype=bool)[rows]
    take = usable(s_ns, K) & ~held
    sg[rows[take]], sub[rows[take]], ns[rows[take]] = s_sg[take], s_sub[take], s_ns[take]
    return (sg, sub, ns), (int(take.sum()), int(held.sum()), int((~take & ~held).sum()))


def in_use_mask(rows, m: int):
    """bool [m]: the bank rows some agent holds (rows < 0: a private list, no bank row)."""
    rows = np.asarray(rows)
    mask = np.zeros(m, bool)
    mask[rows[(rows >= 0) & (rows < m)]] = True
    return mask


def flown_rows(N: int, seed: int, resets, m: int):
    """The scenario id each of the N agents holds after `resets`, a list of (tick, mask [N] of the agents re-drawn at that
    tick) in launch order, or (tick, mask, m_then) where the bank had another size than m.  uavenv_reset_all is
    (0, everyone); -1 = never reset."""
    rows = np.full(N, -1, np.int64)
    for entry in resets:
        tick, mask = entry[0], np.asarray(entry[1], dtype=bool)
        scn, _ = philox.reset_draws(N, seed, int(tick), int(entry[2]) if len(entry) > 2 else m)
        rows[mask] = scn[mask]
    return rows
