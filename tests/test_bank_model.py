"""oracle/bank_model.py on the host: the model does what include/uavenv.h says on inputs small enough to check by hand, and
the comparison the GPU tests use (same_bank + the counters, tests/test_bank_lifecycle_gpu.py) tells the model from every
plausible wrong fix-up / commit -- each of which still leaves "valid paths" in the bank."""
import numpy as np
import pytest

from oracle import philox as px
from oracle.bank_model import commit, fix_up, flown_rows, in_use_mask, same_bank, usable

K = 5


def _rows(m, tag=0.0):
    """m rows that identify themselves in every double (also the unusable ones, also past n_sub)."""
    r = np.arange(m, dtype=np.float64)[:, None]
    sg = tag + 100.0 * r + np.arange(6) / 8.0
    sub = (tag + 100.0 * r + 10.0 + np.arange(K * 3) / 4.0).reshape(m, K, 3)
    return sg, sub


def _bank(n_sub, tag=0.0):
    n = np.asarray(n_sub, np.int32)
    return (*_rows(len(n), tag), n)


# n_sub as the planner reports it: 1 = gave up, -n = needs n > K slots; 0 and K + 1 for the bounds of usable()
WRAP = [3, 1, -7, 0, 5, 2, 6, 4, 1, -9, 1]           # rows 1..3: a run of three; rows 8..10: a run that wraps onto row 0
BOTH_ENDS = [1, -6, 4, 3, 1, 2, -8, 1]                # rows 6, 7, 0, 1: a run of four across the wrap
ONE_OF_TWO = [-6, 2]
FIX_INPUTS = {"wrap": WRAP, "both_ends": BOTH_ENDS, "one_of_two": ONE_OF_TWO}


def test_usable_is_two_to_K():
    assert usable([-3, 0, 1, 2, K, K + 1], K).tolist() == [False, False, False, True, True, False]


def test_fix_up_by_hand():
    sg, sub, ns = _bank(WRAP)
    g, s, n, replaced = fix_up(sg, sub, ns, K)
    src = [0, 4, 4, 4, 4, 5, 7, 7, 0, 0, 0]
    assert replaced == 7 and n.tolist() == [WRAP[j] for j in src]
    assert np.array_equal(g, sg[src]) and np.array_equal(s, sub[src])
    assert np.array_equal(ns, WRAP) and np.array_equal(sg, _rows(len(WRAP))[0])           # the inputs are left alone
    g, s, n, replaced = fix_up(*_bank(BOTH_ENDS), K)
    src = [2, 2, 2, 3, 5, 5, 2, 2]
    assert replaced == 5 and np.array_equal(g, _rows(8)[0][src]) and np.array_equal(s, _rows(8)[1][src])
    g, s, n, replaced = fix_up(*_bank(ONE_OF_TWO), K)
    assert replaced == 1 and n.tolist() == [2, 2] and np.array_equal(g[0], g[1]) and np.array_equal(s[0], s[1])
    # no usable row: counted, nothing moves (the library then refuses the bank)
    none = _bank([1, -6, 0])
    out = fix_up(*none, K)
    assert out[3] == 3 and same_bank(out[:3], none)
    alone = _bank([1])
    assert fix_up(*alone, K)[3] == 1 and fix_up(*_bank([2]), K)[3] == 0


# ---- wrong fix-ups: each leaves only usable-looking rows behind wherever the right one does
def _next_usable(good, i, span):
    return next(((i + d) % len(good) for d in span if good[(i + d) % len(good)]), None)


def _fix_with(pick_sg, pick_sub=None):
    def f(sg, sub, ns, K):
        good = usable(ns, K)
        a = np.array([i if good[i] or pick_sg(good, i) is None else pick_sg(good, i) for i in range(len(ns))])
        pick = pick_sub or pick_sg
        b = np.array([i if good[i] or pick(good, i) is None else pick(good, i) for i in range(len(ns))])
        return sg[a], sub[b], ns[b], int((~good).sum())
    return f


def _fix_chained(sg, sub, ns, K):
    """Sources chosen in place (a patched row's n_sub passes for usable at once, rows visited from the top down), contents
    copied afterwards from what the rows held BEFORE: a patched row hands on its unusable start / goal / list."""
    m, now = len(ns), np.array(ns)
    src = np.arange(m)
    for i in range(m - 1, -1, -1):
        if not usable(now[i], K):
            j = _next_usable(usable(now, K), i, range(1, m))
            if j is not None:
                src[i], now[i] = j, now[j]
    return sg[src], sub[src], now, int((~usable(ns, K)).sum())


FIX_MUTANTS = {
    "previous": _fix_with(lambda good, i: _next_usable(good, i, range(-1, -len(good), -1))),
    "no_wrap": _fix_with(lambda good, i: _next_usable(good, i, range(1, len(good) - i))),
    "chained": _fix_chained,
    "sub_and_start_goal_from_two_rows": _fix_with(lambda good, i: _next_usable(good, i, range(1, len(good))),
                                                  lambda good, i: _next_usable(good, i, range(-1, -len(good), -1))),
}


def _longest_run(bad):
    bad = np.asarray(bad)
    if bad.all():
        return len(bad)
    two = np.r_[bad, bad]
    return max(len(r) for r in "".join("x" if b else " " for b in two).split())


@pytest.mark.parametrize("name", sorted(FIX_MUTANTS))
def test_the_comparison_rejects_every_wrong_fix_up(name):
    mutant = FIX_MUTANTS[name]
    caught = {}
    for key, n_sub in FIX_INPUTS.items():
        bank = _bank(n_sub)
        want, got = fix_up(*bank, K), mutant(*bank, K)
        assert name == "no_wrap" or usable(got[2], K).all()                  # "valid paths" all the same
        caught[key] = not (same_bank(want[:3], got[:3]) and want[3] == got[3])
    assert caught["wrap"], caught                                            # the input with the run of >= 3 and the wrap
    assert _longest_run(~usable(WRAP, K)) >= 3 and not usable(WRAP, K)[-1] and usable(WRAP, K)[0]
    if name != "no_wrap":
        assert caught["both_ends"], caught
    assert _longest_run(~usable(BOTH_ENDS, K)) == 4 and not usable(BOTH_ENDS, K)[[0, -1]].any()


# ---- commit
FIRST, COUNT, M = 3, 6, 12
STAGED_N = [4, 1, 2, -8, 5, 0]                         # staged rows 0, 2, 4 usable
IN_USE = [0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1]         # bank rows 3, 4, 7, 8 of the slice 3..8 are flown (and 1, 11 outside it)
#   bank row     3        4        5      6        7        8
#   staged       usable   no plan  usable no plan  usable   no plan
#   flown        yes      yes      no     no       yes      yes
#   plain        in use   in use   TAKEN  no plan  in use   in use       -> (1, 4, 1)
#   force        TAKEN    no plan  TAKEN  no plan  TAKEN    no plan      -> (3, 0, 3)


def _commit_inputs():
    return _bank([3, 2, 5, 4, 2, 3, 5, 2, 4, 3, 2, 5]), _bank(STAGED_N, tag=5000.0), np.array(IN_USE, bool)


def test_commit_by_hand():
    bank, staged, held = _commit_inputs()
    new, counts = commit(bank, staged, FIRST, held, K, False)
    assert counts == (1, 4, 1)
    want = [np.array(x) for x in bank]
    for x, s in zip(want, staged):
        x[5] = s[2]
    assert same_bank(new, want) and same_bank(bank, _commit_inputs()[0])       # the inputs are left alone
    new, counts = commit(bank, staged, FIRST, held, K, True)
    assert counts == (3, 0, 3)
    for x, s in zip(want, staged):
        x[3], x[7] = s[0], s[4]
    assert same_bank(new, want)
    # a one-row slice at the bank's last row
    new, counts = commit(bank, tuple(x[:1] for x in staged), M - 1, held, K, False)
    assert counts == (0, 1, 0) and same_bank(new, bank)
    new, counts = commit(bank, tuple(x[:1] for x in staged), M - 1, held, K, True)
    assert counts == (1, 0, 0) and np.array_equal(new[0][M - 1], staged[0][0]) and same_bank([x[:M - 1] for x in new], [x[:M - 1] for x in bank])


def _commit_mutant(kind):
    def f(bank, staged, first, in_use, K, force):
        sg, sub, ns = (np.array(x) for x in bank)
        count = len(staged[2])
        rows = (0 if kind == "first_dropped" else first) + np.arange(count)
        held = np.asarray(in_use, bool)[first + np.arange(count)]
        if kind == "ignores_in_use" or (force and kind != "in_use_under_force"):
            held = np.zeros(count, bool)
        ok = np.ones(count, bool) if kind == "takes_unusable" else usable(staged[2], K)
        take = ok & ~held
        for x, s in zip((sg, sub, ns), staged):
            x[rows[take]] = np.asarray(s)[take]
        no_plan = ~ok if kind == "precedence" else ~ok & ~held
        return (sg, sub, ns), (int(take.sum()), int((~take & ~no_plan).sum()), int(no_plan.sum()))
    return f


COMMIT_MUTANTS = ["ignores_in_use", "in_use_under_force", "takes_unusable", "first_dropped", "precedence"]


def test_the_commit_mutant_harness_is_the_model_when_nothing_is_mutated():
    bank, staged, held = _commit_inputs()
    for force in (False, True):
        want, got = commit(bank, staged, FIRST, held, K, force), _commit_mutant("none")(bank, staged, FIRST, held, K, force)
        assert same_bank(want[0], got[0]) and want[1] == got[1]


@pytest.mark.parametrize("kind", COMMIT_MUTANTS)
def test_the_comparison_rejects_every_wrong_commit(kind):
    bank, staged, held = _commit_inputs()
    caught = {}
    for force in (False, True):
        want, got = commit(bank, staged, FIRST, held, K, force), _commit_mutant(kind)(bank, staged, FIRST, held, K, force)
        caught[force] = (not same_bank(want[0], got[0]), want[1] != got[1])
    where = {"ignores_in_use": False, "in_use_under_force": True, "takes_unusable": False, "first_dropped": False, "precedence": False}[kind]
    assert any(caught[where]), caught
    if kind == "precedence":                     # the bank is the same: only the counters tell
        assert caught[False] == (False, True)
    else:                                        # the bank alone tells, without the counters
        assert caught[where][0], caught
    if kind in ("takes_unusable", "first_dropped"):
        assert caught[True][0], caught


# ---- which rows are flown
def test_flown_rows_follow_the_reset_draws():
    N, seed, m = 130, (0x5EED << 32) | 11, 96
    everyone = np.ones(N, bool)
    assert (flown_rows(N, seed, [], m) == -1).all()
    rows = flown_rows(N, seed, [(0, everyone)], m)
    assert np.array_equal(rows, px.reset_draws(N, seed, 0, m)[0])
    held = in_use_mask(rows, m)
    assert held.sum() == 71 and (~held).sum() == 25                          # what tests/test_bank_lifecycle_gpu.py builds on
    for lo, hi in ((5, 12), (91, 96)):
        assert held[lo:hi].any() and not held[lo:hi].all()
    some = np.arange(N) % 3 == 0
    later = flown_rows(N, seed, [(0, everyone), (4, np.zeros(N, bool)), (7, some)], m)
    assert np.array_equal(later[~some], rows[~some]) and np.array_equal(later[some], px.reset_draws(N, seed, 7, m)[0][some])
    assert not np.array_equal(later[some], rows[some])
    # a re-draw from a bank of another size
    small = flown_rows(N, seed, [(0, everyone), (7, some, 3)], m)
    assert np.array_equal(small[some], px.reset_draws(N, seed, 7, 3)[0][some]) and small[some].max() == 2
    assert in_use_mask([-1, 2, 2, 97], 4).tolist() == [False, False, True, False]
