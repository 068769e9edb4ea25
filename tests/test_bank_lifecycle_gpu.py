"""The reset bank's life on the device against oracle/bank_model.py, bit for bit (everything here is row movement):
  A  k_bank_fix / k_bank_fix2 behind uavenv_plan_scenarios: the bank is fix_up(the planner's raw rows);
  B  k_privatize: replacing the bank under flying agents (load / plan / a refused plan) changes nothing they fly, and the
     next resets draw from the bank that is then in place;
  C  k_bank_mark / k_bank_commit: a rolling refresh leaves commit(bank, staged slice, rows in use) and its three counters;
  D  the host state of uavenv_replan_begin / _ready / _commit: dropped slices, the reallocation, two refreshes back to back.
tests/test_bank_model.py shows on the host that these comparisons tell the model from each plausible wrong kernel."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from dqn_based_uav_3d_path_planer_amd._lib import UavEnvError
from dqn_based_uav_3d_path_planer_amd.data import load_city26, make_city26_env
from oracle import philox as px
from oracle.bank_model import commit, fix_up, flown_rows, in_use_mask, same_bank, usable
from test_random_streams_gpu import _bank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 130                              # the last wavefront is ragged

# Rows fail for both of the planner's reasons at K = 21 slots and 120 iterations (the reference's paths need 19 to 34 nodes, four
# attempts each).  Measured on the MI355X over the m = 64 (seeds 0..7) and m = 257 (seeds 0..3) cases below: 0.553 of the raw rows
# unusable (0.341 need more than K slots, 0.212 gave up), per case 0.42 .. 0.67.  Neighbours: K = 20 -> 0.82, K = 22 -> 0.32,
# K = 21 with 10 000 iterations -> 0.53 (no row gives up), with 80 -> 0.61.
K_FAIL, X_FAIL = 21, 120
FIX_CASES = [(2, s) for s in range(16)] + [(7, s) for s in range(16)] + [(64, s) for s in range(8)] + [(257, s) for s in range(4)]


def _np(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def _raw(env, m, seed, max_iter):
    return _np(*env.rrt_plan(m, seed=seed, max_iter=max_iter)[:3])


def _tick(env):
    return int(env.lib.uavenv_tick(env._h))


def _actions(steps, n, seed):
    a = np.random.default_rng(seed).integers(0, 3, (steps, n)).astype(np.int32)
    return torch.from_numpy(a).to(DEV)


def _redrawn(out, U):
    """The agents an auto-reset step re-drew: those of the envs whose U agents are all done."""
    done = out.agent_done.cpu().numpy().astype(bool).reshape(-1, U)
    return np.repeat(done.all(axis=1), U)


def _expire(env, first, count):
    """One step from the time limit: these agents finish in the next step (their list turns private until they are re-drawn)."""
    st, sub, alias = env.get_state(first, count, want_sub=True)
    step = np.full(count, int(load_city26()["max_step"]) - 1, np.int32)
    env.set_state(first, np.c_[st[:, 0:5], st[:, 6:9]], step, st[:, 11].astype(np.int32), sub, alias=alias)


def _fly(env, acts, *, expire=None, resets=None):
    """auto-reset steps; expire = {step index: [(first, count), ...]}; resets collects (tick, re-drawn mask) for flown_rows."""
    out = env.alloc_out()
    for t in range(len(acts)):
        for first, count in (expire or {}).get(t, ()):
            _expire(env, first, count)
        tick = _tick(env)
        env.step(acts[t], out, auto_reset=True)
        who = _redrawn(out, env.uav_per_env)
        for first, count in (expire or {}).get(t, ()):
            assert who[first:first + count].all(), (t, first, count)
        if resets is not None:
            resets.append((tick, who))
    return out


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _assert_in_step(a, b, acts):
    """a and b, driven by the same actions without auto-reset, give the same outputs and hold the same state at every step."""
    oa, ob = a.alloc_out(), b.alloc_out()
    for t in range(len(acts)):
        a.step(acts[t], oa)
        b.step(acts[t], ob)
        for f in ("obs", "reward", "ret_done", "agent_done", "info"):
            assert torch.equal(getattr(oa, f), getattr(ob, f)), (t, f)
        assert _same_state(a.get_state(want_sub=True), b.get_state(want_sub=True)), t


LATE = [(8, 64), (126, 4)]           # a whole wavefront's worth across two of them, and the ragged tail


def _assert_returns(env, seed, m, twin=None):
    """Expire LATE, take one auto-reset step: every agent that finished holds row reset_draws(N, seed, tick, m) of the bank the
    env has NOW -- position, goal, the whole list, n_sub, the alias -- and nobody else moved bank."""
    bank = env.bank_read()
    assert len(bank[2]) == m
    for e in (env, twin) if twin is not None else (env,):
        for first, count in LATE:
            _expire(e, first, count)
    before = env.get_state()
    tick = _tick(env)
    act = torch.ones(env.N, dtype=torch.int32, device=DEV)
    out = env.step(act, env.alloc_out(), auto_reset=True)
    who = _redrawn(out, env.uav_per_env)
    for first, count in LATE:
        assert who[first:first + count].all()
    rows = px.reset_draws(env.N, seed, tick, m)[0]
    st, sub, alias = env.get_state(want_sub=True)
    r = rows[who]
    assert m == 1 or len(np.unique(r)) > 1
    assert np.array_equal(st[who, 0:3], bank[0][r, :3]) and np.array_equal(st[who, 6:9], bank[0][r, 3:])
    assert np.array_equal(st[who, 11], bank[2][r]) and np.array_equal(sub[who], bank[1][r])
    assert (alias[who] == 1).all() and (st[who, 9] == 0).all() and (st[who, 10] == 0).all()
    assert np.array_equal(st[~who, 6:9], before[~who, 6:9])
    if twin is not None:
        ot = twin.step(act, twin.alloc_out(), auto_reset=True)
        assert torch.equal(out.obs, ot.obs) and torch.equal(out.reward, ot.reward) and torch.equal(out.agent_done, ot.agent_done)
        assert _same_state((st, sub, alias), twin.get_state(want_sub=True))


# ------------------------------------------------------------------------------------------------ A  fix-up
@pytest.fixture(scope="module")
def fail_env():
    e = make_city26_env(4, bank="gpu", bank_size=64, bank_seed=1, max_subgoals=K_FAIL)
    yield e
    e.close()


@pytest.fixture(scope="module")
def raws(fail_env):
    """The planner's own rows of every case, planned once."""
    return {(m, s): _raw(fail_env, m, s, X_FAIL) for m, s in FIX_CASES}


def _longest_run(bad):
    if bad.all():
        return len(bad)
    two, best, run = np.r_[bad, bad], 0, 0
    for b in two:
        run = run + 1 if b else 0
        best = max(best, run)
    return best


def test_the_fix_up_cases_cover_what_they_are_there_for(raws):
    bad = {k: ~usable(v[2], K_FAIL) for k, v in raws.items()}
    big = np.concatenate([b for (m, s), b in bad.items() if m >= 64])
    print("unusable share over m = 64, 257: %.3f" % big.mean(), {k: round(float(b.mean()), 2) for k, b in bad.items() if k[0] >= 64})
    assert 0.25 <= big.mean() <= 0.75
    assert any(b[-1] and not b[0] for b in bad.values())                               # the wrap at m - 1
    assert any(b[-1] and b[0] and not b.all() for b in bad.values())                   # a run across the wrap
    assert any(_longest_run(b) >= 3 and not b.all() for b in bad.values())
    assert any(_longest_run(b) >= 3 and not b.all() for (m, s), b in bad.items() if m == 257)
    assert any(m == 2 and b.sum() == 1 for (m, s), b in bad.items())
    assert any(b.all() for b in bad.values())                                          # ... and a bank nobody could plan
    for m in (64, 257):                                                                # both reasons to fail
        ns = np.concatenate([v[2] for (mm, s), v in raws.items() if mm == m])
        assert (ns < 0).any() and (ns == 1).any() and usable(ns, K_FAIL).any()


@pytest.mark.parametrize("m,seed", FIX_CASES)
def test_plan_scenarios_leaves_the_models_fix_up(fail_env, raws, m, seed):
    env, raw = fail_env, raws[(m, seed)]
    before, stats = env.bank_read(), env.bank_stats()
    good = usable(raw[2], K_FAIL)
    sg, sub, ns, replaced = fix_up(*raw, K_FAIL)
    assert replaced == int((~good).sum())
    if not good.any():
        with pytest.raises(UavEnvError, match="none of the"):
            env.plan_scenarios(m, seed=seed, max_iter=X_FAIL)
        assert env.bank_stats() == stats and same_bank(env.bank_read(), before)
        return
    env.plan_scenarios(m, seed=seed, max_iter=X_FAIL)
    got = env.bank_read()
    assert env.bank_stats() == (m, replaced)
    assert same_bank(got, (sg, sub, ns))
    # the same, spelt out: usable rows are the planner's (all K x 3 doubles), a patched row is its source row as the bank holds it
    assert all(np.array_equal(g[good], r[good]) for g, r in zip(got, raw))
    for i in np.nonzero(~good)[0]:
        j = next((i + d) % m for d in range(1, m) if good[(i + d) % m])
        assert all(np.array_equal(g[i], g[j]) for g in got), (i, j)


# ------------------------------------------------------------------------------------------------ B  k_privatize
SEED_B = (0x5EED << 32) | 22      # no agent of the tests below draws one of the rows 0..2 of the packaged bank
EXPIRE_B = {5: [(0, 40)], 14: [(60, 70)], 29: [(100, 20)]}       # the last group is re-drawn by the last step: it keeps the alias


def _packaged(K):
    c = load_city26()
    sub = np.zeros((len(c["n_sub"]), K, 3))
    sub[:, :min(K, c["sub_goals"].shape[1])] = c["sub_goals"][:, :K]
    return c["start_goal"], sub, c["n_sub"]


def _flown_env():
    env = make_city26_env(N)
    env.reset(seed=SEED_B)
    resets = [(0, np.ones(N, bool))]
    _fly(env, _actions(30, N, 1), expire=EXPIRE_B, resets=resets)
    return env, resets


def _padded(bank, K):
    sg, sub, ns = bank
    out = np.zeros((len(ns), K, 3))
    out[:, :sub.shape[1]] = sub
    return sg, out, ns


@pytest.mark.parametrize("how", ["load3", "plan64", "refused"])
def test_replacing_the_bank_under_flying_agents(how):
    env, resets = _flown_env()
    twin, _ = _flown_env()
    old = _packaged(env.K)
    assert same_bank(env.bank_read(), old)
    rows = flown_rows(N, SEED_B, resets, 1024)
    snap = env.get_state(want_sub=True)
    st, sub, alias = snap
    assert _same_state(snap, twin.get_state(want_sub=True))
    assert len(resets) == 31 and (rows >= 0).all()
    n_rem = st[:, 11].astype(int)
    popped = n_rem < old[2][rows]
    assert popped.sum() >= 50 and ((alias == 1) & ~popped).sum() >= 20 and not (alias[popped] == 1).any()
    for i in range(N):                    # what they fly IS their bank row's remainder (behind the current sub-goal, which the agent owns)
        at = old[2][rows[i]] - n_rem[i]
        assert np.array_equal(sub[i, 1:n_rem[i]], old[1][rows[i], at + 1:old[2][rows[i]]]) and np.array_equal(st[i, 6:9], old[0][rows[i], 3:])
    if how == "load3":
        env.load_scenarios(*_bank(3))     # smaller than any id in use
        m_new = 3
        assert rows.min() >= 3 and same_bank(env.bank_read(), _padded(_bank(3), env.K)) and env.bank_stats() == (3, 0)
    elif how == "plan64":
        env.plan_scenarios(64, seed=9)
        m_new = 64
        assert env.bank_stats()[0] == 64 and not np.array_equal(env.bank_read()[0], old[0][:64])
    else:
        with pytest.raises(UavEnvError, match="none of the"):
            env.plan_scenarios(64, seed=3, max_iter=1)
        m_new = 1024
        assert env.bank_stats() == (1024, 0) and same_bank(env.bank_read(), old)
    assert _same_state(env.get_state(want_sub=True), snap)
    _assert_in_step(env, twin, _actions(40, N, 2))
    _assert_returns(env, SEED_B, m_new, twin=twin if how == "refused" else None)
    env.close()
    twin.close()


def test_replacing_the_bank_under_apf_agents_changes_nothing():
    """APF agents fly private lists from the reset on: the swap has nothing to detach."""
    vel = load_golden("apf_episodes.npz")["velocities"]
    envs = []
    for _ in range(2):
        e = make_city26_env(N, apf_enabled=1)
        e.set_buildings(e.buildings, velocities=vel)
        e.reset(seed=SEED_B)
        _fly(e, _actions(30, N, 1))
        envs.append(e)
    env, twin = envs
    snap = env.get_state(want_sub=True)
    assert _same_state(snap, twin.get_state(want_sub=True)) and (snap[0][:, 11] >= 1).all()
    env.load_scenarios(*_bank(3))
    assert _same_state(env.get_state(want_sub=True), snap)
    _assert_in_step(env, twin, _actions(40, N, 2))
    env.close()
    twin.close()


def test_replacing_the_bank_under_four_uavs_per_env():
    env, twin = (make_city26_env(33, uav_per_env=4) for _ in range(2))          # 132 agents
    for e in (env, twin):
        e.reset(seed=SEED_B)
    snap = env.get_state(want_sub=True)
    rows = flown_rows(env.N, SEED_B, [(0, np.ones(env.N, bool))], 1024)
    old = _packaged(env.K)
    assert np.array_equal(snap[1], old[1][rows]) and (snap[2] == 1).all() and rows.min() >= 3
    env.load_scenarios(*_bank(3))
    assert _same_state(env.get_state(want_sub=True), snap)
    _assert_in_step(env, twin, _actions(40, env.N, 2))
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ C  rolling commit
SEED_C = (0x5EED << 32) | 11         # the CPU oracle puts 130 agents on 71 of 96 rows; rows 5..11 and 91..95 are mixed
M_C = 96
EXPIRE_C = {4: [(0, 40)], 12: [(64, 66)]}
STAT_KEYS = ("rows_committed", "rows_in_use", "rows_without_plan")
# (first, count, seed of the refresh, does the staged slice hold both kinds of row); the one-row slice comes with either kind
SLICES = [(0, 96, 77, True), (5, 7, 77, True), (91, 5, 1002, True), (40, 1, 77, False), (40, 1, 78, False)]


def _rolling_env(n_envs=N, U=1, fly=True):
    env = make_city26_env(n_envs, bank="gpu", bank_size=M_C, bank_seed=7, max_subgoals=K_FAIL, uav_per_env=U)
    env.reset(seed=SEED_C)
    resets = [(0, np.ones(env.N, bool))]
    held0 = in_use_mask(flown_rows(env.N, SEED_C, resets, M_C), M_C)
    assert held0.sum() >= 10 and (~held0).sum() >= 10
    if fly:
        _fly(env, _actions(20, env.N, 3), expire=EXPIRE_C, resets=resets)
    rows = flown_rows(env.N, SEED_C, resets, M_C)
    held = in_use_mask(rows, M_C)
    assert held.sum() >= 10 and (~held).sum() >= 10 and (rows >= 0).all()
    return env, held, resets


def _refresh(env, first, count, seed, held, force, stream=None, check_ready=True):
    """begin -> (ready) -> commit of one slice; -> (the model's bank, the model's counters)."""
    staged = tuple(x[first:first + count] for x in _raw(env, M_C, seed, X_FAIL))
    before = env.bank_read()
    env.replan_begin(first, count, seed=seed, max_iter=X_FAIL, stream=stream)
    if check_ready:
        torch.cuda.synchronize()
        assert env.replan_ready() == 1
    env.replan_commit(force)
    return staged, commit(before, staged, first, held, K_FAIL, force)


def _delta(after, before):
    return tuple(after[k] - before[k] for k in STAT_KEYS)


@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("first,count,seed,mixed", SLICES)
def test_a_refresh_commits_what_the_model_commits(first, count, seed, mixed, force):
    env, held, resets = _rolling_env()
    assert len(resets) == 21
    s0 = env.replan_stats()
    staged, (want, counts) = _refresh(env, first, count, seed, held, force)
    ok = usable(staged[2], K_FAIL)
    if mixed:
        assert ok.any() and not ok.all()
    else:
        assert ok[0] == (seed == 78)
    if count == M_C:                     # every combination of flown / free and plan / no plan, so every branch of the commit
        assert all((held == h)[ok == u].any() for h in (False, True) for u in (False, True))
    got, s1 = env.bank_read(), env.replan_stats()
    assert same_bank(got, want)
    assert _delta(s1, s0) == counts and sum(counts) == count
    assert s1["refreshes"] == s0["refreshes"] + 1 and s1["rows_planned"] == s0["rows_planned"] + count
    assert env.replan_ready() == -1
    env.close()


def test_agents_fly_on_undisturbed_by_a_refresh_and_come_back_on_the_new_rows():
    env, held, _ = _rolling_env()
    twin, held_t, _ = _rolling_env()
    assert np.array_equal(held, held_t)
    old = env.bank_read()
    _, (want, counts) = _refresh(env, 0, M_C, 77, held, False)
    assert same_bank(env.bank_read(), want) and counts[0] >= 1 and not same_bank(want, old) and same_bank(twin.bank_read(), old)
    _assert_in_step(env, twin, _actions(40, N, 4))
    _assert_returns(env, SEED_C, M_C)
    env.close()
    twin.close()


def test_a_refresh_with_four_uavs_per_env():
    env, held, _ = _rolling_env(n_envs=40, U=4, fly=False)                     # 160 agents, committed right after the reset
    s0 = env.replan_stats()
    _, (want, counts) = _refresh(env, 0, M_C, 77, held, False)
    assert same_bank(env.bank_read(), want) and _delta(env.replan_stats(), s0) == counts and min(counts) >= 1
    env.close()


# ------------------------------------------------------------------------------------------------ D  the state machine
def test_a_slice_planned_for_another_world_or_bank_is_dropped():
    env, held, _ = _rolling_env(fly=False)
    with pytest.raises(UavEnvError, match="nothing planned"):
        env.replan_commit()
    # the world changed (to the same buildings) between begin and commit
    bank, s0 = env.bank_read(), env.replan_stats()
    env.replan_begin(0, M_C, seed=77, max_iter=X_FAIL)
    torch.cuda.synchronize()
    assert env.replan_ready() == 1
    env.set_buildings(env.buildings)
    env.replan_commit()
    s1 = env.replan_stats()
    assert same_bank(env.bank_read(), bank) and _delta(s1, s0) == (0, 0, 0) and env.replan_ready() == -1
    assert (s1["refreshes"], s1["rows_planned"]) == (1, M_C)
    with pytest.raises(UavEnvError, match="nothing planned"):
        env.replan_commit()
    # the machine goes on: the next refresh is the model's
    _, (want, counts) = _refresh(env, 5, 7, 77, held, False)
    assert same_bank(env.bank_read(), want) and _delta(env.replan_stats(), s1) == counts
    # the bank was replaced by one shorter than first + count
    s2 = env.replan_stats()
    env.replan_begin(90, 6, seed=78, max_iter=X_FAIL)
    torch.cuda.synchronize()
    env.load_scenarios(*_bank(3))
    short = env.bank_read()
    assert same_bank(short, _padded(_bank(3), env.K))
    env.replan_commit()
    assert same_bank(env.bank_read(), short) and _delta(env.replan_stats(), s2) == (0, 0, 0) and env.replan_ready() == -1
    with pytest.raises(UavEnvError):
        env.replan_begin(2, 2, seed=1, max_iter=X_FAIL)                       # rows [2, 4) of a bank of 3
    env.close()


def test_a_larger_slice_reallocates_the_staging_area_and_stays_exact():
    env, held, _ = _rolling_env(fly=False)
    s0 = env.replan_stats()
    _, (want, c1) = _refresh(env, 40, 1, 78, held, False)
    assert same_bank(env.bank_read(), want) and c1 == (1, 0, 0) and not held[40]
    _, (want, c2) = _refresh(env, 0, M_C, 77, held, False)                    # 96 rows after 1: the staging area grows
    assert same_bank(env.bank_read(), want) and _delta(env.replan_stats(), s0) == tuple(a + b for a, b in zip(c1, c2))
    _, (want, c3) = _refresh(env, 91, 5, 1002, held, True)                     # ... and a smaller one in the grown area, forced
    assert same_bank(env.bank_read(), want) and c3[1] == 0 and c3[0] >= 1 and c3[2] >= 1
    env.close()


def test_two_refreshes_back_to_back_without_a_host_synchronise():
    """begin -> commit -> begin -> commit, the planner on a stream of its own: the second planner launch writes the staging area
    the first commit reads, so it has to wait for that commit on the device (rp_committed)."""
    env, held, _ = _rolling_env(fly=False)
    side = torch.cuda.Stream()
    raw_a, raw_b = _raw(env, M_C, 77, X_FAIL), _raw(env, M_C, 1002, X_FAIL)
    bank, s0 = env.bank_read(), env.replan_stats()
    torch.cuda.synchronize()
    env.replan_begin(0, M_C, seed=77, max_iter=X_FAIL, stream=side)
    env.replan_commit()
    env.replan_begin(5, 7, seed=1002, max_iter=X_FAIL, stream=side)          # fits the staging area: no reallocation, no wait
    env.replan_commit()
    one, c1 = commit(bank, raw_a, 0, held, K_FAIL, False)
    two, c2 = commit(one, tuple(x[5:12] for x in raw_b), 5, held, K_FAIL, False)
    assert c2[0] >= 1 and not same_bank(one, two)                              # the second commit moves rows the first one wrote
    assert same_bank(env.bank_read(), two)
    assert _delta(env.replan_stats(), s0) == tuple(a + b for a, b in zip(c1, c2))
    env.close()
