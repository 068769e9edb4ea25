"""oracle/team_model.py on the host, and the scripted scenario of tests/test_team_protocol_gpu.py before any device is involved:
  * the model equals a slow restatement of Envs/PathPlan_City.py:252-259, 365-366, 416-417 (one loop per env and per agent);
  * UAV j's Calc_Fly_Power equals the C oracle's with A_j, xi_j set per agent;
  * the script (tests/team_protocol.py) meets its coverage conditions on the C oracle alone, for every U and form used;
  * the per-launch assertions (team_protocol.check_launch) reject each plausible wrong team protocol, with the device-free
    HostEnv standing in for the device."""
import ctypes as C

import numpy as np
import pytest

import team_protocol as tp
from oracle import pyoracle as po
from oracle import team_model as tm

ALL_U = tm.TEAM_SIZES
# (form, the U that run through it on the device, variant); tests/test_team_protocol_gpu.py takes its cases from here
FORMS = [("coop", ALL_U, 0), ("one_wave", ALL_U, 1), ("apf_split", (8, 16, 64), 0), ("apf_lane", (2, 4, 32), 1),
         ("f16", (1, 8, 32), 0), ("packed", (2, 4, 64), 1), ("noskip", (2, 16, 64), 0), ("active", (4, 8, 32), 0),
         ("active", (4, 8, 32), 1)]
SCRIPT_FORM = {"noskip": "noskip", "active": "active"}          # every other form runs the plain script


def _apf_velocities():
    from dqn_based_uav_3d_path_planer_amd.data import load_city26
    v = np.random.default_rng(42).uniform(-1.0, 1.0, (len(load_city26()["buildings"]), 3))
    v[:, 2] = 0.0
    return v


def make_ctx(U, form):
    apf = form.startswith("apf")
    return tp.Ctx(U, apf=apf, velocities=_apf_velocities() if apf else None)


# ------------------------------------------------------------------------------------------------ the model
def _slow_launch(U, flags, done, done_after, active):
    """Written from the reference lines, one loop per env and per agent."""
    n = len(done)
    steps, agent_done = [False] * n, [False] * n
    for i in range(n):
        masked = active is not None and active[i] == 0
        waits = bool(flags & tm.SKIP_DONE) and bool(done[i])          # run_thread: if uav.done: return
        steps[i] = not masked and not waits
        agent_done[i] = bool(done_after[i]) if steps[i] else bool(done[i])
    restart = []
    for e in range(n // U):
        all_done = True                                              # Check_uav_Done
        for j in range(U):
            if not agent_done[e * U + j]:
                all_done = False
        restart.append(all_done and bool(flags & tm.AUTO_RESET))
    return steps, agent_done, restart


@pytest.mark.parametrize("U", ALL_U)
def test_the_model_equals_the_slow_restatement(U):
    rng = np.random.default_rng(U)
    n = U * tp.N_ENVS[U]
    hits = 0
    for trial in range(60):
        p = rng.choice([0.1, 0.5, 0.9, 0.98])
        done = rng.random(n) < p
        done_after = done | (rng.random(n) < p)
        active = None if trial % 3 == 0 else (rng.random(n) < rng.choice([0.3, 0.9])).astype(np.uint8)
        if trial % 3 == 2:
            active = (np.arange(n) % U == rng.integers(U)).astype(np.uint8)
        for flags in (0, tm.AUTO_RESET, tm.SKIP_DONE, tm.AUTO_RESET | tm.SKIP_DONE):
            info = rng.integers(0, 3, n)
            m = tm.launch(U, flags, done, rng.random(n), done_after, info, done_after, active)
            steps, agent_done, restart = _slow_launch(U, flags, done, done_after, active)
            assert m["stepping"].tolist() == steps and (m["agent_done"] != 0).tolist() == agent_done
            assert m["restart_envs"].tolist() == restart and m["restarted"].tolist() == [restart[i // U] for i in range(n)]
            assert np.array_equal(m["valid"] != 0, m["stepping"]) and (m["info"][~m["stepping"]] == 3).all()
            assert np.array_equal(m["info"][m["stepping"]], info[m["stepping"]])
            assert np.array_equal(m["ret_done"][~m["stepping"]] != 0, done[~m["stepping"]])
            # the lane arithmetic of a wavefront, written out, is the same decision
            if flags & tm.AUTO_RESET:
                assert np.array_equal(tp.wave_restart(U, m["agent_done"] != 0, done, active), m["restarted"])
                hits += int(m["restart_envs"].sum())
    assert hits > 0


def test_the_mask_rules_by_hand():
    U, flags = 4, tm.AUTO_RESET | tm.SKIP_DONE
    done = np.array([1, 1, 0, 1,   1, 0, 0, 1,   1, 1, 1, 1], bool)
    after = np.array([1, 1, 1, 1,   1, 1, 0, 1,   1, 1, 1, 1], bool)
    active = (np.arange(12) % U == 2).astype(np.uint8)
    z = np.zeros(12)
    m = tm.launch(U, flags, done, z, z, z, after, active)
    assert m["stepping"].tolist() == [False, False, True, False, False, False, True, False, False, False, False, False]
    # env 0: three masked done members count; env 1: the masked live member 5 blocks; env 2: complete, everyone masked or waiting
    assert m["restart_envs"].tolist() == [True, False, True]
    assert m["valid"].tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0] and m["ret_done"][[0, 5, 8]].tolist() == [1, 0, 1]


def test_slot_power_against_the_c_oracle():
    from dqn_based_uav_3d_path_planer_amd.data import load_city26
    c = load_city26()
    ctx = tp.Ctx(64)
    b = ctx.batch(0, 128)
    V = np.linspace(0.0, 1.0, 128)
    b.view["vx"], b.view["vy"], b.view["vz"] = V, 0.0, 0.0
    got = tm.fly_power_many(c["power"], V, np.arange(128) % 64)
    ref = np.array([b.lib.orc_calc_fly_power(C.byref(b.arr[i])) for i in range(128)])
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.isclose(c["power"][8], 0.8) and tm.slot_power_params(c["power"], 0) == (c["power"][5], 0.8)
    at_full = tm.fly_power_many(c["power"], np.ones(64), np.arange(64))
    assert (np.diff(at_full) > 0).all()
    # j = i mod U, not i // U: the two differ at every U for some agent of the test shapes
    for U in ALL_U:
        i = np.arange(U * tp.N_ENVS[U])
        assert (tm.uav_slot(i, U) != i // U).any()


# ------------------------------------------------------------------------------------------------ the script on the C oracle
def _run(U, form, variant, mutation=None, checked=True):
    ctx = make_ctx(U, form)
    script = SCRIPT_FORM.get(form, "plain")
    env = tp.HostEnv(ctx, mutation)
    ms = []

    def check(rec, t):
        ms.append(tp.check_launch(ctx, rec, apf=form.startswith("apf")))
    recs = tp.run_script(env, U, variant, script, check if checked else None)
    return ctx, recs, ms


def _coverage(U, script, variant, recs):
    """Classes hit over the scripted launches; that nobody the script does not push finishes by itself."""
    every, ragged = set(), set()
    for t, rec in enumerate(recs[1:]):
        before = rec["pre"][0][:, 10] != 0
        after = rec["out"]["agent_done"] != 0
        pushed = rec["pre"][0][:, 9] == tp.load_city26()["max_step"] - 1
        flags, active = tp.launch_args(U, script, t)
        steps = tm.who_steps(flags, before, active)
        assert np.array_equal(after & ~before, pushed & steps & ~before), (U, script, t)
        e, r = tp.events(U, before, after)
        every |= e
        ragged |= r
    first = recs[0]
    assert not (first["out"]["agent_done"] != 0).any() and (first["post"][0][:, 9] == 0).all()   # the start node popped: Step 0
    return every, ragged


@pytest.mark.parametrize("form,us,variant", FORMS)
def test_the_script_meets_its_coverage_conditions_on_the_oracle_alone(form, us, variant):
    script = SCRIPT_FORM.get(form, "plain")
    for U in us:
        ctx, recs, ms = _run(U, form, variant)
        assert len(recs) == 1 + tp.LAUNCHES and ctx.N == U * tp.N_ENVS[U] and (ctx.N + 63) // 64 == 3
        every, ragged = _coverage(U, script, variant, recs)
        restarts = sum(int(m["restart_envs"].sum()) for m in ms[1:])
        assert restarts >= 2, (U, form)
        if script == "active":
            slot = tp.active_slot(U)
            # in a masked launch: a team completed by its active member, all others masked AND done, restarts ...
            m1, r1 = ms[1 + tp.MASKED[0]], recs[1 + tp.MASKED[0]]
            before = (r1["pre"][0][:, 10] != 0).reshape(-1, U)
            others = np.delete(np.arange(U), slot)
            counted = m1["restart_envs"] & before[:, others].all(axis=1) & ~before[:, slot]
            # ... a team whose active member finishes while a masked member still flies does not ...
            fin = (m1["agent_done"] != 0).reshape(-1, U)
            blocked = ~m1["restart_envs"] & fin[:, slot] & ~before[:, slot] & ~fin[:, others].all(axis=1)
            assert counted.sum() >= 2 and blocked.sum() >= 2, (U, counted.sum(), blocked.sum())
            rag = tp.ragged_envs(U)
            assert counted[rag].any() if variant == 0 else blocked[rag].any()
            # ... and in the second masked launch a done active member waits, a restarted team's masked members stay put
            m2, r2 = ms[1 + tp.MASKED[1]], recs[1 + tp.MASKED[1]]
            d2 = (r2["pre"][0][:, 10] != 0).reshape(-1, U)
            assert d2[:, slot].any() and not m2["stepping"].reshape(-1, U)[d2[:, slot], slot].any()
            assert not m2["restart_envs"].any() and ms[1 + 3]["restart_envs"].any()          # completed later, without the mask
            continue
        assert every >= tp.possible_classes(U), (U, form, tp.possible_classes(U) - every)
        if script == "noskip":              # done agents step on: some agent that was done before the launch steps in it
            assert any((m["stepping"] & (r["pre"][0][:, 10] != 0)).any() for m, r in zip(ms[1:], recs[1:]))
        if tp.ragged_envs(U):
            other = _coverage(U, script, 1 - variant, _run(U, form, 1 - variant, checked=False)[1])[1]
            assert ragged | other >= tp.possible_classes(U), (U, form, tp.possible_classes(U) - ragged - other)
            if U == 1:
                assert ragged >= tp.possible_classes(U)


def test_the_shapes_are_the_edges():
    for U in ALL_U:
        n = U * tp.N_ENVS[U]
        assert (n + 63) // 64 == 3
        assert (n % 64 != 0) == (U != 64)
    assert 32 * tp.N_ENVS[32] % 64 == 32                                   # one team in a half-empty wave
    assert len(tp.ragged_envs(32)) == 1 and tp.ragged_envs(64) == [] and len(tp.ragged_envs(1)) == 2
    for form, us, variant in FORMS[2:]:
        assert set(us) & {2, 8, 32, 64}
    for U in ALL_U:
        assert sum(U in us for _, us, _ in FORMS) >= 3


# ------------------------------------------------------------------------------------------------ mutations
def _same_as_model(mutation, U):
    """Where the mistake is no mistake: a team that is the whole wave, a team of one."""
    return (mutation in ("mask_not_shifted", "team_is_the_wave") and U == 64) or \
           (mutation in ("any_member_done", "waiting_redrawn_early") and U == 1)


@pytest.mark.parametrize("mutation", tp.MUTATIONS)
def test_the_assertions_reject_every_wrong_protocol(mutation):
    form = "active" if mutation == "masked_done_not_counted" else "coop"
    us = (4, 8, 32) if form == "active" else ALL_U
    for U in us:
        for variant in (0, 1):
            if _same_as_model(mutation, U):
                _run(U, form, variant, mutation)                            # passes: the same decision
                continue
            with pytest.raises(AssertionError):
                _run(U, form, variant, mutation)
    # the waiting agents of a team nobody completes are what "re-drawn early" and "one launch late" are told by
    if mutation == "waiting_redrawn_early":
        with pytest.raises(AssertionError, match="restart set"):
            _run(8, "coop", 0, mutation)


def test_the_harness_is_the_model_when_nothing_is_mutated():
    for U in ALL_U:
        ctx, recs, ms = _run(U, "coop", 0)
        assert all(m["stats"].get("reward", 0.0) == 0.0 for m in ms)
