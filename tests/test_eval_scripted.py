"""CPU checks of the scripted baseline (uavenv_scripted_act, uavenv_eval_episodes_scripted): the new ABI struct against the header
as gcc sees it, the argument refusals of evaluate_scripted_policy / scripted_act that need no device, hand cases of the independent
reference (tests/scripted_policy_ref.py), and the condition the GPU tests' fragile-decision caps rest on."""
import ctypes
import inspect
import math
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT
from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev
from dqn_based_uav_3d_path_planer_amd.data import load_city26
from oracle import pyoracle as po

import scripted_policy_ref as spr


def test_scripted_struct_layout_matches_the_header_as_gcc_sees_it(tmp_path):
    name, ct = "UavScriptedPolicy", _lib.UavScriptedPolicy
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "uavenv.h"', 'int main(void){']
    lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
    for fname, _ in ct._fields_:
        lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines.append('printf("kinds %d %d\\n", UAVENV_ACT_INDEX_I32, UAVENV_ACT_STEER_F32);')
    lines.append('printf("limits %d %d %d\\n", UAVENV_SCRIPTED_MAX_LOOKAHEAD, UAVENV_SCRIPTED_MAX_STEER_CANDIDATES, '
                 'UAVENV_SCRIPTED_MAX_INDEX_ACTIONS);')
    lines.append('printf("record %zu args %zu sacargs %zu\\n", sizeof(UavEvalRecord), sizeof(UavEvalArgs), sizeof(UavSacEvalArgs));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {l.split()[0]: l.split()[1:] for l in out}
    assert int(got[name][0]) == ctypes.sizeof(ct) == 16
    for fname, _ in ct._fields_:
        assert int(got[f"{name}.{fname}"][0]) == getattr(ct, fname).offset, fname
    assert [int(x) for x in got["kinds"]] == [_lib.ACT_INDEX_I32, _lib.ACT_STEER_F32]
    assert ev.SCRIPTED_KINDS == {"index": _lib.ACT_INDEX_I32, "steer": _lib.ACT_STEER_F32}
    assert [int(x) for x in got["limits"]] == [_lib.SCRIPTED_MAX_LOOKAHEAD, _lib.SCRIPTED_MAX_STEER_CANDIDATES,
                                               _lib.SCRIPTED_MAX_INDEX_ACTIONS] == [16, 17, 32]
    assert int(got["record"][0]) == 64 == _lib.EVAL_RECORD_BYTES                 # the record did not change
    assert int(got["record"][2]) == ctypes.sizeof(_lib.UavEvalArgs)              # nor did the argument structs
    assert int(got["record"][4]) == ctypes.sizeof(_lib.UavSacEvalArgs)


def test_the_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    for sym in ("uavenv_scripted_act", "uavenv_eval_episodes_scripted"):
        assert sym in _lib.SYMBOLS and f"int {sym}(" in hdr
    assert _lib.ABI_VERSION == 5 and "#define UAVENV_ABI_VERSION 5" in hdr       # additive: the version stays
    sig = inspect.signature(ev.evaluate_scripted_policy)
    assert list(sig.parameters) == ["env", "n_episodes", "action", "candidates", "lookahead", "scenarios", "first", "seed", "eps",
                                    "max_steps", "v0", "trajectory_steps", "max_workgroups"]
    assert sig.parameters["action"].kind is inspect.Parameter.KEYWORD_ONLY
    assert (sig.parameters["action"].default, sig.parameters["candidates"].default, sig.parameters["lookahead"].default) == \
        ("index", None, 8)
    sig = inspect.signature(ev.scripted_act)
    assert list(sig.parameters) == ["env", "actions_out", "action", "candidates", "lookahead"]


class _NoEnv:
    """Stands in for an env: its shape (K, uav_per_env, the configured action count) is all a check may look at; any other use
    fails, so a ValueError proves the check ran before anything was read from the device or enqueued."""
    K = 48
    uav_per_env = 4

    def __init__(self, n_actions=3):
        self.__dict__["cfg"] = types.SimpleNamespace(n_actions=n_actions)

    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the arguments were checked")


BAD_POLICY = [dict(action="both"), dict(action=None), dict(action=2), dict(action="index", candidates=3),
              dict(action="index", candidates=9), dict(action="steer", candidates=4), dict(action="steer", candidates=1),
              dict(action="steer", candidates=19), dict(action="steer", candidates=0), dict(action="steer", candidates=4.5),
              dict(lookahead=-1), dict(lookahead=17), dict(lookahead=2.5), dict(action="steer", lookahead=17)]


@pytest.mark.parametrize("kw", [dict(n_episodes=0), dict(n_episodes=-3), dict(n_episodes=2.5), dict(first=-1),
                                dict(max_steps=-1), dict(trajectory_steps=-2), dict(max_workgroups=-1),
                                dict(eps=-0.1), dict(eps=1.5), dict(eps=float("nan")),
                                dict(action="steer", eps=0.5), dict(action="steer", candidates=9, eps=1.0),
                                dict(scenarios=(np.zeros((4, 6)), np.zeros((4, 7, 3)), np.zeros(4))),
                                dict(scenarios=(np.zeros((0, 6)), np.zeros((0, 48, 3)), np.zeros(0))),
                                dict(scenarios=(np.zeros((4, 6)), np.zeros((4, 48, 3)))),
                                dict(v0=np.zeros((63, 2))), dict(v0=np.zeros((64, 3))), dict(v0=np.zeros(128))] + BAD_POLICY)
def test_bad_arguments_raise_value_error_without_a_device(kw):
    args = dict(n_episodes=64)
    args.update(kw)
    n = args.pop("n_episodes")
    with pytest.raises(ValueError):
        ev.evaluate_scripted_policy(_NoEnv(), n, **args)


@pytest.mark.parametrize("n_actions", [0, 1, 33, 100])
def test_the_index_kind_refuses_an_env_with_too_many_or_too_few_actions(n_actions):
    with pytest.raises(ValueError):
        ev.evaluate_scripted_policy(_NoEnv(n_actions), 64, action="index")
    with pytest.raises(ValueError):
        ev.scripted_act(_NoEnv(n_actions), None, action="index")


@pytest.mark.parametrize("kw", BAD_POLICY)
def test_scripted_act_refuses_a_bad_policy_without_a_device(kw):
    with pytest.raises(ValueError):
        ev.scripted_act(_NoEnv(), None, **kw)


@pytest.mark.parametrize("action", ["index", "steer"])
def test_scripted_act_refuses_a_bad_output_tensor_before_the_env_is_touched(action):
    import torch
    wrong = torch.zeros(8, dtype=torch.float32 if action == "index" else torch.int32)
    for out in (None, np.zeros(8, np.int32), wrong):
        with pytest.raises(ValueError):
            ev.scripted_act(_NoEnv(), out, action=action)


def test_plugin_evaluate_baseline_needs_the_gpu_backend():
    from dqn_based_uav_3d_path_planer_amd.plugins.PathPlan_City import PathPlan_City
    sig = inspect.signature(PathPlan_City.evaluate_baseline)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("n_episodes", 1024), ("seed", 0), ("held_out", True),
                                                                        ("max_steps", 0), ("lookahead", 8), ("candidates", 9)]
    assert list(inspect.signature(PathPlan_City.evaluate_policy).parameters) == ["self", "n_episodes", "seed", "held_out", "max_steps",
                                                                                  "mode"]
    with pytest.raises(RuntimeError, match="GPU backend"):
        PathPlan_City.evaluate_baseline(types.SimpleNamespace(backend=object()))       # (a backend without the planner: the CPU fake)


# ---- hand cases of the reference ------------------------------------------------------------------------------------------------
STEERING = 30.0 / 180.0 * math.pi


def _policy(kind, C, H, buildings=((1000.0, 1000.0, 0.0, 1.0, 10.0),)):
    """An open 500 x 500 x 100 box; the default cylinder stands outside it."""
    b = np.asarray(buildings, np.float64).reshape(-1, 5)
    world = po.OracleWorld(b, 500.0, 500.0, 100.0)
    return spr.Policy(world, b, 500.0, 1.0, STEERING, kind, C, H), world


def _uav(world, pos, heading, sub_goals):
    u = po.OracleUav(world, dict(max_v=1.0, steering_angle=STEERING, max_step=150, apf_enabled=0))
    u.set_state(pos[0], pos[1], pos[2], math.cos(heading), math.sin(heading), 400.0, 400.0, 50.0, 0, sub_goals)
    return u


@pytest.mark.parametrize("kind,C", [("index", 3), ("index", 9), ("steer", 9), ("steer", 17)])
def test_sub_goal_dead_ahead_takes_the_middle_candidate(kind, C):
    pol, world = _policy(kind, C, 4)
    d = pol.decide_uav(_uav(world, (250, 250, 50), 0.0, [[300, 250, 50]]))
    assert d.k[0] == C // 2 and d.steer[0] == 0.0 and not d.fragile[0]


@pytest.mark.parametrize("kind,C", [("index", 3), ("steer", 9)])
def test_sub_goal_at_plus_90_degrees_clamps_to_the_last_candidate(kind, C):
    pol, world = _policy(kind, C, 4)
    d = pol.decide_uav(_uav(world, (250, 250, 50), 0.0, [[250, 300, 50]]))
    assert d.k[0] == C - 1 and d.steer[0] == 1.0
    d = pol.decide_uav(_uav(world, (250, 250, 50), 0.0, [[250, 200, 50]]))       # and at -90 degrees to the first
    assert d.k[0] == 0 and d.steer[0] == -1.0


def test_the_heading_error_wraps():
    """heading 6.2, bearing 0.1: err = 0.1 - 6.2 + 2 pi = 0.183 rad -> s* = 0.35: the nearest of 9 steers is +0.25 (k = 5), and of
    the three index steers 0 (k = 1); without the wrap s* would clamp to -1."""
    pol, world = _policy("steer", 9, 0)
    u = _uav(world, (250, 250, 50), 6.2, [[250 + 100 * math.cos(0.1), 250 + 100 * math.sin(0.1), 50]])
    d = pol.decide_uav(u)
    assert d.k[0] == 5 and d.steer[0] == 0.25
    pol3, _ = _policy("index", 3, 0)
    assert pol3.decide_uav(u).k[0] == 1
    # the other side: heading 0.1, bearing 6.2 -> a small negative steer
    u = _uav(world, (250, 250, 50), 0.1, [[250 + 100 * math.cos(6.2), 250 + 100 * math.sin(6.2), 50]])
    assert pol.decide_uav(u).steer[0] == -0.25


def test_equal_costs_take_the_lower_candidate():
    pol, world = _policy("index", 2, 4)
    d = pol.decide_uav(_uav(world, (250, 250, 50), 0.0, [[300, 250, 50]]))       # s* = 0: |-1 - 0| = |1 - 0|
    assert d.k[0] == 0 and d.steer[0] == -1.0 and d.fragile[0]                   # (a tie is a fragile decision by definition)


def test_one_cylinder_ahead_takes_the_nearest_unblocked_candidate():
    """A cylinder of radius 2 with its axis 4 m ahead: straight on (and the +-7.5 degree steers) enter it within 4 steps."""
    pol, world = _policy("steer", 9, 4, buildings=[(254.0, 250.0, 0.0, 2.0, 100.0)])
    d = pol.decide_uav(_uav(world, (250, 250, 50), 0.0, [[300, 250.5, 50]]))     # the sub-goal a little to the left: s* > 0
    free = np.flatnonzero(~d.blocked[0])
    assert d.blocked[0, 4] and len(free) > 0 and not d.all_blocked_t1[0]
    want = free[np.argmin(np.abs(spr.candidate_steers("steer", 9)[free] - (math.atan2(0.5, 50) / STEERING)))]
    assert d.k[0] == want and d.k[0] > 4                                         # the nearest free steer on the sub-goal's side
    pol0, _ = _policy("steer", 9, 0, buildings=[(254.0, 250.0, 0.0, 2.0, 100.0)])
    assert pol0.decide_uav(_uav(world, (250, 250, 50), 0.0, [[300, 250.5, 50]])).k[0] == 4    # H = 0 blocks nothing
    # above the roof nothing is blocked either
    polr, worldr = _policy("steer", 9, 4, buildings=[(254.0, 250.0, 0.0, 2.0, 40.0)])
    assert polr.decide_uav(_uav(worldr, (250, 250, 50), 0.0, [[300, 250.5, 50]])).k[0] == 4


def test_every_candidate_blocked_takes_the_least_cost_overall():
    """Inside a cylinder of radius 30 every next position is inside too."""
    pol, world = _policy("index", 3, 4, buildings=[(250.0, 250.0, 0.0, 30.0, 100.0)])
    d = pol.decide_uav(_uav(world, (250, 250, 50), 0.0, [[250, 300, 50]]))
    assert d.blocked[0].all() and d.all_blocked_t1[0] and d.k[0] == 2
    d = pol.decide_uav(_uav(world, (250, 250, 50), 0.0, [[300, 250, 50]]))
    assert d.blocked[0].all() and d.k[0] == 1
    # at the box's edge, heading out: all three leave the box with the next step; the sub-goal lies behind (s* = 1)
    pol, world = _policy("index", 3, 4)
    d = pol.decide_uav(_uav(world, (499.5, 250, 50), 0.0, [[400, 250.001, 50]]))
    assert d.blocked[0].all() and d.all_blocked_t1[0] and d.k[0] == 2


def test_every_candidate_blocked_prefers_a_free_next_point():
    """2.5 m from the box's edge, heading out, H = 4: every candidate leaves the box within 4 steps, none with the next one -- the
    least cost; 0.9 m from it only the turns stay inside with the next step (0.866 < 0.9 < 1): a turn, though straight on costs less."""
    pol, world = _policy("index", 3, 4)
    d = pol.decide_uav(_uav(world, (497.5, 250, 50), 0.0, [[499.9, 250, 50]]))
    assert d.blocked[0].all() and not d.all_blocked_t1[0] and d.k[0] == 1
    d = pol.decide_uav(_uav(world, (499.1, 250, 50), 0.0, [[499.9, 250.01, 50]]))
    assert d.blocked[0].all() and not d.all_blocked_t1[0] and d.k[0] == 2


@pytest.mark.parametrize("kind,C", [("index", 3), ("index", 2), ("steer", 9)])
def test_no_sub_goal_left_takes_the_middle_candidate(kind, C):
    pol, world = _policy(kind, C, 4, buildings=[(254.0, 250.0, 0.0, 2.0, 100.0)])
    d = pol.decide_uav(_uav(world, (250, 250, 50), 1.0, np.zeros((0, 3))))
    assert d.k[0] == C // 2 and not d.fragile[0] and not d.all_blocked_t1[0]


def test_batch_and_single_decisions_agree():
    c = load_city26()
    pol, world = spr.city_policy(c, "steer", 9, 4)
    params = dict(max_v=float(c["max_v"]), steering_angle=float(c["steering_angle"]), max_step=int(c["max_step"]), apf_enabled=0)
    n = 32
    batch = po.OracleBatch(world, params, n)
    heading = np.random.default_rng(3).uniform(0, 2 * np.pi, n)
    batch.load_scenarios(c["start_goal"][:n, :3], c["start_goal"][:n, 3:], heading, c["sub_goals"][:n], c["n_sub"][:n],
                         max_v=float(c["max_v"]))
    for _ in range(20):
        d = pol.decide_batch(batch)
        batch.step(d.steer, want_obs=False)
    d = pol.decide_batch(batch)
    for i in range(n):
        u = po.OracleUav(world, params)
        ctypes.memmove(ctypes.addressof(u.u), ctypes.addressof(batch.arr[i]), ctypes.sizeof(po.Uav))
        one = pol.decide_uav(u)
        assert one.k[0] == d.k[i] and one.margin[0] == d.margin[i]


@pytest.mark.parametrize("kind,C", [("index", 3), ("steer", 9)])
def test_fragile_decisions_are_rare_on_the_packaged_missions(kind, C):
    """The cap the GPU tests put on fragile decisions is a condition on the inputs; here it is shown on the reference alone: the
    first 64 rows of data/city26.npz, headings from default_rng(7), 300 steps each under the policy itself, H = 4 -- fragile
    decisions (margin < 1e-6) are at most 0.1 % of all decisions."""
    c = load_city26()
    pol, world = spr.city_policy(c, kind, C, 4)
    params = dict(max_v=float(c["max_v"]), steering_angle=float(c["steering_angle"]), max_step=int(c["max_step"]), apf_enabled=0)
    n = 64
    batch = po.OracleBatch(world, params, n)
    heading = np.random.default_rng(7).uniform(0, 2 * np.pi, n)
    batch.load_scenarios(c["start_goal"][:n, :3], c["start_goal"][:n, 3:], heading, c["sub_goals"][:n], c["n_sub"][:n],
                         max_v=float(c["max_v"]))
    decisions = fragile = collided = 0
    for _ in range(300):
        live = batch.view["done"] == 0
        if not live.any():
            break
        d = pol.decide_batch(batch)
        decisions += int(live.sum())
        fragile += int((d.fragile & live).sum())
        p0 = np.stack([batch.view["px"], batch.view["py"]], 1).copy()
        moved = batch.view["n_sub"] > 0
        batch.step(d.steer, want_obs=False)
        hit = live & moved & (p0 == np.stack([batch.view["px"], batch.view["py"]], 1)).all(1)
        assert not (hit & ~d.all_blocked_t1).any()      # a collision only where every candidate's next point was blocked
        collided += int(hit.sum())
    print(f"{kind} C={C} H=4: {fragile} fragile of {decisions} decisions, {collided} collisions")
    assert decisions > 5000 and fragile <= 1e-3 * decisions
