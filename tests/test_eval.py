"""CPU checks of greedy policy evaluation (uavenv_eval_episodes): the two new ABI structs against the header as gcc sees it,
summary() arithmetic, and argument refusals that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev


def test_eval_struct_layouts_match_the_header_as_gcc_sees_it(tmp_path):
    structs = {"UavEvalRecord": _lib.UavEvalRecord, "UavEvalArgs": _lib.UavEvalArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "uavenv.h"', 'int main(void){']
    for name, ct in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines.append('printf("codes %d %d %d %d\\n", UAVENV_EVAL_SUCCESS, UAVENV_EVAL_LOSE, UAVENV_EVAL_TRUNCATED, UAVENV_EVAL_INVALID);')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {l.split()[0]: l.split()[1:] for l in out}
    for name, ct in structs.items():
        assert int(got[name][0]) == ctypes.sizeof(ct), name
        for fname, _ in ct._fields_:
            assert int(got[f"{name}.{fname}"][0]) == getattr(ct, fname).offset, (name, fname)
    assert ctypes.sizeof(_lib.UavEvalRecord) == 64 == ev.RECORD_DTYPE.itemsize
    assert [int(x) for x in got["codes"]] == [_lib.EVAL_SUCCESS, _lib.EVAL_LOSE, _lib.EVAL_TRUNCATED, _lib.EVAL_INVALID]
    for fname, _ in _lib.UavEvalRecord._fields_:      # the numpy view of a record has the same fields at the same offsets
        assert ev.RECORD_DTYPE.fields[fname][1] == getattr(_lib.UavEvalRecord, fname).offset


def test_summary_arithmetic_on_synthetic_records():
    rec = np.zeros(6, dtype=ev.RECORD_DTYPE)
    rec["outcome"] = [1, 1, 2, 4, 5, 1]
    rec["ret"] = [10.0, 20.0, -5.0, 1.0, 999.0, 4.0]
    rec["steps"] = [10, 20, 150, 600, 0, 2]
    rec["path_len"] = [1.0, 2.0, 3.0, 4.0, 100.0, 5.0]
    rec["energy"] = [2.0, 2.0, 2.0, 2.0, 100.0, 7.0]
    rec["subgoals"] = [1, 2, 0, 3, 50, 4]
    rec["collisions"] = [0, 1, 2, 3, 50, 4]
    rec["total_score"] = [5.0, 6.0, 7.0, 8.0, 100.0, 9.0]
    s = ev.summarize(rec)
    assert s["episodes"] == 6 and s["success"] == 3 and s["lose"] == 1 and s["truncated"] == 1 and s["invalid"] == 1
    assert s["success_rate"] == 3 / 5 and s["lose_rate"] == 1 / 5
    assert s["mean_return"] == pytest.approx(30.0 / 5)
    assert s["mean_steps"] == pytest.approx(782 / 5)
    assert s["mean_path_len"] == pytest.approx(15.0 / 5)
    assert s["mean_energy"] == pytest.approx(15.0 / 5)
    assert s["mean_subgoals"] == pytest.approx(10 / 5)
    assert s["mean_collisions"] == pytest.approx(10 / 5)
    assert s["average_score"] == pytest.approx(35.0 / 5)
    empty = ev.summarize(np.zeros(0, dtype=ev.RECORD_DTYPE))
    assert empty["episodes"] == 0 and empty["success_rate"] == 0.0


class _NoEnv:
    """Stands in for an env: any use of it fails, so a ValueError proves the check ran before anything was enqueued."""
    K = 48

    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(n_episodes=0), dict(n_episodes=-3), dict(n_episodes=2.5), dict(first=-1),
                                dict(eps=-0.1), dict(eps=1.5), dict(eps=float("nan")), dict(max_steps=-1),
                                dict(trajectory_steps=-2), dict(max_workgroups=-1),
                                dict(scenarios=(np.zeros((4, 6)), np.zeros((4, 7, 3)), np.zeros(4))),
                                dict(scenarios=(np.zeros((0, 6)), np.zeros((0, 48, 3)), np.zeros(0)))])
def test_bad_arguments_raise_value_error_without_a_device(kw):
    args = dict(n_episodes=64)
    args.update(kw)
    n = args.pop("n_episodes")
    with pytest.raises(ValueError):
        ev.evaluate_policy(_NoEnv(), object(), n, **args)


def test_held_out_scenarios_rejects_bad_m():
    with pytest.raises(ValueError):
        ev.held_out_scenarios(_NoEnv(), 0, seed=1)


class _NetOnly:
    net = object()


@pytest.mark.parametrize("v0", [np.zeros((63, 2)), np.zeros((64, 3)), np.zeros(128)])
def test_bad_v0_and_learner_raise_before_the_env_is_touched(v0):
    with pytest.raises(ValueError):
        ev.evaluate_policy(_NoEnv(), _NetOnly(), 64, v0=v0)
    with pytest.raises(ValueError):                  # a learner without the fused net
        ev.evaluate_policy(_NoEnv(), object(), 64)


def test_slot_scenarios_give_every_slot_every_mission():
    import torch
    m, K, U = 5, 48, 4
    rng = np.random.default_rng(3)
    scn = (torch.tensor(rng.normal(size=(m, 6))), torch.tensor(rng.normal(size=(m, K, 3))),
           torch.tensor(rng.integers(0, K, m), dtype=torch.int32))
    (sg, sub, ns), v0 = ev.slot_scenarios(scn, U, 2.0, seed=9)
    assert sg.shape == (m * U, 6) and sub.shape == (m * U, K, 3) and ns.shape == (m * U,) and v0.shape == (m * U, 2)
    for e in range(m * U):                           # episode e = mission e // U as slot e % U
        r = e // U
        assert torch.equal(sg[e], scn[0][r]) and torch.equal(sub[e], scn[1][r]) and int(ns[e]) == int(scn[2][r])
        assert torch.equal(v0[e], v0[r * U])         # one heading per mission, whatever the slot
    assert np.allclose(np.hypot(v0[:, 0].numpy(), v0[:, 1].numpy()), 2.0)
    assert len(set(v0[::U, 0].tolist())) == m
