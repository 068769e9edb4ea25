"""CPU checks of SAC policy evaluation (uavenv_eval_episodes_sac): the new ABI struct against the header as gcc sees it, and the
argument refusals of evaluate_sac_policy / sac_noise that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev


def test_sac_eval_struct_layout_matches_the_header_as_gcc_sees_it(tmp_path):
    name, ct = "UavSacEvalArgs", _lib.UavSacEvalArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "uavenv.h"', 'int main(void){']
    lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
    for fname, _ in ct._fields_:
        lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines.append('printf("modes %d %d\\n", UAVENV_EVAL_SAC_MEAN, UAVENV_EVAL_SAC_SAMPLE);')
    lines.append('printf("record %zu slots %d\\n", sizeof(UavEvalRecord), UAVENV_SAC_LOOP_MAX_SLOTS);')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {l.split()[0]: l.split()[1:] for l in out}
    assert int(got[name][0]) == ctypes.sizeof(ct)
    for fname, _ in ct._fields_:
        assert int(got[f"{name}.{fname}"][0]) == getattr(ct, fname).offset, fname
    assert [int(x) for x in got["modes"]] == [_lib.EVAL_SAC_MEAN, _lib.EVAL_SAC_SAMPLE]
    assert ev.SAC_MODES == {"mean": _lib.EVAL_SAC_MEAN, "sample": _lib.EVAL_SAC_SAMPLE}
    assert int(got["record"][0]) == 64 == _lib.EVAL_RECORD_BYTES                 # the record did not change
    assert int(got["record"][2]) == _lib.SAC_LOOP_MAX_SLOTS
    # what the DQN entry and this one share sits at the same offsets up to the seed
    for fname in ("n", "first", "start_goal", "sub", "nsub", "m", "max_steps", "v0", "seed"):
        assert getattr(_lib.UavSacEvalArgs, fname).offset == getattr(_lib.UavEvalArgs, fname).offset, fname


def test_the_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    for sym in ("uavenv_eval_episodes_sac", "uavenv_eval_noise_fill"):
        assert sym in _lib.SYMBOLS and f"int {sym}(" in hdr
    assert _lib.ABI_VERSION == 5 and "#define UAVENV_ABI_VERSION 5" in hdr       # additive: the version stays


class _NoEnv:
    """Stands in for an env: its shape (K, uav_per_env) is all a check may look at; any other use fails, so a ValueError proves
    the check ran before anything was read from the device or enqueued."""
    K = 48
    uav_per_env = 4

    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the arguments were checked")


class _Sac:
    """Looks like a FusedSACLearner to the argument checks; its block must never be dereferenced."""

    def __init__(self, bound=1.0):
        self.action_bound = bound

    @property
    def _blocks(self):
        return self

    def __getitem__(self, k):
        raise AssertionError("the learner's parameter block was read before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(n_episodes=0), dict(n_episodes=-3), dict(n_episodes=2.5), dict(first=-1),
                                dict(max_steps=-1), dict(trajectory_steps=-2), dict(max_workgroups=-1),
                                dict(mode="greedy"), dict(mode=None), dict(mode=1),
                                dict(scenarios=(np.zeros((4, 6)), np.zeros((4, 7, 3)), np.zeros(4))),
                                dict(scenarios=(np.zeros((0, 6)), np.zeros((0, 48, 3)), np.zeros(0))),
                                dict(scenarios=(np.zeros((4, 6)), np.zeros((4, 48, 3)))),
                                dict(v0=np.zeros((63, 2))), dict(v0=np.zeros((64, 3))), dict(v0=np.zeros(128))])
def test_bad_arguments_raise_value_error_without_a_device(kw):
    args = dict(n_episodes=64)
    args.update(kw)
    n = args.pop("n_episodes")
    with pytest.raises(ValueError):
        ev.evaluate_sac_policy(_NoEnv(), _Sac(), n, **args)
    with pytest.raises(ValueError):
        ev.evaluate_sac_policy(_NoEnv(), [_Sac() for _ in range(4)], n, **args)


@pytest.mark.parametrize("learners", [object(), [], [object()], [_Sac(), object(), _Sac(), _Sac()],
                                      [_Sac(), _Sac()], [_Sac() for _ in range(5)],                 # neither 1 nor uav_per_env
                                      _Sac(0.0), _Sac(-1.0), _Sac(float("nan")), _Sac(float("inf")),
                                      [_Sac(1.0), _Sac(1.0), _Sac(2.0), _Sac(1.0)]])                # one action_bound per call
def test_bad_learners_raise_value_error_without_a_device(learners):
    with pytest.raises(ValueError):
        ev.evaluate_sac_policy(_NoEnv(), learners, 64)


def test_evaluate_policy_still_refuses_what_is_not_a_dqn_learner():
    with pytest.raises(ValueError):
        ev.evaluate_policy(_NoEnv(), _Sac(), 64)


@pytest.mark.parametrize("n,steps", [(0, 4), (-1, 4), (4, 0), (2.5, 4), (1 << 16, 1 << 15)])
def test_sac_noise_rejects_bad_shapes_without_a_device(n, steps):
    with pytest.raises(ValueError):
        ev.sac_noise(n, steps, seed=1)


def test_fused_sac_learner_has_the_evaluate_method():
    from dqn_based_uav_3d_path_planer_amd.sac import FusedSACLearner
    import inspect
    sig = inspect.signature(FusedSACLearner.evaluate)
    assert list(sig.parameters)[:3] == ["self", "env", "n_episodes"]
    sig = inspect.signature(ev.evaluate_sac_policy)
    assert [p for p in sig.parameters] == ["env", "learners", "n_episodes", "scenarios", "first", "seed", "mode", "max_steps", "v0",
                                           "trajectory_steps", "max_workgroups"]
    assert sig.parameters["mode"].default == "mean" and sig.parameters["scenarios"].kind is inspect.Parameter.KEYWORD_ONLY
