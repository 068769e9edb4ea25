"""CPU checks of greedy DQN evaluation with one net per UAV slot (uavenv_eval_episodes_slots): the entry is declared and bound,
the ABI it shares with uavenv_eval_episodes did not move, and evaluate_policy refuses bad learner lists before the env is touched."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev


def test_the_new_symbol_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "uavenv_eval_episodes_slots" in _lib.SYMBOLS
    assert re.search(r"int uavenv_eval_episodes_slots\(UavEnv \*env, const UavDqnNet \*const \*nets, int32_t n_nets,\s*"
                     r"const UavEvalArgs \*args, void \*stream\);", code)
    assert _lib.ABI_VERSION == 5 and "#define UAVENV_ABI_VERSION 5" in hdr       # additive: the version stays
    lib = _lib.load()
    assert hasattr(lib, "uavenv_eval_episodes_slots")
    assert lib.uavenv_eval_episodes_slots.argtypes[2] is ctypes.c_int32 and len(lib.uavenv_eval_episodes_slots.argtypes) == 5


def test_eval_struct_layouts_are_unchanged_as_gcc_sees_them(tmp_path):
    structs = {"UavEvalRecord": _lib.UavEvalRecord, "UavEvalArgs": _lib.UavEvalArgs, "UavDqnNet": _lib.UavDqnNet}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "uavenv.h"', 'int main(void){']
    for name, ct in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines.append('printf("slots %d\\n", UAVENV_SAC_LOOP_MAX_SLOTS);')
    lines.append('int (*f)(UavEnv *, const UavDqnNet *const *, int32_t, const UavEvalArgs *, void *) = uavenv_eval_episodes_slots;')
    lines.append('(void)f;')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout.o"
    subprocess.run(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(exe)], check=True)   # the prototype
    lines = [l for l in lines if "uavenv_eval_episodes_slots" not in l and l != "(void)f;"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {l.split()[0]: l.split()[1:] for l in out}
    for name, ct in structs.items():
        assert int(got[name][0]) == ctypes.sizeof(ct), name
        for fname, _ in ct._fields_:
            assert int(got[f"{name}.{fname}"][0]) == getattr(ct, fname).offset, (name, fname)
    # the layouts as they were before this entry existed
    assert ctypes.sizeof(_lib.UavEvalRecord) == 64 == ev.RECORD_DTYPE.itemsize and ctypes.sizeof(_lib.UavEvalArgs) == 96
    assert [getattr(_lib.UavEvalArgs, f).offset for f, _ in _lib.UavEvalArgs._fields_] == \
        [0, 4, 8, 16, 24, 32, 36, 40, 48, 56, 60, 64, 72, 80, 88, 92]
    assert [getattr(_lib.UavEvalRecord, f).offset for f, _ in _lib.UavEvalRecord._fields_] == \
        [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 61, 62, 63]
    assert int(got["slots"][0]) == _lib.SAC_LOOP_MAX_SLOTS == 8


class _NoEnv:
    """Stands in for an env: its shape (K, uav_per_env) is all a check may look at; any other use fails, so a ValueError proves
    the check ran before anything was read from the device or enqueued."""
    K = 48
    uav_per_env = 4

    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the arguments were checked")


class _OnlyK:
    """tests/test_eval.py's stand-in: a single learner's checks may not even ask for uav_per_env."""
    K = 48

    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the arguments were checked")


class _Net:
    def __init__(self, n_actions=3, dueling=0):
        self.n_actions, self.dueling = n_actions, dueling

    @property
    def local(self):
        raise AssertionError("the net's parameter block was read before the arguments were checked")


class _Dqn:
    """Looks like a FusedDQNLearner to the argument checks."""

    def __init__(self, n_actions=3, dueling=0):
        self.net = _Net(n_actions, dueling)


class _Sac:
    """A fused SAC learner has no `net`."""
    action_bound = 1.0
    _blocks = ()


@pytest.mark.parametrize("learners", [[], (), [_Dqn(), _Dqn()], [_Dqn(), _Dqn(), _Dqn()], [_Dqn() for _ in range(5)],   # length
                                      [_Dqn() for _ in range(8)],
                                      [_Dqn(), object(), _Dqn(), _Dqn()], [object()], [None], [_Sac()],                 # not learners
                                      [_Dqn(), _Sac(), _Dqn(), _Dqn()],
                                      [_Dqn(), _Dqn(), _Dqn(dueling=1), _Dqn()],                                       # mixed kinds
                                      [_Dqn(dueling=1), _Dqn(), _Dqn(), _Dqn()],
                                      [_Dqn(3), _Dqn(3), _Dqn(3), _Dqn(2)]])                                           # action counts
def test_bad_learner_lists_raise_value_error_without_touching_the_env(learners):
    with pytest.raises(ValueError):
        ev.evaluate_policy(_NoEnv(), learners, 64)
    with pytest.raises(ValueError):
        ev.evaluate_policy(_NoEnv(), learners, 64, v0=np.zeros((64, 2)))


@pytest.mark.parametrize("kw", [dict(n_episodes=0), dict(n_episodes=2.5), dict(first=-1), dict(eps=1.5), dict(eps=float("nan")),
                                dict(max_steps=-1), dict(trajectory_steps=-2), dict(max_workgroups=-1),
                                dict(scenarios=(np.zeros((4, 6)), np.zeros((4, 7, 3)), np.zeros(4))),
                                dict(v0=np.zeros((63, 2))), dict(v0=np.zeros((64, 3))), dict(v0=np.zeros(128))])
def test_bad_arguments_with_a_good_list_raise_without_touching_the_env(kw):
    args = dict(n_episodes=64)
    args.update(kw)
    n = args.pop("n_episodes")
    with pytest.raises(ValueError):
        ev.evaluate_policy(_NoEnv(), [_Dqn() for _ in range(4)], n, **args)
    with pytest.raises(ValueError):
        ev.evaluate_policy(_NoEnv(), [_Dqn()], n, **args)


def test_the_learner_check_comes_before_v0_and_the_length_check_after():
    """Today's order: the learner check, then v0, and only then anything of the env (the list's length against uav_per_env)."""
    with pytest.raises(ValueError, match="fused"):
        ev.evaluate_policy(_OnlyK(), [_Dqn(), object()], 64, v0=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="v0"):
        ev.evaluate_policy(_OnlyK(), [_Dqn(), _Dqn()], 64, v0=np.zeros((3, 2)))     # (a bad length too: v0 is reported first)
    with pytest.raises(ValueError, match="uav_per_env"):
        ev.evaluate_policy(_NoEnv(), [_Dqn(), _Dqn()], 64)


@pytest.mark.parametrize("v0", [np.zeros((63, 2)), np.zeros((64, 3)), np.zeros(128)])
def test_single_learner_refusals_still_raise_before_the_env_is_touched(v0):
    with pytest.raises(ValueError):
        ev.evaluate_policy(_OnlyK(), _Dqn(), 64, v0=v0)
    with pytest.raises(ValueError):
        ev.evaluate_policy(_OnlyK(), object(), 64)
    with pytest.raises(ValueError):
        ev.evaluate_policy(_OnlyK(), _Sac(), 64)
    with pytest.raises(ValueError):
        ev.evaluate_policy(_OnlyK(), _Dqn(), 0)


def test_signature_and_defaults_did_not_change():
    sig = inspect.signature(ev.evaluate_policy)
    assert list(sig.parameters) == ["env", "learner", "n_episodes", "scenarios", "first", "seed", "eps", "max_steps", "v0",
                                    "trajectory_steps", "max_workgroups"]
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(scenarios=None, first=0, seed=0, eps=0.0, max_steps=0, v0=None, trajectory_steps=0, max_workgroups=0)
    assert sig.parameters["scenarios"].kind is inspect.Parameter.KEYWORD_ONLY
