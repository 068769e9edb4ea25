"""CPU checks of greedy evaluation for f16-MFMA learners (uavenv_eval_episodes_f16): the entry is declared and bound with its
exact prototype, the ABI it shares with uavenv_eval_episodes did not move, and evaluate_policy refuses an f16 learner in a list
before the env is touched."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev

PROTO = "int uavenv_eval_episodes_f16(UavEnv *env, const UavDqnNet *net, const UavEvalArgs *args, void *stream);"


def _header():
    return open(os.path.join(ROOT, "include", "uavenv.h")).read()


def test_the_symbol_is_declared_with_its_exact_prototype_and_bound(tmp_path):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert PROTO in code
    assert "uavenv_eval_episodes_f16" in _lib.SYMBOLS
    # the prototype as gcc sees it: a function pointer of exactly this type takes the symbol without a diagnostic
    src = tmp_path / "proto.c"
    src.write_text('#include "uavenv.h"\n'
                   "int (*f)(UavEnv *, const UavDqnNet *, const UavEvalArgs *, void *) = uavenv_eval_episodes_f16;\n")
    subprocess.run(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "proto.o")], check=True)
    lib = _lib.load()
    fn = lib.uavenv_eval_episodes_f16
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 4
    assert fn.argtypes[0] is ctypes.c_void_p and fn.argtypes[3] is ctypes.c_void_p
    assert fn.argtypes[1] is lib.uavenv_eval_episodes.argtypes[1] and fn.argtypes[2] is lib.uavenv_eval_episodes.argtypes[2]


def test_the_abi_version_and_the_eval_layouts_did_not_move():
    assert _lib.ABI_VERSION == 5 and "#define UAVENV_ABI_VERSION 5" in _header()       # additive: the version stays
    assert ctypes.sizeof(_lib.UavEvalArgs) == 96
    assert ctypes.sizeof(_lib.UavEvalRecord) == 64 == ev.RECORD_DTYPE.itemsize == _lib.EVAL_RECORD_BYTES
    assert [getattr(_lib.UavEvalArgs, f).offset for f, _ in _lib.UavEvalArgs._fields_] == \
        [0, 4, 8, 16, 24, 32, 36, 40, 48, 56, 60, 64, 72, 80, 88, 92]
    assert [getattr(_lib.UavEvalRecord, f).offset for f, _ in _lib.UavEvalRecord._fields_] == \
        [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 61, 62, 63]


class _NoEnv:
    """tests/test_eval_slots.py's stand-in: the env's shape is all a check may look at; any other use fails, so a ValueError
    proves the check ran before anything was read from the device or enqueued."""
    K = 48
    uav_per_env = 4

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

    def __init__(self, mfma="f32"):
        self.net = _Net()
        self.mfma = mfma


@pytest.mark.parametrize("learners", [[_Dqn("f16")], (_Dqn("f16"),), [_Dqn("f16") for _ in range(4)],
                                      [_Dqn(), _Dqn("f16"), _Dqn(), _Dqn()], [_Dqn(), _Dqn(), _Dqn(), _Dqn("f16")]])
def test_a_list_with_an_f16_learner_raises_before_the_env_is_touched(learners):
    with pytest.raises(ValueError, match="f32-MFMA"):
        ev.evaluate_policy(_NoEnv(), learners, 64)


def test_an_f32_list_still_passes_the_learner_checks():
    """The same stand-ins on the f32 MFMA get as far as the env (the _NoEnv assertion), so the refusal above is about mfma."""
    with pytest.raises(AssertionError, match="the env was touched"):
        ev.evaluate_policy(_NoEnv(), [_Dqn() for _ in range(4)], 64)
