"""The head limit of the whole-episode evaluation, without a GPU: one number in the header, the Python mirror and the device
header, and evaluate_policy's refusals of heads beyond it before anything is touched."""
import os
import re
import types

import pytest

from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_limit():
    text = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    return int(re.search(r"^#define\s+UAVENV_EVAL_MAX_OUTPUTS\s+(\d+)", text, re.M).group(1))


def test_the_header_and_the_python_mirror_agree():
    assert _header_limit() == _lib.EVAL_MAX_OUTPUTS == 14


def test_the_limit_is_what_the_act_and_grad_kernels_take():
    text = open(os.path.join(ROOT, "dqn_based_uav_3d_path_planer_amd", "csrc", "qnet_device.hpp")).read()
    k_max_out = int(re.search(r"constexpr\s+int\s+kMaxOut\s*=\s*(\d+)\s*;", text).group(1))
    assert _header_limit() == k_max_out - 2


class _NoEnv:
    """Stands in for an env: any use of it fails, so a ValueError proves the check ran before anything was enqueued."""
    K = 48

    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the arguments were checked")


def _learner(n_actions, dueling, mfma="f32"):
    return types.SimpleNamespace(net=types.SimpleNamespace(n_actions=n_actions, dueling=dueling), mfma=mfma)


@pytest.mark.parametrize("n_actions,dueling", [(15, 0), (14, 1), (32, 0)])
def test_more_than_14_outputs_raise_before_the_env_is_touched(n_actions, dueling):
    with pytest.raises(ValueError, match="at most 14"):
        ev.evaluate_policy(_NoEnv(), _learner(n_actions, dueling), 64)
    with pytest.raises(ValueError, match="at most 14"):
        ev.evaluate_policy(_NoEnv(), [_learner(n_actions, dueling)], 64)


@pytest.mark.parametrize("n_actions,dueling", [(5, 0), (4, 1), (9, 0)])
def test_an_f16_learner_with_more_than_4_outputs_raises_before_the_env_is_touched(n_actions, dueling):
    with pytest.raises(ValueError, match="at most 4"):
        ev.evaluate_policy(_NoEnv(), _learner(n_actions, dueling, mfma="f16"), 64)
