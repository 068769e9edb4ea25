"""Whole-episode evaluation of DQN heads of 5 .. 14 layer-2 outputs (uavenv_eval_episodes, uavenv_eval_episodes_slots: the wide
instantiations of k_eval_episodes and k_eval_episodes_slots, layer 2 in groups of four outputs) against the composition of the
launches that took such heads before (tests/eval_wide_cases.py::compose).  Bit for bit: no tolerance anywhere."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev
from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
from eval_wide_cases import (DEV, SHAPES, bias_only, check_equal, compose, env_of, headings, learner_of, missions, state_bytes)

pytestmark = pytest.mark.gpu

# the net seed of every shape: one whose composition (the reference alone) takes an action >= 4 (of ("dueling", 4): its last
# action, 3 -- there the fifth output is the value head) and ends episodes in success, lose and with collisions
SEED = 2


@pytest.mark.parametrize("kind,A", SHAPES)
def test_equals_the_composed_launches(kind, A):
    n, cap = 1024, 300
    scn = missions(n)
    rows = np.arange(n)
    v0 = headings(n, 10 * A + len(kind))
    L = learner_of(kind, A, SEED)
    ref = compose([L], 1, A, 0, scn, rows, v0, cap)
    # conditions on the reference alone
    assert ref["act"].max() >= min(4, A - 1)
    assert (ref["outcome"] == _lib.EVAL_SUCCESS).any() and (ref["outcome"] == _lib.EVAL_LOSE).any() and ref["coll"].sum() > 0
    env = env_of(64, A)
    res = ev.evaluate_policy(env, L, n, scenarios=scn, v0=v0, max_steps=cap, trajectory_steps=cap)
    check_equal(res.host_records(), res, ref, v0, cap, 1)
    env.close()


ARGMAX = [(0,), (3,), (4,), (7,), (8,), (12,), (-1,), (3, 4), (4, -1), (7, 8)]   # (-1: A - 1); a pair: a tie, the first wins


@pytest.mark.parametrize("kind,A", [("dqn", 14), ("dueling", 13)])
def test_constructed_argmax_and_ties(kind, A):
    """fc1 = 0 and b1 = 0: q depends on b2 only.  b2 = 5 onehot(k): every action is k; b2[k] = b2[k'] = 5: the first, k."""
    n, cap = 128, 24
    scn = missions(n)
    rows = np.arange(n)
    v0 = headings(n, 3)
    env = env_of(64, A)
    L = learner_of(kind, A, 7)
    for case in ARGMAX:
        ks = [k % A for k in case]
        b2 = np.zeros(A)
        b2[ks] = 5.0
        bias_only(L, b2)
        res = ev.evaluate_policy(env, L, n, scenarios=scn, v0=v0, max_steps=cap, trajectory_steps=cap)
        rec = res.host_records()
        act = res.actions.cpu().numpy()
        flown = np.arange(cap)[None, :] < rec["steps"][:, None]
        assert (rec["steps"] > 0).all() and (act[flown] == ks[0]).all() and (act[~flown] == -1).all(), case
        check_equal(rec, res, compose([L], 1, A, 0, scn, rows, v0, cap), v0, cap, 1)
    env.close()


@pytest.mark.parametrize("kind,A", [("dqn", 9), ("dueling", 13)])
@pytest.mark.parametrize("apf", [0, 1])
def test_slots_entry_equals_the_composition_slot_by_slot(apf, kind, A):
    U, n, cap = 4, 512, 200
    scn = missions()
    rows = np.arange(n)
    v0 = headings(n, 100 * apf + A)
    Ls = [learner_of(kind, A, 40 + j) for j in range(U)]
    env = env_of(64, A, apf, U)
    res = ev.evaluate_policy(env, Ls, n, scenarios=scn, v0=v0, max_steps=cap, trajectory_steps=cap)
    rec = res.host_records()
    ref = compose(Ls, U, A, apf, scn, rows, v0, cap)
    check_equal(rec, res, ref, v0, cap, U)
    assert ref["act"].max() >= 4 and (rec["steps"] > 0).all()
    other = ev.evaluate_policy(env, [Ls[0]] * U, n, scenarios=scn, v0=v0, max_steps=cap).host_records()   # the nets differ
    assert other[0::U].tobytes() == rec[0::U].tobytes() and other[1::U].tobytes() != rec[1::U].tobytes()
    env.close()


@pytest.mark.parametrize("kind,A", [("dqn", 9), ("dueling", 13)])
def test_single_wide_learner_on_an_apf_env(kind, A):
    n, cap = 512, 200
    scn = missions()
    rows = np.arange(n)
    v0 = headings(n, 5 + A)
    L = learner_of(kind, A, 61)
    env = env_of(64, A, 1, 1)
    res = ev.evaluate_policy(env, L, n, scenarios=scn, v0=v0, max_steps=cap, trajectory_steps=cap)
    ref = compose([L], 1, A, 1, scn, rows, v0, cap)
    check_equal(res.host_records(), res, ref, v0, cap, 1)
    assert ref["act"].max() >= 4
    env.close()


def _bytes(res):
    return res.records.cpu().numpy().tobytes() + res.positions.cpu().numpy().tobytes() + res.actions.cpu().numpy().tobytes()


def test_two_kernels_one_answer_and_the_random_policy():
    A = 9
    env = env_of(64, A)
    n = 1000 + 37
    for kind in ("dqn", "dueling"):
        L = learner_of(kind, A, 21)
        for eps in (0.0, 0.3):
            kw = dict(seed=9, eps=eps, first=5, max_steps=300, trajectory_steps=8)   # the bank, default headings (no v0)
            one, lst = ev.evaluate_policy(env, L, n, **kw), ev.evaluate_policy(env, [L], n, **kw)
            assert _bytes(one) == _bytes(lst)
            assert (one.host_records()["steps"] > 0).all()
        greedy = ev.evaluate_policy(env, L, n, **dict(kw, eps=0.0)).host_records()
        assert greedy.tobytes() != one.host_records().tobytes()                         # the draws reached the actions
        # eps = 1: every action is the draw -- the scripted baseline's on the same missions (the same eval_eps_action)
        kw = dict(seed=9, eps=1.0, first=5, max_steps=300, trajectory_steps=8)
        rnd = ev.evaluate_policy(env, L, n, **kw)
        scr = ev.evaluate_scripted_policy(env, n, action="index", **kw)
        assert _bytes(rnd) == _bytes(scr)
        assert rnd.actions.max().item() >= 4
    env.close()


def test_placement_invariance():
    A, U = 9, 4
    n = 3000 + 37                                  # neither a multiple of 64 nor of U
    env = env_of(64, A)
    L = learner_of("dqn", A, 3)
    kw = dict(seed=9, max_steps=300, trajectory_steps=4)
    assert _bytes(ev.evaluate_policy(env, L, n, max_workgroups=1, **kw)) == _bytes(ev.evaluate_policy(env, L, n, **kw))
    env.close()
    env = env_of(64, 13, 1, U)
    Ls = [learner_of("dueling", 13, 50 + j) for j in range(U)]
    one = ev.evaluate_policy(env, Ls, n, max_workgroups=1, **kw)
    assert _bytes(one) == _bytes(ev.evaluate_policy(env, Ls, n, **kw))
    rec = one.host_records()
    assert (rec["steps"] > 0).all() and (rec["slot"] == np.arange(n) % U).all()
    env.close()


def _last_error():
    return _lib.load().uavenv_last_error().decode("utf-8", "replace")


def test_refusals_and_the_env_is_left_alone():
    rec = torch.zeros((64, 64), dtype=torch.uint8, device=DEV)

    def args():
        a = _lib.UavEvalArgs()
        a.n, a.records = 64, rec.data_ptr()
        return a

    def single(env, net, f16=False):
        fn = env.lib.uavenv_eval_episodes_f16 if f16 else env.lib.uavenv_eval_episodes
        return fn(env._h, C.byref(net), C.byref(args()), env._stream())

    def slots(env, net):
        arr = (C.POINTER(_lib.UavDqnNet) * 1)(C.pointer(net))
        return env.lib.uavenv_eval_episodes_slots(env._h, arr, 1, C.byref(args()), env._stream())

    def prepared(A):
        env = env_of(16, A)
        env.reset(seed=4)
        act = torch.zeros(env.N, dtype=torch.float32, device=DEV)
        for _ in range(3):
            env.step(act, skip_done=True)
        torch.cuda.synchronize()
        return env, state_bytes(env), env.lib.uavenv_tick(env._h)

    def unchanged(env, before, tick):
        torch.cuda.synchronize()
        return state_bytes(env) == before and env.lib.uavenv_tick(env._h) == tick

    L14 = learner_of("dqn", 14, 2)
    # 15 layer-2 outputs on an env of 15 actions: only the head is wrong
    env, before, tick = prepared(15)
    n15 = _lib.UavDqnNet.from_buffer_copy(L14.net); n15.n_actions = 15
    assert single(env, n15) == _lib.EINVAL and "<= %d outputs" % _lib.EVAL_MAX_OUTPUTS in _last_error()
    assert slots(env, n15) == _lib.EINVAL and "<= %d outputs" % _lib.EVAL_MAX_OUTPUTS in _last_error()
    assert unchanged(env, before, tick)
    env.close()
    # a wide net on an env with another action count; the f16 entry's own limit
    L9, L6 = learner_of("dueling", 9, 2), learner_of("dqn", 6, 2)
    env, before, tick = prepared(6)
    assert single(env, L9.net) == _lib.EINVAL and slots(env, L9.net) == _lib.EINVAL
    h6 = _lib.UavDqnNet.from_buffer_copy(L6.net); h6.mfma_dtype = _lib.MFMA_F16
    assert single(env, h6, f16=True) == _lib.EINVAL and "<= 4 outputs" in _last_error()
    assert unchanged(env, before, tick)
    # and the wide evaluations that are taken leave the env as it was, too
    assert single(env, L6.net) == 0 and slots(env, L6.net) == 0
    assert ev.evaluate_policy(env, L6, 512, max_steps=100).summary()["episodes"] == 512
    assert L6.evaluate(env, 256, max_steps=50, eps=0.2).summary()["episodes"] == 256
    assert unchanged(env, before, tick)
    env.close()


def test_plugin_evaluate_policy_with_nine_actions(tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver
    monkeypatch.chdir(tmp_path)                    # (the config's paths are relative to the working directory)
    xml = driver.make_config_dir(str(tmp_path), "DuelingDQN", num_envs=64, num_uav=4)
    t_xml = tmp_path / "config" / "Trainer.xml"
    t_xml.write_text(re.sub(r"<output>3</output>", "<output>9</output>", t_xml.read_text()))
    torch.manual_seed(0)
    env = driver.simulator(xml).env
    learners = [u.Trainer.learner for u in env.Agents]
    assert env.backend.cfg.n_actions == 9 and all(isinstance(L, FusedDQNLearner) and L.dueling and L.n_actions == 9 for L in learners)
    before = state_bytes(env.backend)
    n = 256
    summ = env.evaluate_policy(n_episodes=n, seed=1, max_steps=300)
    assert len(summ) == 4
    scn_u, v0 = env._evaluation_missions(n, 1, True)
    res = ev.evaluate_policy(env.backend, learners, n * 4, scenarios=scn_u, v0=v0, seed=1, max_steps=300, trajectory_steps=8)
    rec = res.host_records()
    for j in range(4):
        assert summ[j] == ev.summarize(rec[j::4]), j
        assert summ[j]["episodes"] == n and summ[j]["invalid"] == 0
    assert res.actions.max().item() >= 4
    torch.cuda.synchronize()
    assert state_bytes(env.backend) == before
