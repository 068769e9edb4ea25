"""Greedy evaluation of an f16-MFMA learner in one launch (uavenv_eval_episodes_f16, k_eval_episodes_h) against the composition of
the launches that existed before it, on a fresh env of the same obs_dtype with one agent per episode: set_state -> observe ->
per step uavenv_dqn_act(net, obs, the env's obs_dtype, eps = -1: always greedy) + uavenv_step with STEP_SKIP_DONE, accumulated on
the host.  The acting kernels are held to the float64 forward with f16 operands by tests/test_dqn_act_kernels_gpu.py; equality
with them carries that bar to the evaluation.  Every comparison is an equality."""
import ctypes as C

import numpy as np
import pytest
import torch

from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev
from dqn_based_uav_3d_path_planer_amd.data import load_city26, make_city26_env
from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PARAM = {"w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99", "Update_loop": "3"}
KINDS = {"f16": torch.float16, "packed": "packed"}


def _env(n, obs, **kw):
    return make_city26_env(n, obs_dtype=KINDS[obs], **kw)


def _learner(kind, seed, straight=False, mfma="f16"):
    torch.manual_seed(seed)
    net = "VAnet2" if kind == "dueling" else "Qnet2"
    L = FusedDQNLearner(dict(PARAM, NetWork=net), kind, device=DEV, mfma=mfma)
    if straight:                                    # fc2's bias favours the middle action (steer 0): "fly straight"
        with torch.no_grad():
            L.q_local.fc2.bias.copy_(torch.tensor([0.0, 5.0, 0.0], device=DEV))
    return L


def _hand_rows(K):
    """tests/test_eval_gpu.py's rows for the rare branches: an empty list, the final sub-goal within reach, the goal within 7 m
    of a UAV that is still >= 7 m from its sub-goal.  Flown at z = 90 (above every roof of the stock world)."""
    sg = np.zeros((3, 6)); sub = np.zeros((3, K, 3)); ns = np.zeros(3, np.int32)
    sg[0] = [100, 100, 90, 300, 300, 90]; ns[0] = 0
    sg[1] = [100, 100, 90, 300, 300, 90]; sub[1, 0] = [100, 100, 90]; sub[1, 1] = [101, 100, 90]; ns[1] = 2
    sg[2] = [244, 250, 90, 250, 250, 90]; sub[2, 0] = [253, 250, 90]; ns[2] = 1
    return sg, sub, ns


_SCN = {}


def _scenarios():
    """The hand-built rows + the packaged bank + held-out planner rows (device tensors; built once, never written)."""
    if "s" not in _SCN:
        env = _env(64, "packed")
        sg0, sub0, ns0 = env.bank_read(0, 1024)
        hsg, hsub, hns = ev.held_out_scenarios(env, 1024, seed=0xE7A1)
        a, b, c = _hand_rows(env.K)
        sg = np.concatenate([a, sg0, hsg.cpu().numpy()])
        sub = np.concatenate([b, sub0, hsub.cpu().numpy()])
        ns = np.concatenate([c, ns0, hns.cpu().numpy()]).astype(np.int32)
        _SCN["s"] = (torch.tensor(sg, device=DEV), torch.tensor(sub, device=DEV), torch.tensor(ns, device=DEV))
        env.close()
    return _SCN["s"]


def _v0(n, seed):
    t = np.random.default_rng(seed).uniform(0, 2 * np.pi, n)
    return np.stack([np.cos(t), np.sin(t)], 1)      # Max_V = 1


def _compose(L, obs, scn, rows, v0, max_steps):
    """The same episodes through the launches of the parent commit: agent i of a fresh env with `obs` rows is episode i."""
    n = len(rows)
    sg, sub, ns = (x.cpu().numpy() for x in scn)
    env2 = _env(n, obs)
    kin = np.concatenate([sg[rows, :3], v0, sg[rows, 3:]], 1)
    nsub = ns[rows]
    env2.set_state(0, kin, np.zeros(n, np.int32), nsub, sub[rows], alias=(nsub >= 2).astype(np.int32))
    cur = env2.observe()
    out = env2.alloc_out(want_energy=True)
    act = torch.zeros(n, dtype=torch.int32, device=DEV)
    st = env2.get_state(0, n)
    final = st.copy()
    ret, energy = np.zeros(n), np.zeros(n)
    steps, coll = np.zeros(n, np.int64), np.zeros(n, np.int64)
    outcome = np.zeros(n, np.int64)
    pos, acts = [st[:, :3].copy()], []
    cap = nsub.astype(np.int64) * env2.cfg.max_step + 1
    t = 0
    while (outcome == 0).any():
        rc = env2.lib.uavenv_dqn_act(C.byref(L.net), cur.data_ptr(), env2.obs_code, n, -1.0, 5, t, act.data_ptr(), None, None,
                                     env2._stream())
        _lib.check(rc, "uavenv_dqn_act")
        env2.step(act, out, skip_done=True)
        cur, out.obs = out.obs, cur                                 # the rows just written are the next step's input
        nst = env2.get_state(0, n)
        v = (out.valid.cpu().numpy() == 1) & (outcome == 0)        # (a truncated agent flies on here; its episode has ended)
        ret[v] += out.reward.cpu().numpy()[v]
        energy[v] += out.energy.cpu().numpy()[v]
        steps[v] += 1
        same = (nst[:, 0] == st[:, 0]) & (nst[:, 1] == st[:, 1]) & (nst[:, 2] == st[:, 2])
        coll[v & same & (st[:, 11] > 0)] += 1                       # a moved step whose position did not change
        a = act.cpu().numpy().astype(np.int64)
        a[~v] = -1
        acts.append(a)
        p = nst[:, :3].copy()
        p[~v] = np.nan
        pos.append(p)
        inf = out.info.cpu().numpy()
        d = v & (out.agent_done.cpu().numpy() == 1)
        outcome[d] = np.where(inf[d] == _lib.INFO_LOSE, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS)
        tr = v & (outcome == 0) & (((max_steps > 0) & (steps >= max_steps)) | (steps >= cap))
        outcome[tr] = _lib.EVAL_TRUNCATED
        final[v] = nst[v]
        st = nst
        t += 1
        assert t < 20000, "the composition did not finish"
    env2.close()
    return dict(ret=ret, energy=energy, steps=steps, coll=coll, outcome=outcome, state=final, nsub=nsub,
                pos=np.stack(pos, 1), act=np.stack(acts, 1))


def _check_equal(rec, res, ref, v0, T):
    assert (rec["outcome"] == ref["outcome"]).all()
    assert (rec["steps"] == ref["steps"]).all()
    assert np.array_equal(rec["ret"], ref["ret"])
    assert np.array_equal(rec["energy"], ref["energy"])
    assert (rec["collisions"] == ref["coll"]).all()
    assert (rec["subgoals"] == ref["nsub"] - ref["state"][:, 11]).all()
    assert np.array_equal(rec["total_score"], ref["state"][:, 13])
    assert np.array_equal(rec["path_len"], ref["state"][:, 14])
    assert (rec["reach_goal"] == ref["state"][:, 15]).all()
    assert np.array_equal(rec["v0x"], v0[:, 0]) and np.array_equal(rec["v0y"], v0[:, 1])
    assert (rec["slot"] == 0).all() and (rec["reserved"] == 0).all()
    pos = res.positions.cpu().numpy()
    act = res.actions.cpu().numpy().astype(np.int64)
    k = min(T + 1, ref["pos"].shape[1])
    assert np.array_equal(pos[:, :k], ref["pos"][:, :k], equal_nan=True)
    assert np.array_equal(act[:, :k - 1], ref["act"][:, :k - 1])
    assert np.isnan(pos[:, k:]).all() and (act[:, k - 1:] == -1).all()


NETS = [("dqn", 11, False), ("dueling", 12, False), ("dqn", 13, True)]


@pytest.mark.parametrize("kind,seed,straight", NETS)
@pytest.mark.parametrize("obs", ["f16", "packed"])
def test_equals_the_composed_launches(obs, kind, seed, straight):
    scn = _scenarios()
    env = _env(64, obs)
    L = _learner(kind, seed, straight)
    n, T, cap = 1027, 600, 600                     # not a multiple of 64: the last wavefront has idle lanes feeding zero rows
    rows = np.arange(n) % scn[0].shape[0]
    v0 = _v0(n, seed)
    # one workgroup: every lane flies four or five episodes
    res = ev.evaluate_policy(env, L, n, scenarios=scn, v0=v0, max_steps=cap, trajectory_steps=T, max_workgroups=1)
    rec = res.host_records()
    ref = _compose(L, obs, scn, rows, v0, cap)
    _check_equal(rec, res, ref, v0, T)
    # every branch of the episode's end shows up in this set
    assert (rec["outcome"] == _lib.EVAL_SUCCESS).any() and (rec["outcome"] == _lib.EVAL_LOSE).any()
    assert rec["collisions"].sum() > 0
    assert rec["outcome"][0] == _lib.EVAL_SUCCESS and rec["steps"][0] == 1 and rec["reach_goal"][0] == 0    # empty list
    assert rec["outcome"][1] == _lib.EVAL_SUCCESS and rec["reach_goal"][1] == 1 and rec["subgoals"][1] == 2  # final sub-goal
    assert rec["outcome"][2] == _lib.EVAL_SUCCESS and rec["reach_goal"][2] == 1 and rec["subgoals"][2] == 0  # goal within 7 m
    env.close()


@pytest.mark.parametrize("obs", ["f16", "packed"])
def test_natural_completion_and_truncation(obs):
    scn = _scenarios()
    env = _env(64, obs)
    L = _learner("dqn", 21, True)
    for n, cap, first in ((256, 0, 3), (512, 40, 700)):
        rows = (first + np.arange(n)) % scn[0].shape[0]
        v0 = _v0(n, n)
        T = 64
        res = ev.evaluate_policy(env, L, n, scenarios=scn, first=first, v0=v0, max_steps=cap, trajectory_steps=T)
        rec = res.host_records()
        ref = _compose(L, obs, scn, rows, v0, cap)
        _check_equal(rec, res, ref, v0, T)
        if cap:
            assert (rec["outcome"] == _lib.EVAL_TRUNCATED).any()
        else:
            assert not (rec["outcome"] == _lib.EVAL_TRUNCATED).any()
    env.close()


@pytest.mark.parametrize("obs", ["f16", "packed"])
def test_placement_invariance_and_repeatability(obs):
    env = _env(64, obs)
    L = _learner("dueling", 31)
    n = 3000 + 37                                  # not a multiple of 64
    outs = []
    for mw in (1, 3, 0, 0):
        res = ev.evaluate_policy(env, L, n, seed=9, max_steps=300, max_workgroups=mw)
        outs.append(res.records.cpu().numpy().tobytes())
    assert outs[0] == outs[1] == outs[2] == outs[3]
    rec = np.frombuffer(outs[0], dtype=ev.RECORD_DTYPE)
    assert (rec["steps"] > 0).all()
    env.close()


def test_the_random_policy_is_the_f32_entrys():
    """At eps = 1 no action depends on the net: the eps stream, the default heading stream and everything around the forward
    are the existing kernel's, byte for byte."""
    env = _env(64, "packed")
    Lh = _learner("dqn", 51, mfma="f16")
    Lf = _learner("dqn", 51, mfma="f32")
    assert torch.equal(Lh.flat[0], Lf.flat[0]) and Lh.net.mfma_dtype == _lib.MFMA_F16 and Lf.net.mfma_dtype == _lib.MFMA_F32
    kw = dict(seed=3, eps=1.0, max_steps=200, first=5, trajectory_steps=200)
    rh = ev.evaluate_policy(env, Lh, 2048, **kw)
    rf = ev.evaluate_policy(env, Lf, 2048, **kw)
    assert rh.records.cpu().numpy().tobytes() == rf.records.cpu().numpy().tobytes()
    assert torch.equal(rh.actions, rf.actions)
    assert rh.positions.cpu().numpy().tobytes() == rf.positions.cpu().numpy().tobytes()
    rec = rh.host_records()
    assert (rec["steps"] > 0).all() and {0, 1, 2} <= set(np.unique(rh.actions.cpu().numpy()).tolist())
    env.close()


def _state_bytes(env):
    st, sub, al = env.get_state(0, env.N, want_sub=True)
    return st.tobytes() + sub.tobytes() + al.tobytes()


def test_refusals_leave_the_env_unchanged():
    env = _env(64, "packed")
    env.reset(seed=4)
    L = _learner("dqn", 61)
    before, tick = _state_bytes(env), env.lib.uavenv_tick(env._h)
    rec = torch.zeros((64, 64), dtype=torch.uint8, device=DEV)

    def args(**kw):
        a = _lib.UavEvalArgs()
        a.n, a.records = 64, rec.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(net=None, on=None, **kw):
        on = env if on is None else on
        return on.lib.uavenv_eval_episodes_f16(on._h, C.byref(net if net is not None else L.net), C.byref(args(**kw)), on._stream())

    assert call() == 0
    torch.cuda.synchronize()
    f32 = _lib.UavDqnNet.from_buffer_copy(L.net); f32.mfma_dtype = _lib.MFMA_F32
    assert call(net=f32) == _lib.EINVAL                                                  # an f32-MFMA net
    L5 = FusedDQNLearner(dict(PARAM, NetWork="VAnet2", output="5"), "dueling", device=DEV, mfma="f16")
    assert call(net=L5.net) == _lib.EINVAL                                               # 6 layer-2 outputs
    big = _lib.UavDqnNet.from_buffer_copy(L.net); big.n_actions = 4
    assert call(net=big) == _lib.EINVAL                                                  # not the env's n_actions
    wide = _lib.UavDqnNet.from_buffer_copy(L.net); wide.hid = 32
    assert call(net=wide) == _lib.EINVAL
    odd = _lib.UavDqnNet.from_buffer_copy(L.net); odd.local = L.net.local + 4
    assert call(net=odd) == _lib.EINVAL                                                  # a misaligned parameter block
    assert call(records=rec.data_ptr() + 4) == _lib.EINVAL
    assert call(records=None) == _lib.EINVAL
    assert call(n=0) == _lib.EINVAL
    assert call(first=-1) == _lib.EINVAL
    sg = torch.zeros((4, 6), dtype=torch.float64, device=DEV)
    sub = torch.zeros((4, env.K, 3), dtype=torch.float64, device=DEV)
    ns = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert call(start_goal=sg.data_ptr(), m=4) == _lib.EINVAL                            # only one of the three
    assert call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), m=4) == _lib.EINVAL        # two of the three
    assert call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), nsub=ns.data_ptr(), m=0) == _lib.EINVAL
    assert call(traj_steps=5) == _lib.EINVAL
    # the two existing entries still refuse the f16 net
    assert env.lib.uavenv_eval_episodes(env._h, C.byref(L.net), C.byref(args()), env._stream()) == _lib.EINVAL
    nets = (C.POINTER(_lib.UavDqnNet) * 1)(C.pointer(L.net))
    assert env.lib.uavenv_eval_episodes_slots(env._h, nets, 1, C.byref(args()), env._stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert _state_bytes(env) == before and env.lib.uavenv_tick(env._h) == tick
    env.close()
    # envs the entry does not take: f32 rows, APF, no bank -- each left as it was
    from dqn_based_uav_3d_path_planer_amd.env import VecPathPlanEnv
    others = [make_city26_env(64, obs_dtype=torch.float32), make_city26_env(64, obs_dtype="packed", apf_enabled=1),
              VecPathPlanEnv(64, load_city26()["buildings"], obs_dtype="packed")]
    for k, other in enumerate(others):
        if k < 2:
            other.reset(seed=4)
        before, tick = _state_bytes(other), other.lib.uavenv_tick(other._h)
        assert call(on=other) == _lib.EINVAL
        torch.cuda.synchronize()
        assert _state_bytes(other) == before and other.lib.uavenv_tick(other._h) == tick
        other.close()


def test_evaluate_policy_refuses_an_f16_learner_where_the_entry_would():
    L = _learner("dqn", 62)
    for other in (make_city26_env(64, obs_dtype=torch.float32), make_city26_env(64, obs_dtype="packed", apf_enabled=1)):
        with pytest.raises(ValueError, match="f16-MFMA"):
            ev.evaluate_policy(other, L, 64)
        other.close()
    env = _env(64, "packed")
    with pytest.raises(ValueError, match="f32-MFMA"):
        ev.evaluate_policy(env, [L], 64)
    assert L.evaluate(env, 64, max_steps=5).summary()["episodes"] == 64              # FusedDQNLearner.evaluate forwards
    env.close()


def test_training_is_the_same_with_evaluations_in_between():
    from dqn_based_uav_3d_path_planer_amd.loop import HotLoop
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing

    def run(with_eval):
        env = _env(4096, "f16")
        ring = DeviceReplayRing(env, 1 << 16, discrete=True)
        ring.reset(seed=1000)
        torch.manual_seed(42)
        L = FusedDQNLearner(dict(PARAM, NetWork="VAnet2"), "dueling", device=DEV, mfma="f16")
        loop = HotLoop(ring, L, 4096, seed=7, eps=0.1)
        for _ in range(4):
            loop.run(64)
            if with_eval:
                assert ev.evaluate_policy(env, L, 2048, seed=5, max_steps=200).summary()["episodes"] == 2048
        torch.cuda.synchronize()
        out = (L.flat.cpu().numpy().tobytes(), ring.obs.cpu().numpy().tobytes(), ring.action.cpu().numpy().tobytes(),
               ring.reward.cpu().numpy().tobytes(), ring.head, _state_bytes(env), env.lib.uavenv_tick(env._h))
        env.close()
        return out

    a, b = run(False), run(True)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x == y, ("parameters + Adam state", "ring rows", "ring actions", "ring rewards", "ring head", "env state", "tick")[k]

