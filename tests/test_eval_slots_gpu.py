"""Greedy DQN evaluation with one net per UAV slot, APF off and on (uavenv_eval_episodes_slots, k_eval_episodes_slots), against
  * the composition of the launches that existed before it: set_state -> observe -> per UAV slot FusedDQNLearner.act (uavenv_dqn_act)
    on the slot's rows -> env.step(skip_done) in its default form (k_apf_adjust + k_step on an APF env), accumulated on the host;
  * the old entry (uavenv_eval_episodes) where both apply;
  * the C oracle (oracle/uav_oracle.c) for the endings.
Everything is equality: each comparison is between two runs of the same device functions on the same operands."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev
from dqn_based_uav_3d_path_planer_amd.data import load_city26
from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
from test_eval_sac_gpu import _env, _hand_rows, _oracle_fly_straight, _scenarios, _state_bytes, _v0

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PARAM = {"w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99", "Update_loop": "3"}
NETS = ["qnet", "vanet", "straight"]
_LS = {}


def _learner(kind, seed):
    """kind: "qnet" (random Qnet2), "vanet" (random VAnet2, dueling), "straight" (Qnet2 whose fc2 bias favours action 1 = steer 0),
    "zero" (Qnet2 with fc2 = 0 and that bias: Q = (0, 5, 0) whatever the state -- steer exactly 0 on every step)."""
    torch.manual_seed(seed)
    dueling = kind == "vanet"
    L = FusedDQNLearner(dict(PARAM, NetWork="VAnet2" if dueling else "Qnet2"), "dueling" if dueling else "dqn", device=DEV)
    if kind in ("straight", "zero"):
        with torch.no_grad():
            if kind == "zero":
                L.q_local.fc2.weight.zero_()
            L.q_local.fc2.bias.copy_(torch.tensor([0.0, 5.0, 0.0], device=DEV))
    return L


def _learners(kind, U):
    """U different nets of one kind (cached)."""
    if (kind, U) not in _LS:
        _LS[(kind, U)] = [_learner(kind, 1000 + 100 * U + 10 * j + len(kind)) for j in range(U)]
    return _LS[(kind, U)]


def _compose(Ls, U, apf, scn, rows, v0, max_steps):
    """The same episodes through the launches of the parent commit: agent i of a fresh env (uav_per_env = U) is episode i, UAV slot
    i mod U, acted for by Ls[i mod U] (greedy: eps = 0)."""
    n = len(rows)
    assert n % U == 0
    sg, sub, ns = (x.cpu().numpy() for x in scn)
    env2 = _env(n // U, apf, U)
    kin = np.concatenate([sg[rows, :3], v0, sg[rows, 3:]], 1)
    nsub = ns[rows]
    env2.set_state(0, kin, np.zeros(n, np.int32), nsub, sub[rows], alias=(nsub >= 2).astype(np.int32))
    obs = env2.observe()
    out = env2.alloc_out(want_energy=True)
    act = torch.zeros(n, dtype=torch.int32, device=DEV)
    tmp = torch.zeros(n // U, dtype=torch.int32, device=DEV)
    st = env2.get_state(0, n)
    final = st.copy()
    ret, energy = np.zeros(n), np.zeros(n)
    steps, coll = np.zeros(n, np.int64), np.zeros(n, np.int64)
    outcome = np.zeros(n, np.int64)
    pos, acts = [st[:, :3].copy()], []
    cap = nsub.astype(np.int64) * env2.cfg.max_step + 1
    t = 0
    while (outcome == 0).any():
        for j in range(U):
            Ls[j].act(obs[j::U].contiguous(), 0.0, 5, t, index_out=tmp)
            act[j::U] = tmp
        env2.step(act, out, skip_done=True)
        obs = out.obs
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


def _check_equal(rec, res, ref, v0, T, U):
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
    assert (rec["slot"] == np.arange(len(rec)) % U).all() and (rec["reserved"] == 0).all()
    pos = res.positions.cpu().numpy()
    act = res.actions.cpu().numpy().astype(np.int64)
    k = min(T + 1, ref["pos"].shape[1])
    assert np.array_equal(pos[:, :k], ref["pos"][:, :k], equal_nan=True)
    assert np.array_equal(act[:, :k - 1], ref["act"][:, :k - 1])
    assert np.isnan(pos[:, k:]).all() and (act[:, k - 1:] == -1).all()


@pytest.mark.parametrize("kind", NETS)
@pytest.mark.parametrize("U", [1, 4])
@pytest.mark.parametrize("apf", [0, 1])
def test_equals_the_composed_launches(apf, U, kind):
    scn = _scenarios()
    Ls = _learners(kind, U)
    env = _env(64, apf, U)
    n, T, cap = 2048, 600, 600
    m = scn[0].shape[0]
    rows = np.arange(n) % m
    v0 = _v0(n, 1000 * apf + 100 * U + len(kind))
    # one workgroup per net: every lane flies 2 (U = 4) or 8 (U = 1) episodes
    res = ev.evaluate_policy(env, Ls, n, scenarios=scn, v0=v0, max_steps=cap, trajectory_steps=T, max_workgroups=1)
    rec = res.host_records()
    ref = _compose(Ls, U, apf, scn, rows, v0, cap)
    _check_equal(rec, res, ref, v0, T, U)
    assert (rec["steps"] > 0).all() and rec["collisions"].sum() > 0
    if U > 1 and kind != "straight":              # the nets differ: slot 0's net in every slot flies something else
        other = ev.evaluate_policy(env, [Ls[0]] * U, n, scenarios=scn, v0=v0, max_steps=cap, max_workgroups=1).host_records()
        assert other[0::U].tobytes() == rec[0::U].tobytes() and other[1::U].tobytes() != rec[1::U].tobytes()
    env.close()


@pytest.mark.parametrize("eps", [0.0, 0.3])
def test_new_entry_equals_the_old_entry_for_one_net(eps):
    env = _env(64, 0, 1)
    for kind in ("qnet", "vanet"):
        L = _learner(kind, 21)
        n = 3000 + 37
        kw = dict(seed=9, eps=eps, first=5, max_steps=300, trajectory_steps=8)   # the bank, default headings (no v0)
        new = ev.evaluate_policy(env, [L], n, **kw)
        old = ev.evaluate_policy(env, L, n, **kw)
        assert new.records.cpu().numpy().tobytes() == old.records.cpu().numpy().tobytes()
        assert new.positions.cpu().numpy().tobytes() == old.positions.cpu().numpy().tobytes()
        assert new.actions.cpu().numpy().tobytes() == old.actions.cpu().numpy().tobytes()
        rec = old.host_records()
        assert (rec["steps"] > 0).all()
        if eps > 0:                                # the draws reached the actions
            greedy = ev.evaluate_policy(env, [L], n, **dict(kw, eps=0.0)).host_records()
            assert greedy.tobytes() != rec.tobytes()
    env.close()


@pytest.mark.parametrize("eps", [0.0, 0.3])
def test_one_launch_equals_the_old_entry_slot_by_slot(eps):
    U = 4
    env = _env(64, 0, U)
    Ls = _learners("qnet", U)
    n = 512 * U
    kw = dict(seed=11, eps=eps, first=5, max_steps=300)
    one = ev.evaluate_policy(env, Ls, n, **kw).host_records()
    for j in range(U):
        old = ev.evaluate_policy(env, Ls[j], n, **kw).host_records()
        assert one[j::U].tobytes() == old[j::U].tobytes(), j
    assert (one["slot"] == np.arange(n) % U).all() and (one["steps"] > 0).all()
    env.close()


@pytest.mark.parametrize("apf", [0, 1])
def test_every_ending_is_exercised(apf):
    """The hand-built rows and the packaged bank under the fly-straight net (Q = (0, 5, 0): steer exactly 0), cap 200.  The C oracle
    alone, on the CPU, says how each episode ends -- success by empty list (row 0), by the final sub-goal (row 1), by the goal within
    7 m (row 2), lose, truncation, collisions, with APF off and on (APF shifts the sub-goals: the hand-built rows are re-checked
    there) -- and the kernel's records must show those endings."""
    c = load_city26()
    a, b, d = _hand_rows(48)
    sg = np.concatenate([a, c["start_goal"]]); sub = np.concatenate([b, c["sub_goals"]])
    ns = np.concatenate([d, c["n_sub"]]).astype(np.int32)
    n, cap = len(sg), 200
    rows = np.arange(n)
    v0 = _v0(n, 7)
    o, s, cl, rg, popped = _oracle_fly_straight(apf, sg, sub, ns, rows, v0, cap, int(c["max_step"]))
    # the oracle alone shows every ending
    assert o[0] == _lib.EVAL_SUCCESS and s[0] == 1 and rg[0] == 0 and popped[0] == 0           # empty list
    assert o[1] == _lib.EVAL_SUCCESS and rg[1] == 1 and popped[1] == 2                          # final sub-goal
    assert o[2] == _lib.EVAL_SUCCESS and rg[2] == 1 and popped[2] == 0                          # goal within 7 m
    assert (o == _lib.EVAL_LOSE).sum() > 100 and (o == _lib.EVAL_TRUNCATED).sum() > 100 and (cl > 0).sum() > 100
    assert (s[o == _lib.EVAL_TRUNCATED] == cap).all()
    env = _env(64, apf)
    L = _learner("zero", 5)
    scn = (torch.tensor(sg, device=DEV), torch.tensor(sub, device=DEV), torch.tensor(ns, device=DEV))
    res = ev.evaluate_policy(env, [L], n, scenarios=scn, v0=v0, max_steps=cap, trajectory_steps=4)
    rec = res.host_records()
    assert (res.actions.cpu().numpy()[rec["steps"] >= 4] == 1).all()
    assert (rec["outcome"] == o).all() and (rec["steps"] == s).all()
    assert (rec["reach_goal"] == rg).all() and (rec["subgoals"] == popped).all() and (rec["collisions"] == cl).all()
    env.close()


@pytest.mark.parametrize("apf", [0, 1])
def test_placement_invariance_and_repeatability(apf):
    U = 4
    env = _env(64, apf, U)
    Ls = _learners("vanet", U)
    n = 3000 + 37                                  # neither a multiple of 64 nor of U
    outs = []
    for mw in (1, 3, 0, 0):                        # (1 -> 3 -> automatic: every call has more resident lanes than the one before)
        res = ev.evaluate_policy(env, Ls, n, seed=9, max_steps=300, max_workgroups=mw)
        outs.append(res.records.cpu().numpy().tobytes())
    assert outs[0] == outs[1] == outs[2] == outs[3]
    rec = np.frombuffer(outs[0], dtype=ev.RECORD_DTYPE)
    assert (rec["steps"] > 0).all() and (rec["slot"] == np.arange(n) % U).all()
    env.close()


@pytest.mark.parametrize("apf", [0, 1])
def test_invalid_rows_are_recorded_not_flown(apf):
    env = _env(64, apf)
    L = _learner("qnet", 41)
    sg, sub, ns = (x.clone() for x in _scenarios())
    ns[5] = -3
    ns[6] = env.K + 1
    rec = ev.evaluate_policy(env, [L], 16, scenarios=(sg, sub, ns), v0=_v0(16, 1)).host_records()
    assert (rec["outcome"][[5, 6]] == _lib.EVAL_INVALID).all() and (rec["steps"][[5, 6]] == 0).all()
    assert ((rec["outcome"] != _lib.EVAL_INVALID).sum() == 14) and (rec["steps"][rec["outcome"] != _lib.EVAL_INVALID] > 0).all()
    env.close()


def _nets(Ls):
    return [C.pointer(L.net) for L in Ls]


@pytest.mark.parametrize("apf", [0, 1])
def test_the_env_is_left_alone_by_evaluations_and_refusals(apf):
    U = 4
    env = _env(16, apf, U)
    env.reset(seed=4)
    act = torch.zeros(env.N, dtype=torch.float32, device=DEV)
    for _ in range(3):                             # (an APF env: the sub-goal lists have moved by now)
        env.step(act, skip_done=True)
    Ls = _learners("qnet", U)
    before, tick = _state_bytes(env), env.lib.uavenv_tick(env._h)
    rec = torch.zeros((64, 64), dtype=torch.uint8, device=DEV)
    lib = env.lib
    good = _nets(Ls)

    def call(nets=None, n_nets=None, h=None, **kw):
        a = _lib.UavEvalArgs()
        a.n, a.records = 64, rec.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        nets = good if nets is None else nets
        arr = (C.POINTER(_lib.UavDqnNet) * max(len(nets), 1))(*nets)
        return lib.uavenv_eval_episodes_slots(env._h if h is None else h, arr, len(nets) if n_nets is None else n_nets, C.byref(a),
                                              env._stream())

    def changed():
        torch.cuda.synchronize()
        return _state_bytes(env) != before or env.lib.uavenv_tick(env._h) != tick

    assert call() == 0 and call(nets=good[:1]) == 0 and call(eps=0.3, traj_steps=0) == 0
    assert ev.evaluate_policy(env, Ls, 512, max_steps=100).summary()["episodes"] == 512
    assert Ls[0].evaluate(env, 256, max_steps=50).summary()["episodes"] == 256
    assert not changed()
    f16 = _lib.UavDqnNet.from_buffer_copy(Ls[1].net); f16.mfma_dtype = _lib.MFMA_F16
    L5 = FusedDQNLearner(dict(PARAM, NetWork="VAnet2", output="5"), "dueling", device=DEV)
    duel = _learner("vanet", 3)
    off = _lib.UavDqnNet.from_buffer_copy(Ls[2].net); off.local = Ls[2].net.local + 4
    four = _lib.UavDqnNet.from_buffer_copy(Ls[1].net); four.n_actions = 4
    narrow = _lib.UavDqnNet.from_buffer_copy(Ls[1].net); narrow.hid = 32
    nul = _lib.UavDqnNet.from_buffer_copy(Ls[1].net); nul.local = None
    tp = torch.zeros((64, 6, 3), dtype=torch.float64, device=DEV)
    ta = torch.zeros((64, 5), dtype=torch.int8, device=DEV)
    sg = torch.zeros((4, 6), dtype=torch.float64, device=DEV)
    sub = torch.zeros((4, env.K, 3), dtype=torch.float64, device=DEV)
    ns = torch.zeros(4, dtype=torch.int32, device=DEV)
    v0 = torch.zeros((64, 2), dtype=torch.float64, device=DEV)
    swap = lambda k, net: good[:k] + [C.pointer(net)] + good[k + 1:]   # noqa: E731
    refusals = [
        lambda: call(n_nets=0), lambda: call(n_nets=-1), lambda: call(nets=good[:2]), lambda: call(nets=good[:3]),   # not in {1, U}
        lambda: call(nets=good + good + good[:1]),                                                                  # 9
        lambda: call(nets=good + good),                                                                             # 8 on a U = 4 env
        lambda: call(nets=[good[0], C.POINTER(_lib.UavDqnNet)(), good[2], good[3]]),                                # a null net pointer
        lambda: call(nets=swap(1, f16)), lambda: call(nets=[C.pointer(f16)]),                                       # an f16-MFMA net
        lambda: call(nets=swap(3, L5.net)), lambda: call(nets=[C.pointer(L5.net)]),                                 # 6 layer-2 outputs
        lambda: call(nets=swap(2, duel.net)), lambda: call(nets=swap(0, duel.net)),                                 # differ in dueling
        lambda: call(nets=swap(2, off)), lambda: call(nets=[C.pointer(off)]),                                       # a misaligned local
        lambda: call(nets=swap(1, four)), lambda: call(nets=swap(1, narrow)), lambda: call(nets=swap(1, nul)),
        lambda: call(n=0), lambda: call(n=-5), lambda: call(first=-1),
        lambda: call(records=rec.data_ptr() + 8), lambda: call(records=None),                                       # records misaligned
        lambda: call(start_goal=sg.data_ptr(), m=4),                                                                # one of the three
        lambda: call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), m=4),
        lambda: call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), nsub=ns.data_ptr(), m=0),
        lambda: call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), nsub=ns.data_ptr() + 2, m=4),
        lambda: call(traj_steps=5), lambda: call(traj_steps=-1),                                                    # without pointers
        lambda: call(traj_steps=5, traj_pos=tp.data_ptr()), lambda: call(traj_steps=5, traj_act=ta.data_ptr()),
        lambda: call(traj_steps=5, traj_pos=tp.data_ptr() + 4, traj_act=ta.data_ptr()),
        lambda: call(v0=v0.data_ptr() + 4), lambda: call(max_steps=-1), lambda: call(max_workgroups=-1),
        lambda: call(n=2 ** 31 - 100),                                                                              # n + lanes
    ]
    for k, f in enumerate(refusals):
        assert f() == _lib.EINVAL, k
        assert not changed(), k
    a = _lib.UavEvalArgs(); a.n, a.records = 64, rec.data_ptr()
    assert lib.uavenv_eval_episodes_slots(env._h, None, 1, C.byref(a), env._stream()) == _lib.EINVAL                # nets NULL
    assert lib.uavenv_eval_episodes_slots(env._h, (C.POINTER(_lib.UavDqnNet) * 1)(good[0]), 1, None, env._stream()) == _lib.EINVAL
    assert call() == 0 and not changed()
    # no world: an env that never saw uavenv_set_buildings; no scenarios: an env without a bank
    h = C.c_void_p()
    _lib.check(lib.uavenv_create(C.byref(env.cfg), C.byref(h)), "uavenv_create")
    assert call(h=h) == _lib.EINVAL
    lib.uavenv_destroy(h)
    env.close()
    from dqn_based_uav_3d_path_planer_amd.env import VecPathPlanEnv
    nob = VecPathPlanEnv(16, load_city26()["buildings"], obs_dtype="packed", uav_per_env=U, apf_enabled=apf)
    arr = (C.POINTER(_lib.UavDqnNet) * U)(*good)
    assert nob.lib.uavenv_eval_episodes_slots(nob._h, arr, U, C.byref(a), nob._stream()) == _lib.EINVAL
    nob.close()
    if apf:                                        # the old entry still refuses an APF env
        e2 = _env(16, 1)
        assert e2.lib.uavenv_eval_episodes(e2._h, C.byref(Ls[0].net), C.byref(a), e2._stream()) == _lib.EINVAL
        e2.close()


def test_training_on_an_apf_env_is_the_same_with_an_evaluation_in_between():
    from dqn_based_uav_3d_path_planer_amd.loop import HotLoop
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing

    def run(with_eval):
        env = _env(1024, 1)
        ring = DeviceReplayRing(env, 1 << 15, discrete=True)
        ring.reset(seed=1000)
        torch.manual_seed(42)
        L = FusedDQNLearner(dict(PARAM, NetWork="Qnet2"), "dqn", device=DEV)
        loop = HotLoop(ring, L, 256, seed=7, eps=0.1)
        loop.run(12)
        if with_eval:
            assert ev.evaluate_policy(env, L, 1024, seed=5, max_steps=200).summary()["episodes"] == 1024
            assert L.evaluate(env, 256, max_steps=50, eps=0.2).summary()["episodes"] == 256
        loop.run(12)
        torch.cuda.synchronize()
        out = (L.flat.cpu().numpy().tobytes(), ring.obs.cpu().numpy().tobytes(), ring.action.cpu().numpy().tobytes(),
               ring.reward.cpu().numpy().tobytes(), _state_bytes(env), env.lib.uavenv_tick(env._h))
        loop.close()
        env.close()
        return out

    assert run(False) == run(True)


def test_the_apf_workspace_is_shared_with_the_sac_entry():
    from dqn_based_uav_3d_path_planer_amd.sac import FusedSACLearner
    from test_eval_sac_gpu import PARAM as SAC_PARAM
    U = 4
    env = _env(64, 1, U)
    Ls = _learners("qnet", U)
    torch.manual_seed(77)
    Ss = [FusedSACLearner(SAC_PARAM, DEV) for _ in range(U)]
    n = 3000 + 37
    kw = dict(seed=3, max_steps=200, trajectory_steps=4)

    def dqn(mw):
        r = ev.evaluate_policy(env, Ls, n, max_workgroups=mw, **kw)
        return r.records.cpu().numpy().tobytes() + r.positions.cpu().numpy().tobytes() + r.actions.cpu().numpy().tobytes()

    def sac():
        r = ev.evaluate_sac_policy(env, Ss, n, mode="mean", **kw)
        return r.records.cpu().numpy().tobytes() + r.positions.cpu().numpy().tobytes()

    d1 = dqn(1)                                    # 1 024 lists
    s1 = sac()                                     # grows the workspace
    d0 = dqn(0)                                    # the default grid on the grown workspace
    d1b = dqn(1)
    assert d1b == d1 and d0 == d1
    assert sac() == s1 and dqn(0) == d0
    env.close()


@pytest.mark.parametrize("apf", [0, 1])
@pytest.mark.parametrize("trainer", ["DQN", "DuelingDQN"])
def test_plugin_evaluate_policy(apf, trainer, tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver
    monkeypatch.chdir(tmp_path)                    # (the config's paths are relative to the working directory)
    xml = driver.make_config_dir(str(tmp_path), trainer, num_envs=64, num_uav=4)
    if apf:
        uav_xml = tmp_path / "config" / "UAV.xml"
        uav_xml.write_text(re.sub(r"<APF_Enabled>0</APF_Enabled>", "<APF_Enabled>1</APF_Enabled>", uav_xml.read_text()))
    torch.manual_seed(0)
    env = driver.simulator(xml).env
    learners = [u.Trainer.learner for u in env.Agents]
    assert env.backend.cfg.apf_enabled == apf and len({id(L) for L in learners}) == 4
    assert all(isinstance(L, FusedDQNLearner) for L in learners)
    before = _state_bytes(env.backend)
    calls = []
    real = ev.evaluate_policy

    def counted(*a, **kw):
        calls.append(a[1])
        return real(*a, **kw)

    monkeypatch.setattr(ev, "evaluate_policy", counted)
    summ = env.evaluate_policy(n_episodes=256, seed=1, max_steps=300)
    monkeypatch.setattr(ev, "evaluate_policy", real)
    assert len(calls) == 1 and isinstance(calls[0], (list, tuple)) and [id(L) for L in calls[0]] == [id(L) for L in learners]
    assert len(summ) == 4
    scn = ev.held_out_scenarios(env.backend, 256, seed=0x7E57_0000 + 1)
    scn_u, v0 = ev.slot_scenarios(scn, 4, float(env.backend.cfg.max_v), 1)
    rec = ev.evaluate_policy(env.backend, learners, 256 * 4, scenarios=scn_u, v0=v0, seed=1, max_steps=300).host_records()
    for j in range(4):
        assert summ[j] == ev.summarize(rec[j::4]), j
        assert summ[j]["episodes"] == 256 and summ[j]["invalid"] == 0
    assert len({s["mean_energy"] for s in summ}) == 4
    torch.cuda.synchronize()
    assert _state_bytes(env.backend) == before
    # all slots sharing one learner: one call with that learner
    keep = [u.Trainer for u in env.Agents]
    for u in env.Agents:
        u.Trainer = keep[0]
    calls.clear()
    monkeypatch.setattr(ev, "evaluate_policy", counted)
    shared = env.evaluate_policy(n_episodes=256, seed=1, max_steps=300)
    monkeypatch.setattr(ev, "evaluate_policy", real)
    for u, t in zip(env.Agents, keep):
        u.Trainer = t
    assert len(calls) == 1 and calls[0] is learners[0]
    assert shared[0] == summ[0] and len(shared) == 4
