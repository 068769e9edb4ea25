"""SAC policy evaluation on the device (uavenv_eval_episodes_sac, k_eval_episodes_sac), APF off and on, against
  * the composition of the launches that existed before it: set_state -> observe -> FusedSACLearner.act_rows per UAV slot ->
    env.step(skip_done) in its default form (k_apf_adjust + k_step on an APF env), accumulated on the host -- bit for bit;
  * the C oracle (oracle/uav_oracle.c), which shares no code with the device step.
The kernel under test is never its own yardstick."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd import evaluate as ev
from dqn_based_uav_3d_path_planer_amd.data import load_city26, make_city26_env
from dqn_based_uav_3d_path_planer_amd.sac import FusedSACLearner

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PARAM = {"actor": {"NetWork": "PolicyNetContinuous_SAC", "w": "100", "action_bound": "1", "hiden_dim": "64", "output": "2", "lr": "0.0001"},
         "critic": {"NetWork": "QValueNetContinuous_SAC", "w": "100", "hiden_dim": "64", "action_dim": "2", "lr": "0.001"},
         "SAC_param": {"IS_Continuous": "1", "alpha_lr": "0.0001", "target_entropy": "1", "gamma": "0.99", "tau": "0.05"}}


def _velocities():
    """tests/golden/apf_episodes.npz: every third building static, the others moving."""
    return load_golden("apf_episodes.npz")["velocities"]


def _env(n_envs, apf, U=1):
    kw = dict(apf_enabled=1, velocities=_velocities()) if apf else {}
    return make_city26_env(n_envs, obs_dtype="packed", uav_per_env=U, **kw)


def _train(L, seed, updates=300):
    """A few hundred fused updates on synthetic batches: rows of a reset env, random actions, rewards, done flags and pairs."""
    env = make_city26_env(4096, obs_dtype="packed")
    obs = env.reset(seed=seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    n, B = env.N, 256
    a0 = torch.rand(n, device=DEV, generator=g) * 2 - 1
    a1 = torch.rand(n, device=DEV, generator=g) * 2 - 1
    rew = torch.randn(n, device=DEV, generator=g)
    done = (torch.rand(n, device=DEV, generator=g) < 0.1).to(torch.uint8)
    for _ in range(updates):
        idx = torch.randint(0, n, (2, B), device=DEV, generator=g, dtype=torch.int32)
        b = L.make_batch(obs, a0, a1, rew, done, idx_s=idx[0].contiguous(), idx_n=idx[1].contiguous())
        L.learn(b, noise=(torch.randn((B, 2), device=DEV, generator=g), torch.randn((B, 2), device=DEV, generator=g)))
    torch.cuda.synchronize()
    assert torch.isfinite(L._blocks).all()
    env.close()


def _sac(kind, seed):
    """kind: "init" (random init), "trained" (random init + 300 fused updates), "straight" (fc_mu zeroed: the mean action is 0)."""
    torch.manual_seed(seed)
    L = FusedSACLearner(PARAM, DEV)
    if kind == "trained":
        _train(L, seed)
    elif kind == "straight":
        with torch.no_grad():
            L.actor.fc_mu.weight.zero_()
            L.actor.fc_mu.bias.zero_()
    return L


def _hand_rows(K):
    """tests/test_eval_gpu.py::_hand_rows: an empty list, the final sub-goal within reach, the goal within 7 m of a UAV that is
    still >= 7 m from its sub-goal (z = 90: above every roof)."""
    sg = np.zeros((3, 6)); sub = np.zeros((3, K, 3)); ns = np.zeros(3, np.int32)
    sg[0] = [100, 100, 90, 300, 300, 90]; ns[0] = 0
    sg[1] = [100, 100, 90, 300, 300, 90]; sub[1, 0] = [100, 100, 90]; sub[1, 1] = [101, 100, 90]; ns[1] = 2
    sg[2] = [244, 250, 90, 250, 250, 90]; sub[2, 0] = [253, 250, 90]; ns[2] = 1
    return sg, sub, ns


_SCN = {}


def _scenarios():
    """hand-built rows + the packaged bank + held-out planner rows (device tensors; the same set for every env)."""
    if "s" not in _SCN:
        env = make_city26_env(64, obs_dtype="packed")
        sg0, sub0, ns0 = env.bank_read(0, 1024)
        hsg, hsub, hns = ev.held_out_scenarios(env, 1024, seed=0x5AC1)
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


def _compose(Ls, U, apf, scn, rows, v0, max_steps, noise):
    """The same episodes through the launches of the parent commit: agent i of a fresh env (uav_per_env = U) is episode i, UAV
    slot i mod U, acted for by Ls[i mod len(Ls)].  noise: [n, steps, 2] f32 or None (zeros)."""
    n = len(rows)
    assert n % U == 0
    sg, sub, ns = (x.cpu().numpy() for x in scn)
    env2 = _env(n // U, apf, U)
    kin = np.concatenate([sg[rows, :3], v0, sg[rows, 3:]], 1)
    nsub = ns[rows]
    env2.set_state(0, kin, np.zeros(n, np.int32), nsub, sub[rows], alias=(nsub >= 2).astype(np.int32))
    obs = env2.observe()
    out = env2.alloc_out(want_energy=True)
    act0 = torch.zeros(n, dtype=torch.float32, device=DEV)
    act1 = torch.zeros(n, dtype=torch.float32, device=DEV)
    zero = torch.zeros((n, 2), dtype=torch.float32, device=DEV)
    st = env2.get_state(0, n)
    final = st.copy()
    ret, energy = np.zeros(n), np.zeros(n)
    steps, coll = np.zeros(n, np.int64), np.zeros(n, np.int64)
    outcome = np.zeros(n, np.int64)
    pos, acts = [st[:, :3].copy()], []
    cap = nsub.astype(np.int64) * env2.cfg.max_step + 1
    t = 0
    while (outcome == 0).any():
        z = zero if noise is None else noise[:, t]
        for j in range(U):
            Ls[j % len(Ls)].act_rows(obs, j, U, n // U, act0, act1, eps=z[j::U].contiguous())
        env2.step(act0, out, skip_done=True)
        obs = out.obs
        nst = env2.get_state(0, n)
        v = (out.valid.cpu().numpy() == 1) & (outcome == 0)        # (a truncated agent flies on here; its episode has ended)
        ret[v] += out.reward.cpu().numpy()[v]
        energy[v] += out.energy.cpu().numpy()[v]
        steps[v] += 1
        same = (nst[:, 0] == st[:, 0]) & (nst[:, 1] == st[:, 1]) & (nst[:, 2] == st[:, 2])
        coll[v & same & (st[:, 11] > 0)] += 1                       # a moved step whose position did not change
        a = np.stack([act0.cpu().numpy(), act1.cpu().numpy()], 1)
        a[~v] = np.nan
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
    act = res.actions.cpu().numpy()
    k = min(T + 1, ref["pos"].shape[1])
    assert np.array_equal(pos[:, :k], ref["pos"][:, :k], equal_nan=True)
    assert np.array_equal(act[:, :k - 1, 0], ref["act"][:, :k - 1, 0], equal_nan=True)
    assert np.array_equal(act[:, :k - 1, 1], ref["act"][:, :k - 1, 1], equal_nan=True)
    assert np.isnan(pos[:, k:]).all() and np.isnan(act[:, k - 1:]).all()


_ACTORS = {}


def _actors(kind, U):
    """U different actors of one kind (cached: the fused updates of "trained" are the expensive part)."""
    key = (kind, U)
    if key not in _ACTORS:
        _ACTORS[key] = [_sac(kind, 100 * U + 10 * j + len(kind)) for j in range(U)]
    return _ACTORS[key]


@pytest.mark.parametrize("mode", ["mean", "sample"])
@pytest.mark.parametrize("kind", ["init", "trained", "straight"])
@pytest.mark.parametrize("U", [1, 4])
@pytest.mark.parametrize("apf", [0, 1])
def test_equals_the_composed_launches(apf, U, kind, mode):
    scn = _scenarios()
    Ls = _actors(kind, U)
    env = _env(64, apf, U)
    n, T, cap = 4096, 600, 600
    m = scn[0].shape[0]
    first = 0
    rows = (first + np.arange(n)) % m
    seed = 1000 * apf + 100 * U + len(kind) + (7 if mode == "sample" else 0)
    v0 = _v0(n, seed)
    res = ev.evaluate_sac_policy(env, Ls if U > 1 else Ls[0], n, scenarios=scn, first=first, v0=v0, seed=seed, mode=mode,
                                 max_steps=cap, trajectory_steps=T)
    rec = res.host_records()
    noise = ev.sac_noise(n, cap, seed, DEV) if mode == "sample" else None
    ref = _compose(Ls, U, apf, scn, rows, v0, cap, noise)
    _check_equal(rec, res, ref, v0, T, U)
    assert (rec["steps"] > 0).all() and rec["collisions"].sum() > 0
    if mode == "sample":                           # the noise reached the actions: the other mode flies something else
        other = ev.evaluate_sac_policy(env, Ls if U > 1 else Ls[0], n, scenarios=scn, first=first, v0=v0, seed=seed, mode="mean",
                                       max_steps=cap).host_records()
        assert not np.array_equal(other["ret"], rec["ret"])
    env.close()


def _oracle_batch(apf, sg, sub, ns, rows, v0):
    from oracle import pyoracle as po
    c = load_city26()
    world = po.OracleWorld(c["buildings"], c["len"], c["width"], c["h"], velocities=_velocities() if apf else None)
    params = dict(max_v=float(c["max_v"]), steering_angle=float(c["steering_angle"]), max_step=int(c["max_step"]),
                  apf_enabled=int(apf))
    n = len(rows)
    batch = po.OracleBatch(world, params, n)
    for i in range(n):
        u = batch.arr[i]
        r = rows[i]
        u.px, u.py, u.pz = (float(x) for x in sg[r, :3])
        u.gx, u.gy, u.gz = (float(x) for x in sg[r, 3:])
        u.vx, u.vy, u.vz = float(v0[i, 0]), float(v0[i, 1]), 0.0
        u.V = batch.lib.orc_calc_v(C.byref(u))
        u.step = u.done = u.reach_goal = u.error = 0
        u.score = u.total_score = u.path_len = 0.0
        u.n_sub = int(ns[r])
        u.sub0_alias = 1 if int(ns[r]) >= 2 else 0
        if ns[r] > 0:
            C.memmove(C.addressof(u.sub), np.ascontiguousarray(sub[r, :ns[r]]).ctypes.data, int(ns[r]) * 24)
    return batch


def _oracle_fly_straight(apf, sg, sub, ns, rows, v0, cap, max_step):
    """Whole episodes under steer 0 by the C oracle alone -> outcome, steps, collisions, reach_goal, sub-goals popped."""
    n = len(rows)
    batch = _oracle_batch(apf, sg, sub, ns, rows, v0)
    steps, coll, outcome = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    capn = ns[rows].astype(np.int64) * max_step + 1
    while (outcome == 0).any():
        p0 = np.stack([batch.view["px"], batch.view["py"], batch.view["pz"]], 1).copy()
        left = batch.view["n_sub"].copy()
        _, _, info, _ = batch.step(np.zeros(n), want_obs=False)
        live = outcome == 0
        steps[live] += 1
        p1 = np.stack([batch.view["px"], batch.view["py"], batch.view["pz"]], 1)
        coll[live & (p0 == p1).all(1) & (left > 0)] += 1
        dn = live & (batch.view["done"] == 1)
        outcome[dn] = np.where(info[dn] == 2, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS)
        tr = live & (outcome == 0) & ((steps >= cap) | (steps >= capn))
        outcome[tr] = _lib.EVAL_TRUNCATED
    return outcome, steps, coll, batch.view["reach_goal"].copy(), ns[rows] - batch.view["n_sub"]


@pytest.mark.parametrize("apf", [0, 1])
def test_every_ending_is_exercised(apf):
    """The hand-built rows and the packaged bank under the fly-straight policy (mean mode: steer exactly 0), cap 200.  The C
    oracle alone, on the CPU, says how each episode ends -- success by empty list (row 0), by the final sub-goal (row 1), by the
    goal within 7 m (row 2), lose, truncation, collisions, with APF off and on (APF shifts the sub-goals, so the hand-built rows
    are re-checked there) -- and the kernel's records must show those endings."""
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
    L = _sac("straight", 5)
    scn = (torch.tensor(sg, device=DEV), torch.tensor(sub, device=DEV), torch.tensor(ns, device=DEV))
    rec = ev.evaluate_sac_policy(env, L, n, scenarios=scn, v0=v0, mode="mean", max_steps=cap).host_records()
    assert (rec["outcome"] == o).all() and (rec["steps"] == s).all()
    assert (rec["reach_goal"] == rg).all() and (rec["subgoals"] == popped).all() and (rec["collisions"] == cl).all()
    env.close()


@pytest.mark.parametrize("kind,mode", [("straight", "mean"), ("init", "sample"), ("trained", "sample")])
def test_oracle_replay_of_recorded_actions_with_apf(kind, mode):
    """APF on: the recorded act0 of 512 episodes replayed through the C oracle (APF, the same velocities) from the same resets.
    Outcome and step count exactly, no episode left out; positions <= 1e-8 and |return error| <= 1e-9 x steps -- the bars of
    tests/test_env_parity_gpu.py::test_apf_episodes_from_reference_resets_without_resync (state 1e-8, reward 1e-9 per step)."""
    env = _env(64, 1)
    scn = _scenarios()
    L = _sac(kind, 71)
    n, T = 512, 600
    v0 = _v0(n, 71)
    res = ev.evaluate_sac_policy(env, L, n, scenarios=scn, v0=v0, seed=71, mode=mode, max_steps=T, trajectory_steps=T)
    rec = res.host_records()
    pos = res.positions.cpu().numpy()
    act = res.actions.cpu().numpy()[:, :, 0].astype(np.float64)
    sg, sub, ns = (x.cpu().numpy() for x in scn)
    rows = np.arange(n) % len(sg)
    batch = _oracle_batch(1, sg, sub, ns, rows, v0)
    assert np.abs(pos[:, 0] - np.stack([batch.view["px"], batch.view["py"], batch.view["pz"]], 1)).max() == 0.0
    steps = rec["steps"].astype(np.int64)
    assert (steps > 0).all()
    ret = np.zeros(n)
    outcome = np.zeros(n, np.int64)
    ended = np.zeros(n, bool)
    max_p = 0.0
    for t in range(int(steps.max())):
        alive = t < steps
        assert np.isfinite(act[alive, t]).all()
        a0 = np.where(alive, np.nan_to_num(act[:, t]), 0.0)
        r, d, info, _ = batch.step(a0, want_obs=False)
        ret[alive] += r[alive]
        p = np.stack([batch.view["px"], batch.view["py"], batch.view["pz"]], 1)
        max_p = max(max_p, np.abs(p[alive] - pos[alive, t + 1]).max())
        done_now = alive & ~ended & (batch.view["done"] == 1)
        outcome[done_now] = np.where(info[done_now] == 2, _lib.EVAL_LOSE, _lib.EVAL_SUCCESS)
        ended |= done_now
        assert not (ended & (t + 1 < steps)).any(), "the oracle ended an episode before the kernel did"
    outcome[~ended] = _lib.EVAL_TRUNCATED
    err = np.abs(ret - rec["ret"])
    print(f"oracle replay, APF on, {kind}/{mode}: max |position error| {max_p:.3e}, max |return error| {err.max():.3e}, "
          f"max |return error| / steps {(err / steps).max():.3e}, steps up to {steps.max()}")
    assert (outcome == rec["outcome"]).all()
    assert (ended == (rec["outcome"] != _lib.EVAL_TRUNCATED)).all()
    assert max_p <= 1e-8
    assert (err <= 1e-9 * steps).all()
    assert (rec["outcome"] == _lib.EVAL_SUCCESS).any() and (rec["outcome"] == _lib.EVAL_LOSE).any()
    assert (steps[rec["outcome"] == _lib.EVAL_TRUNCATED] == T).all()
    env.close()


@pytest.mark.parametrize("apf", [0, 1])
def test_placement_invariance_and_repeatability(apf):
    U = 4
    env = _env(64, apf, U)
    Ls = _actors("init", U)
    n = 3000 + 37                                  # neither a multiple of 64 nor of U
    for mode in ("mean", "sample"):
        outs = []
        for mw in (1, 3, 0, 0):                    # (1 -> 3 -> automatic: every call has more resident lanes than the one before)
            res = ev.evaluate_sac_policy(env, Ls, n, seed=9, mode=mode, max_steps=300, max_workgroups=mw, trajectory_steps=8)
            outs.append(res.records.cpu().numpy().tobytes() + res.positions.cpu().numpy().tobytes() +
                        res.actions.cpu().numpy().tobytes())
        assert outs[0] == outs[1] == outs[2] == outs[3]
        rec = np.frombuffer(outs[0][:n * 64], dtype=ev.RECORD_DTYPE)
        assert (rec["steps"] > 0).all() and (rec["slot"] == np.arange(n) % U).all()
        # one actor for all episodes == the same actor in every slot
        one = ev.evaluate_sac_policy(env, Ls[0], n, seed=9, mode=mode, max_steps=300).host_records()
        four = ev.evaluate_sac_policy(env, [Ls[0]] * U, n, seed=9, mode=mode, max_steps=300).host_records()
        assert one.tobytes() == four.tobytes()
    env.close()


@pytest.mark.parametrize("apf", [0, 1])
def test_invalid_rows_are_recorded_not_flown(apf):
    env = _env(64, apf)
    L = _sac("init", 41)
    sg, sub, ns = (x.clone() for x in _scenarios())
    ns[5] = -3
    ns[6] = env.K + 1
    rec = ev.evaluate_sac_policy(env, L, 16, scenarios=(sg, sub, ns), v0=_v0(16, 1)).host_records()
    assert (rec["outcome"][[5, 6]] == _lib.EVAL_INVALID).all() and (rec["steps"][[5, 6]] == 0).all()
    assert ((rec["outcome"] != _lib.EVAL_INVALID).sum() == 14)
    env.close()


def test_noise_fill_is_deterministic_and_standard_normal():
    from scipy import stats
    a = ev.sac_noise(4096, 50, 3, DEV).cpu().numpy()
    b = ev.sac_noise(4096, 50, 3, DEV).cpu().numpy()
    c = ev.sac_noise(4096, 50, 4, DEV).cpu().numpy()
    assert a.tobytes() == b.tobytes() and not np.array_equal(a, c)
    assert np.isfinite(a).all()
    for d in (0, 1):
        assert stats.kstest(a[:, :, d].reshape(-1).astype(np.float64), "norm").pvalue > 1e-4
    assert stats.kstest(a.reshape(-1).astype(np.float64), "norm").pvalue > 1e-4
    assert abs(np.corrcoef(a[:, :, 0].reshape(-1), a[:, :, 1].reshape(-1))[0, 1]) < 0.01
    # a smaller table is a prefix in (episode, step): the draw depends on (seed, e, t, d) alone
    s = ev.sac_noise(100, 20, 3, DEV).cpu().numpy()
    assert np.array_equal(s, a[:100, :20])
    lib = _lib.load()
    out = torch.zeros(8, dtype=torch.float32, device=DEV)
    for bad in ((0, 2), (2, 0), (-1, 2), (1 << 16, 1 << 15)):
        assert lib.uavenv_eval_noise_fill(1, bad[0], bad[1], out.data_ptr(), None) == _lib.EINVAL
    assert lib.uavenv_eval_noise_fill(1, 2, 2, None, None) == _lib.EINVAL
    assert lib.uavenv_eval_noise_fill(1, 2, 2, out.data_ptr() + 2, None) == _lib.EINVAL


def _state_bytes(env):
    st, sub, al = env.get_state(0, env.N, want_sub=True)
    return st.tobytes() + sub.tobytes() + al.tobytes()


@pytest.mark.parametrize("apf", [0, 1])
def test_refusals_leave_the_env_unchanged(apf):
    U = 4
    env = _env(16, apf, U)
    env.reset(seed=4)
    act = torch.zeros(env.N, dtype=torch.float32, device=DEV)
    for _ in range(3):                             # (an APF env: the sub-goal lists have moved by now)
        env.step(act, skip_done=True)
    Ls = _actors("init", U)
    before, tick = _state_bytes(env), env.lib.uavenv_tick(env._h)
    rec = torch.zeros((64, 64), dtype=torch.uint8, device=DEV)
    lib = env.lib
    ptrs = [L._blocks[0].data_ptr() for L in Ls]

    def call(actors=None, h=None, **kw):
        a = _lib.UavSacEvalArgs()
        a.n, a.records = 64, rec.data_ptr()
        actors = ptrs if actors is None else actors
        arr = (C.c_void_p * max(len(actors), 1))(*actors)
        a.actors, a.n_actors, a.action_bound, a.mode = arr, len(actors), 1.0, _lib.EVAL_SAC_MEAN
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.uavenv_eval_episodes_sac(env._h if h is None else h, C.byref(a), env._stream())

    assert call() == 0 and call(actors=ptrs[:1]) == 0 and call(mode=_lib.EVAL_SAC_SAMPLE) == 0
    torch.cuda.synchronize()
    assert call(n=0) == _lib.EINVAL and call(n=-5) == _lib.EINVAL
    assert call(first=-1) == _lib.EINVAL
    assert call(actors=ptrs[:2]) == _lib.EINVAL and call(actors=ptrs[:3]) == _lib.EINVAL           # n_actors not in {1, U}
    assert call(n_actors=0) == _lib.EINVAL and call(n_actors=-1) == _lib.EINVAL
    assert call(actors=ptrs + ptrs) == _lib.EINVAL
    assert call(actors=None, n_actors=1) == 0                                                      # (sanity: the helper's default)
    a = _lib.UavSacEvalArgs(); a.n, a.records, a.n_actors, a.action_bound = 64, rec.data_ptr(), 1, 1.0
    assert lib.uavenv_eval_episodes_sac(env._h, C.byref(a), env._stream()) == _lib.EINVAL         # actors NULL
    assert call(actors=[ptrs[0], 0, ptrs[2], ptrs[3]]) == _lib.EINVAL                              # a NULL actor block
    assert call(actors=[ptrs[0] + 4]) == _lib.EINVAL                                               # a misaligned one
    for bound in (0.0, -1.0, float("nan"), float("inf")):
        assert call(action_bound=bound) == _lib.EINVAL
    assert call(mode=2) == _lib.EINVAL and call(mode=-1) == _lib.EINVAL
    assert call(traj_steps=5) == _lib.EINVAL and call(traj_steps=-1) == _lib.EINVAL
    tp = torch.zeros((64, 6, 3), dtype=torch.float64, device=DEV)
    ta = torch.zeros((64, 5, 2), dtype=torch.float32, device=DEV)
    assert call(traj_steps=5, traj_pos=tp.data_ptr()) == _lib.EINVAL                               # only one of the two
    assert call(traj_steps=5, traj_act=ta.data_ptr()) == _lib.EINVAL
    assert call(traj_steps=5, traj_pos=tp.data_ptr() + 4, traj_act=ta.data_ptr()) == _lib.EINVAL   # misaligned arrays
    assert call(traj_steps=5, traj_pos=tp.data_ptr(), traj_act=ta.data_ptr() + 4) == _lib.EINVAL
    assert call(records=rec.data_ptr() + 8) == _lib.EINVAL and call(records=None) == _lib.EINVAL
    v0 = torch.zeros((64, 2), dtype=torch.float64, device=DEV)
    assert call(v0=v0.data_ptr() + 4) == _lib.EINVAL
    sg = torch.zeros((4, 6), dtype=torch.float64, device=DEV)
    sub = torch.zeros((4, env.K, 3), dtype=torch.float64, device=DEV)
    ns = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert call(start_goal=sg.data_ptr(), m=4) == _lib.EINVAL                                      # only some of the three
    assert call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), m=4) == _lib.EINVAL
    assert call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), nsub=ns.data_ptr(), m=0) == _lib.EINVAL
    assert call(start_goal=sg.data_ptr(), sub=sub.data_ptr(), nsub=ns.data_ptr() + 2, m=4) == _lib.EINVAL
    assert call(max_steps=-1) == _lib.EINVAL and call(max_workgroups=-1) == _lib.EINVAL
    assert call(n=2 ** 31 - 100) == _lib.EINVAL                                                    # n + lanes leaves the index range
    torch.cuda.synchronize()
    assert _state_bytes(env) == before and env.lib.uavenv_tick(env._h) == tick
    # no world: an env that never saw uavenv_set_buildings; no scenarios: an env without a bank
    h = C.c_void_p()
    _lib.check(lib.uavenv_create(C.byref(env.cfg), C.byref(h)), "uavenv_create")
    assert call(h=h) == _lib.EINVAL
    lib.uavenv_destroy(h)
    env.close()
    from dqn_based_uav_3d_path_planer_amd.env import VecPathPlanEnv
    nob = VecPathPlanEnv(16, load_city26()["buildings"], obs_dtype="packed", uav_per_env=U, apf_enabled=apf)
    a = _lib.UavSacEvalArgs(); a.n, a.records, a.n_actors, a.action_bound = 64, rec.data_ptr(), 1, 1.0
    a.actors = (C.c_void_p * 1)(ptrs[0])
    assert nob.lib.uavenv_eval_episodes_sac(nob._h, C.byref(a), nob._stream()) == _lib.EINVAL
    nob.close()
    # the DQN entry still refuses an APF env
    if apf:
        from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
        D = FusedDQNLearner({"w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99", "Update_loop": "3",
                             "NetWork": "Qnet2"}, "dqn", device=DEV)
        e2 = _env(16, 1)
        b = _lib.UavEvalArgs(); b.n, b.records = 64, rec.data_ptr()
        assert e2.lib.uavenv_eval_episodes(e2._h, C.byref(D.net), C.byref(b), e2._stream()) == _lib.EINVAL
        e2.close()


@pytest.mark.parametrize("apf", [0, 1])
def test_training_is_the_same_with_an_evaluation_in_between(apf):
    from dqn_based_uav_3d_path_planer_amd.loop import SACHotLoop
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing

    def run(with_eval):
        U, envs, B = 4, 512, 256
        env = _env(envs, apf, U)
        ring = DeviceReplayRing(env, 40 * env.N, discrete=False)
        ring.reset(seed=1000)
        a1 = torch.zeros((ring.frames, env.N), dtype=torch.float32, device=DEV)
        torch.manual_seed(42)
        Ls = [FusedSACLearner(PARAM, DEV) for _ in range(U)]
        loop = SACHotLoop(ring, Ls, B, seed=7, act1_plane=a1)
        loop.run(12)
        if with_eval:
            for mode in ("mean", "sample"):
                s = ev.evaluate_sac_policy(env, Ls, 2048, seed=5, mode=mode, max_steps=200).summary()
                assert s["episodes"] == 2048
            assert Ls[0].evaluate(env, 256, max_steps=50).summary()["episodes"] == 256
        loop.run(12)
        torch.cuda.synchronize()
        out = tuple(L._blocks.cpu().numpy().tobytes() + L._cblocks.cpu().numpy().tobytes() + L._alpha_mv.cpu().numpy().tobytes() +
                    L.log_alpha.cpu().numpy().tobytes() for L in Ls)
        out += tuple(getattr(ring, k).cpu().numpy().tobytes() for k in ("obs", "action", "reward", "done", "valid"))
        out += (a1.cpu().numpy().tobytes(), _state_bytes(env), env.lib.uavenv_tick(env._h), ring.head, ring.filled)
        loop.close()
        env.close()
        return out

    assert run(False) == run(True)


@pytest.mark.parametrize("apf", [0, 1])
def test_plugin_evaluate_policy(apf, tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver

    def episode(with_eval):
        torch.manual_seed(0)
        d = tmp_path / ("eval" if with_eval else "plain")
        d.mkdir()
        monkeypatch.chdir(d)                       # (the config's paths are relative to the working directory)
        xml = driver.make_config_dir(str(d), "SAC", num_envs=64, num_uav=4)
        if apf:
            uav_xml = d / "config" / "UAV.xml"
            uav_xml.write_text(re.sub(r"<APF_Enabled>0</APF_Enabled>", "<APF_Enabled>1</APF_Enabled>", uav_xml.read_text()))
        env = driver.simulator(xml).env
        assert env.backend.cfg.apf_enabled == apf and all(isinstance(u.Trainer.learner, FusedSACLearner) for u in env.Agents)
        summ = None
        if with_eval:
            summ = env.evaluate_policy(n_episodes=128, seed=1, max_steps=300)
            assert env.evaluate_policy(n_episodes=128, seed=1, max_steps=300, mode="mean") == summ
            smp = env.evaluate_policy(n_episodes=128, seed=1, max_steps=300, mode="sample")
            assert smp != summ
            with pytest.raises(ValueError):
                env.evaluate_policy(n_episodes=128, mode="greedy")
            # the slots fly the same missions from the same headings: with slot 0's actor in slot 1 the two agree on everything
            # but the energy (each slot's own power parameters)
            l0, l1 = env.Agents[0].Trainer.learner, env.Agents[1].Trainer.learner
            saved = l1._blocks[0].clone()
            with torch.no_grad():
                l1._blocks[0].copy_(l0._blocks[0])
            same = env.evaluate_policy(n_episodes=128, seed=1, max_steps=300)
            with torch.no_grad():
                l1._blocks[0].copy_(saved)
            for k in ("success", "lose", "truncated", "mean_return", "mean_steps", "mean_path_len", "mean_subgoals",
                      "mean_collisions", "average_score"):
                assert same[0][k] == same[1][k], k
            assert same[0]["mean_energy"] != same[1]["mean_energy"]
            assert same[0] == summ[0] and same[2] == summ[2] and same[3] == summ[3]
        torch.manual_seed(1)
        res = env.run_eposide(0.5)
        return summ, res

    summ, res1 = episode(True)
    assert len(summ) == 4
    for s in summ:
        assert s["episodes"] == 128 and s["success"] + s["lose"] + s["truncated"] + s["invalid"] == 128
    _, res0 = episode(False)
    assert res0["success"] == res1["success"] and res0["lose"] == res1["lose"] and res0["sum_epoch"] == res1["sum_epoch"]
    assert (res0["loss"] == res1["loss"]) or (np.isnan(res0["loss"]) and np.isnan(res1["loss"]))


def test_plugin_refuses_a_mixture_of_trainers(tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver
    monkeypatch.chdir(tmp_path)
    env = driver.simulator(driver.make_config_dir(str(tmp_path), "SAC", num_envs=64, num_uav=2)).env

    class _Other:
        learner = object()
    keep = env.Agents[1].Trainer
    env.Agents[1].Trainer = _Other()
    with pytest.raises(RuntimeError):
        env.evaluate_policy(n_episodes=64)
    env.Agents[1].Trainer = keep
    assert len(env.evaluate_policy(n_episodes=64, max_steps=100)) == 2
