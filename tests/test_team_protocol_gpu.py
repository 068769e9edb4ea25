"""The step kernels' team protocol on the device against oracle/team_model.py, at every team size U = 1 .. 64.

What binds the U agents of an env together -- a finished agent waits, the env restarts in the launch that completes it, UAV j
flies with its own power parameters -- is wavefront arithmetic that depends on U (the done ballot, the group mask shifted to the
team's first lane, reset_agents_wave, ii % U).  tests/team_protocol.py scripts three-wavefront envs (N = U x 130, 65, 33, 17, 9, 5,
3: the last wavefront ragged wherever U allows, one team in a half-empty wave at U = 32, a team the whole wave at U = 64) through
every way a team can finish, and check_launch holds every launch to the model, the C oracle (loaded from the device's own pre-step
state, with UAV j's A and xi) and reset_draws.  tests/test_team_model.py shows on the host that the script covers what it is there
for and that these assertions reject each plausible wrong protocol.

Injection: uavenv_set_state clears `done`, so only agents that still fly are injected (contiguous runs of them); that the
waiting members stay bit-identical is asserted at every injection.

Rule pinned where include/uavenv.h left it open: when a team is complete, EVERY agent of it is re-drawn in that launch -- also a
member the `active` mask leaves out (its outputs still say info SKIPPED, valid 0, ret_done = done as it was).

RECORD (MI355X; worst error over bar per form, over all U of the form and all launches; bars: REWARD_TOL, STATE_TOL, OBS_TOL_F32 /
OBS_TOL_F16, 1e-9 relative energy -- all the project's existing ones, none derived from these numbers):
  form       U            variant  classes hit (ragged wavefront's team)                      reward    state     obs     energy
  coop       1..64        0        all (U = 2..32: one@0, one@1, all_but_one, later)          5.7e-5    1.4e-5    0.030   0
  one_wave   1..64        1        all (U = 2..32: none, whole, one@U/2, one@U-1)             5.7e-5    1.4e-5    0.030   0
  apf_split  8, 16, 64    0        all (as variant 0)                                         5.7e-5    1.4e-5    0.029   0
  apf_lane   2, 4, 32     1        all (as variant 1)                                         5.7e-5    1.4e-5    0.029   0
  f16        1, 8, 32     0        all (as variant 0)                                         5.7e-5    1.4e-5    0.24    0
  packed     2, 4, 64     1        all (as variant 1)                                         5.7e-5    1.4e-5    0.030   0
  noskip     2, 16, 64    0        all (as variant 0); done agents step on                    5.7e-5    1.4e-5    0.030   0
  active     4, 8, 32     0, 1     masked done member counts / masked live member blocks,     5.7e-5    1.4e-5    0.029   0
                                   each in the ragged wavefront (variant 0 / 1)
  large      8            -        none, one@0, one@1, all_but_one, whole, later (ragged too) 6.4e-5    2.8e-5    0.030   0
  policy, polh  8         0        all; bit-equal to the twin
  eval slots    8         -        per-step energy 150.88 .. 161.94 J rising with j; energy worst / bar 0
"all" = none, one@0, one@1, one@U/2, one@U-1, all_but_one, whole, later (U = 1: none, whole).  U = 64 has no ragged wavefront.
Energy came out bit-equal to the float64 restatement of Calc_Fly_Power everywhere.  No kernel fault or wrong result was found;
a library built with the cooperative kernel's mask unshifted and the one-wave kernel's j = i / U failed 15 of the 17 coop /
one_wave / noskip cases (all but coop and noskip at U = 64, where an unshifted mask is the same mask).
"""
import numpy as np
import pytest
import torch

import team_protocol as tp
from dqn_based_uav_3d_path_planer_amd import _lib
from dqn_based_uav_3d_path_planer_amd.data import load_city26, make_city26_env
from dqn_based_uav_3d_path_planer_amd.env import StepOut
from oracle import pyoracle as po
from oracle import team_model as tm
from test_team_model import FORMS, SCRIPT_FORM, _apf_velocities, _coverage, make_ctx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(form, U, variant) for form, us, variant in FORMS for U in us]
CANARY = 64                                # rows behind every output plane


def _env_kw(form):
    kw = dict(max_subgoals=tp.K)
    if form.startswith("apf"):
        kw["apf_enabled"] = 1
    if form in ("f16", "polh"):
        kw["obs_dtype"] = torch.float16
    if form in ("packed", "policy"):
        kw["obs_dtype"] = "packed"
    return kw


def _step_kw(form):
    return dict(one_wave=form == "one_wave", apf_lane=form == "apf_lane")      # apf_split: an APF env's default (k_apf_adjust + k_step)


def _runs(mask):
    """[(first, count)] of the contiguous runs of a bool mask."""
    idx = np.nonzero(mask)[0]
    if not len(idx):
        return []
    cut = np.nonzero(np.diff(idx) != 1)[0] + 1
    return [(int(r[0]), len(r)) for r in np.split(idx, cut)]


class DevEnv:
    """HostEnv's interface on a VecPathPlanEnv: reset, state, expire, step -> the record check_launch takes."""

    def __init__(self, U, form, n_envs=None):
        self.form, self.U = form, U
        self.env = make_city26_env(tp.N_ENVS[U] if n_envs is None else n_envs, uav_per_env=U, **_env_kw(form))
        if form.startswith("apf"):
            self.env.set_buildings(self.env.buildings, velocities=_apf_velocities())
        self.N = n = self.env.N
        self.max_step = int(load_city26()["max_step"])
        e = self.env
        self.planes = dict(
            obs=torch.full((n + CANARY, e.obs_width), -7, dtype=e.obs_dtype, device=DEV),
            reward=torch.full((n + CANARY,), -7.0, dtype=torch.float64, device=DEV),
            reward32=torch.full((n + CANARY,), -7.0, dtype=torch.float32, device=DEV),
            energy=torch.full((n + CANARY,), -7.0, dtype=torch.float64, device=DEV),
            **{k: torch.full((n + CANARY,), 0xA5, dtype=torch.uint8, device=DEV) for k in ("ret_done", "agent_done", "info", "valid")})
        self.out = StepOut(**{k: v[:n] for k, v in self.planes.items()})

    def close(self):
        self.env.close()

    def tick(self):
        return int(self.env.lib.uavenv_tick(self.env._h))

    def reset(self, seed):
        self.seed = seed
        self.env.reset(seed)
        assert self.tick() == 1

    def state(self):
        return self.env.get_state(0, self.N, want_sub=True)

    def expire(self, who):
        """Step = max_step - 1 for the agents of `who` (all of them still flying), run by run; everyone else bit-identical."""
        before = self.state()
        st, sub, alias = before
        assert not (st[who, 10] != 0).any()
        for first, count in _runs(who):
            s = slice(first, first + count)
            self.env.set_state(first, np.c_[st[s, 0:5], st[s, 6:9]], np.full(count, self.max_step - 1, np.int32),
                               st[s, 11].astype(np.int32), sub[s], alias=alias[s])
        st2, sub2, alias2 = self.state()
        assert np.array_equal(st2[~who], st[~who]) and np.array_equal(sub2[~who], sub[~who]) and np.array_equal(alias2[~who], alias[~who])
        assert np.array_equal(st2[who][:, [0, 1, 2, 6, 7, 8, 11]], st[who][:, [0, 1, 2, 6, 7, 8, 11]])
        assert not who.any() or np.abs(st2[who, 3:6] - st[who, 3:6]).max() <= 1e-15        # (Calc_V may rescale the velocity by an ulp)
        assert (st2[who, 9] == self.max_step - 1).all() and (st2[who, 10] == 0).all()
        assert np.array_equal(sub2[who], sub[who]) and np.array_equal(alias2[who], alias[who])

    def canaries_intact(self):
        n = self.N
        for k, v in self.planes.items():
            tail = v[n:]
            want = 0xA5 if v.dtype == torch.uint8 else -7
            assert bool((tail == want).all()), k

    def step(self, steer, flags, active=None, pre=None, post_window=None):
        n = self.N
        pre = self.state() if pre is None else pre
        tick = self.tick()
        act = None if active is None else torch.from_numpy(np.ascontiguousarray(active, dtype=np.uint8)).to(DEV)
        a = torch.from_numpy(np.ascontiguousarray(steer, dtype=np.float64)).to(DEV)
        self.env.step(a, self.out, auto_reset=bool(flags & tm.AUTO_RESET), skip_done=bool(flags & tm.SKIP_DONE), active=act,
                      **_step_kw(self.form))
        torch.cuda.synchronize()
        assert self.tick() == tick + 1
        self.canaries_intact()
        o = self.out
        out = {k: getattr(o, k).cpu().numpy().copy() for k in ("reward", "reward32", "ret_done", "agent_done", "info", "valid", "energy")}
        out["obs"] = self.env.unpack(o.obs).cpu().numpy().astype(np.float64)
        assert np.array_equal(out["reward32"], out["reward"].astype(np.float32))
        return dict(flags=flags, active=active, seed=self.seed, tick=tick, steer=np.asarray(steer, dtype=np.float64), pre=pre,
                    post=self.state() if post_window is None else None, out=out)


def _obs_tol(form):
    return tp.OBS_TOL_F16 if form in ("f16", "polh") else tp.OBS_TOL_F32


def _merge(total, stats):
    for k, v in stats.items():
        total[k] = max(total.get(k, 0.0), v)


@pytest.mark.parametrize("form,U,variant", CASES)
def test_scripted_teams_against_the_model(form, U, variant):
    ctx = make_ctx(U, form)
    dev = DevEnv(U, form)
    script = SCRIPT_FORM.get(form, "plain")
    total, ms = {}, []

    def check(rec, t):
        m = tp.check_launch(ctx, rec, _obs_tol(form), apf=form.startswith("apf"))
        ms.append(m)
        _merge(total, m["stats"])

    recs = tp.run_script(dev, U, variant, script, check)
    every, ragged = _coverage(U, script, variant, recs)          # the device went through the classes the host run predicts
    restarts = sum(int(m["restart_envs"].sum()) for m in ms[1:])
    assert restarts >= 2
    if script != "active":
        assert every >= tp.possible_classes(U)
    else:
        m1 = ms[1 + tp.MASKED[0]]
        masked_restarted = m1["restarted"] & ~m1["stepping"]
        assert masked_restarted.any()                            # masked members of a completed team were re-drawn with it
    print("TEAM %-9s U=%-2d v%d classes=%s ragged=%s restarts=%d worst/bar: %s" % (
        form, U, variant, ",".join(sorted(every)), ",".join(sorted(ragged)) or "-", restarts,
        " ".join("%s=%.3g" % kv for kv in sorted(total.items()))))
    dev.close()


def test_one_large_launch_pair_at_256_thread_workgroups():
    """U = 8, N = 131 144 (just above 131 072: 256-thread workgroups and the tile store; eight agents in the last wavefront), f32
    rows, two scripted launches.  The team model and the restart draws over ALL agents (flags, who is re-drawn, who is untouched);
    the C oracle on a window of 4 096 envs -- the first ones in launch 0, the last ones, with the ragged wavefront, in launch 1.
    Programs: P1 / P2 alternate (nobody, then the whole team / the whole team, then all but one of the fresh one); the last 128 envs
    take P0 (one@0, one@1 beside a waiting member) and P3 (all but one, then completed by the last member while seven wait -- the
    ragged wavefront's team among them).  Waiting members exist only in those 128 envs, so the live agents between them are
    few enough runs to inject run by run."""
    U, n_envs, W = 8, 16384 + 9, 4096
    ctx = tp.Ctx(U, n_envs=n_envs)
    dev = DevEnv(U, "coop", n_envs=n_envs)
    N, env = dev.N, dev.env
    assert N > 131072 and N % 64 == 8
    prog = [("P1", "P2")[e % 2] for e in range(n_envs - 128)] + ["P0"] * 64 + ["P3"] * 64
    dev.reset(tp.SEED)
    rng = np.random.default_rng(8)
    out = dev.step(-1.0 + rng.integers(0, 3, N), tp.FLAGS, pre=(env.get_state(0, N), None, None), post_window=True)["out"]
    assert not out["agent_done"].any()
    restarts, seen = 0, set()
    for t in range(2):
        st, sub, alias = env.get_state(0, N, want_sub=True)
        done = st[:, 10] != 0
        who = tp.expire_mask(U, 0, "plain", t, done, prog)
        step = np.where(who, ctx.max_step - 1, st[:, 9]).astype(np.int32)
        runs = _runs(~done)                              # the live agents, whoever is pushed among them: Step is per agent
        assert len(runs) <= 130 and (t == 0 or len(runs) > 100)
        for first, count in runs:
            s = slice(first, first + count)
            env.set_state(first, np.c_[st[s, 0:5], st[s, 6:9]], step[s], st[s, 11].astype(np.int32), sub[s], alias=alias[s])
        st_in = env.get_state(0, N)
        assert np.array_equal(st_in[done], st[done]) and np.array_equal(st_in[:, [0, 1, 2, 6, 7, 8, 10, 11]], st[:, [0, 1, 2, 6, 7, 8, 10, 11]])
        assert np.abs(st_in[:, 3:6] - st[:, 3:6]).max() <= 1e-15
        first = 0 if t == 0 else N - W * U
        pre_w = env.get_state(first, W * U, want_sub=True)
        assert np.array_equal(pre_w[1], sub[first:first + W * U]) and np.array_equal(pre_w[2], alias[first:first + W * U])
        steer = -1.0 + rng.integers(0, 3, N).astype(np.float64)
        rec = dev.step(steer, tp.FLAGS, pre=(st_in, None, None), post_window=True)
        st1 = env.get_state(0, N)
        o = rec["out"]
        stepping = tm.who_steps(tp.FLAGS, done)
        z = np.zeros(N)
        m = tm.launch(U, tp.FLAGS, done, z, z, z, o["agent_done"], None)       # done-after of the stepping agents: the device's
        assert np.array_equal(o["valid"], m["valid"]) and np.array_equal(o["agent_done"], m["agent_done"])
        assert (o["info"][~stepping] == tm.INFO_SKIPPED).all() and (o["info"][stepping] != tm.INFO_SKIPPED).all()
        assert np.array_equal(o["ret_done"][~stepping] != 0, done[~stepping])
        assert np.array_equal((o["agent_done"] != 0) & ~done, who)             # who finishes is who was pushed, nobody else
        tp.check_restarts(ctx, tp.SEED, rec["tick"], 0, st_in, st1, m["restarted"])
        same = ~stepping & ~m["restarted"]
        assert same.any() == (t == 1)
        assert np.array_equal(st1[same], st_in[same])
        restarts += int(m["restart_envs"].sum())
        b, a = done.reshape(-1, U), (o["agent_done"] != 0).reshape(-1, U)
        for e in list(range(6)) + list(range(n_envs - 128, n_envs)):
            seen |= tp.classify(U, b[e], a[e] & ~b[e])
        post_w = env.get_state(first, W * U, want_sub=True)
        win = slice(first, first + W * U)
        wrec = dict(rec, steer=steer[win], pre=pre_w, post=post_w, out={k: v[win] for k, v in o.items()})
        mw = tp.check_launch(ctx, wrec, tp.OBS_TOL_F32, first=first)
        assert np.array_equal(mw["restarted"], m["restarted"][win])
        print("TEAM large U=8 launch", t, "restart envs", int(m["restart_envs"].sum()), "worst/bar:", mw["stats"])
    assert restarts > 10000 and m["restarted"][-U:].all()                      # ... the ragged wavefront's team in launch 1
    assert seen >= {"none", "one@0", "one@1", "all_but_one", "whole", "later"}, seen
    dev.close()


# ------------------------------------------------------------------------------------------------ the policy-in-step forms
PARAM = {"w": "100", "hiden_dim": "64", "output": "3", "LEARNING_RATE": "0.001", "gamma": "0.99", "Update_loop": "3"}


@pytest.mark.parametrize("form", ["policy", "polh"])
def test_policy_in_step_forms_equal_a_twin_stepped_by_plain_step(form):
    """uavenv_step_policy at U = 8, eps = 0: k_step_coop<policy> on packed rows, k_step_polh on f16 rows.  A twin env stepped by
    plain env.step (the form held to the oracle above) with the actions the kernel recorded agrees bit for bit on state, flags,
    valid and restart set over the same script; the restart set is also the model's."""
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
    U = 8
    ctx = tp.Ctx(U)
    a_env = make_city26_env(tp.N_ENVS[U], uav_per_env=U, **_env_kw(form))
    twin = DevEnv(U, "f16" if form == "polh" else "packed")
    N = a_env.N
    ring = DeviceReplayRing(a_env, 8 * N, discrete=True)
    torch.manual_seed(5)
    if form == "polh":
        ring.extra_flags = _lib.STEP_ONE_WAVE
        L = FusedDQNLearner(dict(PARAM, NetWork="VAnet2"), "dueling", device=DEV, mfma="f16")
    else:
        L = FusedDQNLearner(dict(PARAM, NetWork="Qnet2"), "dqn", device=DEV)
    ring.reset(seed=tp.SEED)
    twin.reset(tp.SEED)
    ad = torch.zeros(N, dtype=torch.uint8, device=DEV)
    restarts, seen = 0, set()
    for t in range(-1, tp.LAUNCHES):
        st, sub, alias = a_env.get_state(0, N, want_sub=True)
        done = st[:, 10] != 0
        if t >= 0:
            who = tp.expire_mask(U, 0, "plain", t, done)
            for first, count in _runs(who):
                s = slice(first, first + count)
                a_env.set_state(first, np.c_[st[s, 0:5], st[s, 6:9]], np.full(count, ctx.max_step - 1, np.int32),
                                st[s, 11].astype(np.int32), sub[s], alias=alias[s])
            a_env.observe(ring.obs[ring.head])                              # the current frame's rows carry Step
            twin.expire(who)
        pre = a_env.get_state(0, N, want_sub=True)
        tpre = twin.state()
        assert all(np.array_equal(x, y) for x, y in zip(pre, tpre))
        frame, tick = ring.head, int(a_env.lib.uavenv_tick(a_env._h))
        assert ring.step_policy(L, 0.0, 31, t + 1, auto_reset=True, skip_done=True, agent_done=ad)
        torch.cuda.synchronize()
        act = ring.action[frame].clone()
        assert int(act.min()) >= 0 and int(act.max()) <= 2
        twin.env.step(act, twin.out, auto_reset=True, skip_done=True)
        torch.cuda.synchronize()
        twin.canaries_intact()
        o = twin.out
        assert torch.equal(ring.reward[frame], o.reward32) and torch.equal(ring.done[frame], o.ret_done)
        assert torch.equal(ring.valid[frame], o.valid) and torch.equal(ad, o.agent_done)
        assert torch.equal(ring.obs[ring.head], o.obs)
        post = a_env.get_state(0, N, want_sub=True)
        assert all(np.array_equal(x, y) for x, y in zip(post, twin.state()))
        z = np.zeros(N)
        done_now = pre[0][:, 10] != 0
        m = tm.launch(U, tp.FLAGS, done_now, z, z, z, ad.cpu().numpy(), None)
        assert np.array_equal(ring.valid[frame].cpu().numpy(), m["valid"])
        tp.check_restarts(ctx, tp.SEED, tick, 0, pre[0], post[0], m["restarted"], post[1], post[2])
        restarts += int(m["restart_envs"].sum())
        if t >= 0:
            seen |= tp.events(U, done_now, ad.cpu().numpy())[0]
    assert restarts >= 2 and seen >= tp.possible_classes(U)
    a_env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ the evaluation kernels
def test_evaluation_energy_is_uav_js_power_along_the_trajectory():
    """uavenv_eval_episodes_slots with one net at U = 8 (episode e flies as UAV slot e mod U): the mean recorded energy per step
    strictly increases with j, and for one episode per slot the recorded energy is the sum of the model's Calc_Fly_Power of UAV j
    along the trajectory the kernel recorded, replayed by the C oracle (<= 1e-9 relative x steps)."""
    from dqn_based_uav_3d_path_planer_amd import evaluate as ev
    from dqn_based_uav_3d_path_planer_amd.learner import FusedDQNLearner
    U, n, T = 8, 128, 24
    c = load_city26()
    env = make_city26_env(8, uav_per_env=U, max_subgoals=tp.K)
    torch.manual_seed(7)
    L = FusedDQNLearner(dict(PARAM, NetWork="Qnet2"), "dqn", device=DEV)
    ang = np.random.default_rng(3).uniform(0, 2 * np.pi, n)
    v0 = np.c_[np.cos(ang), np.sin(ang)] * float(c["max_v"])
    res = ev.evaluate_policy(env, [L], n, v0=v0, max_steps=T, trajectory_steps=T)
    rec = res.host_records()
    pos, act = res.positions.cpu().numpy(), res.actions.cpu().numpy().astype(np.int64)
    assert (rec["slot"] == np.arange(n) % U).all() and (rec["steps"] == T).all()
    per_step = np.array([(rec["energy"][j::U] / rec["steps"][j::U]).mean() for j in range(U)])
    assert (np.diff(per_step) > 0).all(), per_step
    ctx = tp.Ctx(U)
    sg, sub, ns = ctx.bank
    worst = 0.0
    for e in range(U, 2 * U):                                                  # one episode per slot
        j, row = e % U, e % len(ns)
        u = po.OracleUav(ctx.world, ctx.params)
        u.set_state(*sg[row, :3], v0[e, 0], v0[e, 1], *sg[row, 3:], 0, sub[row, :ns[row]])
        u.u.sub0_alias = 1
        total = 0.0
        for t in range(int(rec["steps"][e])):
            assert act[e, t] in (0, 1, 2)
            u.update(-1.0 + act[e, t])
            assert abs(u.u.px - pos[e, t + 1, 0]) <= tp.STATE_TOL and abs(u.u.py - pos[e, t + 1, 1]) <= tp.STATE_TOL
            total += tm.fly_power(ctx.power, u.u.V, j)
        err = abs(rec["energy"][e] - total) / abs(total)
        worst = max(worst, err / (tp.ENERGY_RTOL * rec["steps"][e]))
        assert err <= tp.ENERGY_RTOL * rec["steps"][e], (e, err)
    print("TEAM eval per-step energy by slot", per_step, "worst/bar", worst)
    env.close()
