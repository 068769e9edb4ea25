"""What tests/test_team_model.py (host) and tests/test_team_protocol_gpu.py (device) share: the scripted scenario that walks every
team through every way of finishing, the per-launch assertions against oracle/team_model.py + oracle/uav_oracle.c +
oracle/philox.py, and a device-free stand-in for the env (HostEnv) on which the assertions are shown to reject each plausible
wrong team protocol.  No torch, no device here."""
import ctypes as C

import numpy as np

from dqn_based_uav_3d_path_planer_amd.data import load_city26
from oracle import philox as px
from oracle import pyoracle as po
from oracle import team_model as tm

REWARD_TOL = 1e-9          # the bars of tests/test_env_parity_gpu.py
STATE_TOL = 1e-9
OBS_TOL_F32 = 2e-6
OBS_TOL_F16 = 2e-3
ENERGY_RTOL = 1e-9         # test_energy_column_is_calc_fly_power
SUB_TOL = 1e-8             # sub-goal lists (Adjust_subgoal moves all of them under APF), as _check_slice_against_oracle

SEED = (0x7EA3 << 32) | 5                                   # above 2^32: the key's high word
N_ENVS = {1: 130, 2: 65, 4: 33, 8: 17, 16: 9, 32: 5, 64: 3}  # three wavefronts each; the last one ragged wherever U allows
LAUNCHES = 4
K = 48
FLAGS = tm.AUTO_RESET | tm.SKIP_DONE
CLASSES = ("none", "one@0", "one@1", "one@U/2", "one@U-1", "all_but_one", "whole", "later")


# ------------------------------------------------------------------------------------------------ the script
# A program tells, per scripted launch, which members of ONE env are put one step from the time limit (only members that still
# fly are; a waiting member stays as it is).  ("set", p, ...) the members at those places, ("all_but", p), ("all",), ("none",).
def _programs(U):
    h, last = U // 2, U - 1
    return {
        "P0": [("set", 0), ("set", 1), ("all_but", last), ("all",)],       # one@0, one@1, all but one, completed by the last member
        "P1": [("none",), ("all",), ("set", h), ("set", last)],             # nobody, the whole team at once, one@U/2, one@U-1 (fresh team)
        "P2": [("all",), ("all_but", min(1, last)), ("all",), ("none",)],   # whole, all but one of a fresh team, completed, nobody
        "P3": [("all_but", last), ("all",), ("none",), ("none",)],          # (the large case) all but one, completed by the last member
        # the `active` form (mask = slot S_ACTIVE in launches 1 and 2, see MASKED): a masked done member counts, a masked live one blocks
        "M0": [("all_but", min(1, last)), ("set", min(1, last)), ("none",), ("none",)],
        "M1": [("none",), ("set", min(1, last)), ("none",), ("all",)],
        "M2": [("set", 0), ("set", min(1, last)), ("none",), ("none",)],
    }


MASKED = (1, 2)                       # the launches of the `active` form that run under the mask


def active_slot(U):
    return min(1, U - 1)


def program_of(U, variant, form="plain", n_envs=None):
    """The program name of every env: they rotate, and the LAST env (the ragged wavefront's team for U = 2..32) takes the
    variant's, so that over variants 0 and 1 it goes through every class."""
    names = ("M0", "M1", "M2") if form == "active" else ("P0", "P1", "P2")
    n = N_ENVS[U] if n_envs is None else n_envs
    out = [names[e % 3] for e in range(n)]
    out[-1] = names[variant % 2]
    if U == 1:                        # two teams in the ragged wavefront: one of each
        out[-2] = names[(variant + 1) % 2]
    return out


def members(spec, U):
    m = np.zeros(U, bool)
    if spec[0] == "set":
        m[[p for p in spec[1:] if p < U]] = True
    elif spec[0] == "all_but":
        m[:] = True
        m[spec[1]] = False
    elif spec[0] == "all":
        m[:] = True
    return m


def expire_mask(U, variant, form, t, done, prog=None):
    """bool [N]: the agents to put one step from the limit before scripted launch t, given the done flags then (prog: the
    program name of every env where it is not program_of's)."""
    prog, P = program_of(U, variant, form, len(done) // U) if prog is None else prog, _programs(U)
    rows = {name: members(P[name][t], U) for name in set(prog)}
    want = np.concatenate([rows[name] for name in prog])
    return want & ~np.asarray(done).astype(bool)


def launch_args(U, form, t, n_envs=None):
    """(flags, active mask or None) of scripted launch t."""
    N = U * (N_ENVS[U] if n_envs is None else n_envs)
    if form == "noskip":
        return tm.AUTO_RESET, None
    if form == "active" and t in MASKED:
        return FLAGS, (np.arange(N) % U == active_slot(U)).astype(np.uint8)
    return FLAGS, None


def classify(U, before, finishing):
    """The classes of one team's launch: before / finishing bool [U] (done before it; finishing in it)."""
    live = ~before
    if not live.any():
        return set()
    f, out = np.nonzero(finishing)[0], set()
    after_live = int((live & ~finishing).sum())
    if len(f) == 0:
        out.add("none")
    if len(f) == 1 and after_live >= 1:
        for name, p in (("one@0", 0), ("one@1", 1), ("one@U/2", U // 2), ("one@U-1", U - 1)):
            if f[0] == p:
                out.add(name)
    if len(f) >= 1 and after_live == 1:
        out.add("all_but_one")
    if not before.any() and after_live == 0:
        out.add("whole")
    if before.any() and len(f) == 1 and after_live == 0:
        out.add("later")
    return out


def possible_classes(U):
    if U == 1:
        return {"none", "whole"}
    return set(CLASSES)


def ragged_envs(U):
    """The envs of the last wavefront where it is ragged (none at U = 64: a team is the whole wave)."""
    N = U * N_ENVS[U]
    if N % 64 == 0:
        return []
    return list(range((N // 64 * 64) // U, N_ENVS[U]))


def events(U, done_before, done_after_launch):
    """-> (classes hit anywhere, classes hit in the ragged wavefront) of one launch; done_after_launch = agent_done of it."""
    b = np.asarray(done_before).astype(bool).reshape(-1, U)
    a = np.asarray(done_after_launch).astype(bool).reshape(-1, U)
    every, ragged = set(), set()
    rag = set(ragged_envs(U))
    for e in range(len(b)):
        c = classify(U, b[e], a[e] & ~b[e])
        every |= c
        if e in rag:
            ragged |= c
    return every, ragged


# ------------------------------------------------------------------------------------------------ the oracle side
class Ctx:
    """World, bank and parameters of one team size on the host."""

    def __init__(self, U, n_envs=None, apf=False, velocities=None):
        c = load_city26()
        self.U, self.n_envs = U, N_ENVS[U] if n_envs is None else n_envs
        self.N = self.U * self.n_envs
        self.power, self.max_v, self.max_step = c["power"], float(c["max_v"]), int(c["max_step"])
        self.world = po.OracleWorld(c["buildings"], float(c["len"]), float(c["width"]), float(c["h"]), velocities=velocities)
        self.params = dict(po.default_uav_params(c), apf_enabled=1 if apf else 0)
        sub = np.zeros((len(c["n_sub"]), K, 3))
        sub[:, :min(K, c["sub_goals"].shape[1])] = c["sub_goals"][:, :K]
        self.bank = (c["start_goal"], sub, c["n_sub"])
        self._batches = {}

    def batch(self, first, count):
        """An OracleBatch for agents [first, first + count) with UAV j's own A and xi (Agents/UAV.py:55,58)."""
        key = (first % self.U, count)
        if key not in self._batches:
            b = po.OracleBatch(self.world, self.params, count)
            b.view["A"], b.view["xi"] = tm.slot_power_params(self.power, tm.uav_slot(first + np.arange(count), self.U))
            self._batches[key] = b
        return self._batches[key]


def _view_state(v, n_k):
    st = np.c_[v["px"], v["py"], v["pz"], v["vx"], v["vy"], v["V"], v["gx"], v["gy"], v["gz"], v["step"], v["done"], v["n_sub"],
               v["score"], v["total_score"], v["path_len"], v["reach_goal"]].astype(np.float64)
    return st, np.array(v["sub"][:, :n_k]), np.array(v["sub0_alias"])


def oracle_step(ctx, pre, steer, first=0):
    """update_PathPlan + state_PathPlan of EVERY agent of the slice from the state `pre` (the caller reads the agents that step)."""
    st, sub, alias = pre
    b = ctx.batch(first, len(st))
    b.set_from_state16(st, sub, alias)
    r, d, info, obs = b.step(np.asarray(steer, dtype=np.float64), want_obs=True)
    post = _view_state(b.view, sub.shape[1])
    energy = np.array([b.lib.orc_calc_fly_power(C.byref(b.arr[i])) for i in range(len(st))]) if len(st) <= 4096 else None
    return dict(reward=r, ret_done=d, info=info, done_after=b.view["done"].astype(bool).copy(), post=post, obs=obs,
                error=b.view["error"].copy(), energy=energy)


def oracle_obs(ctx, state, first=0):
    """state_PathPlan of every agent of the slice, in the state given."""
    st, sub, alias = state
    b = ctx.batch(first, len(st))
    b.set_from_state16(st, sub, alias)
    obs = np.zeros((len(st), po.OBS_DIM))
    for i in range(len(st)):
        b.lib.orc_state_pathplan(C.byref(ctx.world.w), C.byref(b.arr[i]), obs[i].ctypes.data)
    return obs


def fresh_state(ctx, seed, tick, n=None):
    """UAV.reset() of every agent at `tick` as apply_reset defines it: the bank row and heading of reset_draws at the agent's own
    index, speed Max_V, Step 0, done 0, scores 0, the whole list of the row, the alias where the row has a start node."""
    n = ctx.N if n is None else n
    sg, bsub, bns = ctx.bank
    scn, heading = px.reset_draws(n, seed, tick, len(bns))
    st = np.zeros((n, 16))
    st[:, 0:3], st[:, 6:9] = sg[scn, :3], sg[scn, 3:]
    st[:, 3], st[:, 4], st[:, 5] = ctx.max_v * np.cos(heading), ctx.max_v * np.sin(heading), ctx.max_v
    st[:, 11] = bns[scn]
    return (st, bsub[scn].copy(), (bns[scn] >= 2).astype(np.int32)), scn


def obs_err(got, exp):
    return np.abs(np.asarray(got, dtype=np.float64) - exp) / np.maximum(1.0, np.abs(exp))


OBS_BITS = np.r_[11:86, 90:95]


def _worst(stats, key, value, bar):
    stats[key] = max(stats.get(key, 0.0), float(value) / bar)


def check_restarts(ctx, seed, tick, first, st, st1, want, sub1=None, alias1=None, stats=None):
    """The restart set read off what the agents [first, first + n) hold after the launch equals `want`, both ways; every restarted
    agent -- waiting and masked ones included -- holds the bank row and heading of reset_draws(tick) at its own index, Step 0, done
    0, the alias and (where sub1 is given) the whole list as apply_reset defines them; nobody else changed scenario."""
    n = len(st)
    (f_st, f_sub, f_alias), scn = fresh_state(ctx, seed, tick, first + n)
    f_st, f_sub, f_alias = f_st[first:], f_sub[first:], f_alias[first:]
    is_fresh = ((st1[:, 0:3] == f_st[:, 0:3]).all(1) & (st1[:, 6:9] == f_st[:, 6:9]).all(1) & (st1[:, 9] == 0) & (st1[:, 10] == 0)
                & (st1[:, 11] == f_st[:, 11]) & (st1[:, 14] == 0) & (np.abs(st1[:, 3:5] - f_st[:, 3:5]).max(axis=1) <= STATE_TOL))
    assert np.array_equal(is_fresh, want), ("restart set", np.nonzero(is_fresh & ~want)[0][:8], np.nonzero(~is_fresh & want)[0][:8])
    if want.any():
        w = want
        assert np.array_equal(st1[w][:, [9, 10, 12, 13, 14, 15]], np.zeros((int(w.sum()), 6)))
        if sub1 is not None:
            assert np.array_equal(alias1[w], f_alias[w]) and np.array_equal(sub1[w], f_sub[w])  # the whole K x 3 list: the bank row
        err = max(np.abs(st1[w, 3:5] - f_st[w, 3:5]).max(), np.abs(st1[w, 5] - ctx.max_v).max())
        if stats is not None:
            _worst(stats, "state", err, STATE_TOL)
        assert err <= STATE_TOL, ("heading of the reset", err)
    assert np.array_equal(st1[~want, 6:9], st[~want, 6:9])


def check_launch(ctx, rec, obs_tol=OBS_TOL_F32, first=0, model_all=None, apf=False):
    """The assertions of one launch.  rec: flags, active, seed, tick, steer [n], pre / post = (state16, sub, alias) around the
    launch, out = dict(reward, ret_done, agent_done, info, valid, energy or None, obs [n, 100] or None), all for the agents
    [first, first + n) of the env.  model_all: where rec is a window of a larger launch, the dict (restarted, scn_changed) the
    caller took over ALL agents.  -> the model's dict + 'stats' (worst error over bar per quantity)."""
    U, out = ctx.U, rec["out"]
    st, sub, alias = rec["pre"]
    st1, sub1, alias1 = rec["post"]
    n = len(st)
    done = st[:, 10] != 0
    act = None if rec.get("active") is None else np.asarray(rec["active"])[first:first + n]
    orc = oracle_step(ctx, rec["pre"], rec["steer"], first)
    m = tm.launch(U, rec["flags"], done, orc["reward"], orc["ret_done"], orc["info"], orc["done_after"], act)
    s, stats = m["stepping"], {}
    assert not orc["error"][s].any()
    # ---- flags of everyone; waiting and masked agents: info 3, valid 0, ret_done = done
    for name in ("info", "valid", "ret_done", "agent_done"):
        assert np.array_equal(np.asarray(out[name]), m[name]), (name, np.nonzero(np.asarray(out[name]) != m[name])[0][:8])
    assert (m["info"][~s] == tm.INFO_SKIPPED).all() and (m["valid"][~s] == 0).all() and np.array_equal(m["ret_done"][~s] != 0, done[~s])
    assert (np.asarray(out["reward"])[~s] == 0.0).all()
    if s.any():
        err = np.abs(np.asarray(out["reward"])[s] - orc["reward"][s]).max()
        _worst(stats, "reward", err, REWARD_TOL)
        assert err <= REWARD_TOL, ("reward", err)
    # ---- the restart set equal to the model's, both ways; every restarted agent fresh; nobody else changed scenario
    want = m["restarted"]
    check_restarts(ctx, rec["seed"], rec["tick"], first, st, st1, want, sub1, alias1, stats)
    # ---- waiting and masked agents that were not restarted: untouched, bit for bit
    same = ~s & ~want
    assert np.array_equal(st1[same], st[same]) and np.array_equal(sub1[same], sub[same]) and np.array_equal(alias1[same], alias[same])
    # ---- stepping agents that were not restarted: the oracle's post-step state
    keep = s & ~want
    if keep.any():
        o_st, o_sub, o_alias = orc["post"]
        assert np.array_equal(st1[keep][:, [9, 10, 11, 15]], o_st[keep][:, [9, 10, 11, 15]])
        err = max(np.abs(st1[keep, :9] - o_st[keep, :9]).max(), np.abs(st1[keep, 12:15] - o_st[keep, 12:15]).max() / 10.0)
        _worst(stats, "state", err, STATE_TOL)
        assert np.abs(st1[keep, :9] - o_st[keep, :9]).max() <= STATE_TOL
        assert np.abs(st1[keep, 12:15] - o_st[keep, 12:15]).max() <= 1e-8
        assert np.array_equal(alias1[keep], o_alias[keep])
        left = (np.arange(sub1.shape[1])[None, :] < o_st[:, 11][:, None].astype(int)) & keep[:, None]
        if left.any():
            assert np.abs(sub1 - o_sub)[left].max() <= (SUB_TOL if apf else STATE_TOL)
    # ---- the observation of everyone: state_PathPlan of the state the agent holds after the launch
    if out.get("obs") is not None:
        exp = oracle_obs(ctx, rec["post"], first)
        exp[keep] = orc["obs"][keep]                             # (the oracle's own post-step state where it stepped)
        got = np.asarray(out["obs"], dtype=np.float64)
        e = obs_err(got, exp)
        _worst(stats, "obs", e.max(), obs_tol)
        assert e.max() <= obs_tol, ("obs", e.max(), np.unravel_index(e.argmax(), e.shape))
        assert np.array_equal(got[:, OBS_BITS], exp[:, OBS_BITS])
    # ---- energy of the stepping agents: UAV j's Calc_Fly_Power at the post-step speed (before any reset), j = i mod U
    if out.get("energy") is not None and s.any():
        idx = np.nonzero(s)[0]
        ref = tm.fly_power_many(ctx.power, orc["post"][0][idx, 5], tm.uav_slot(first + idx, U))
        if orc["energy"] is not None:                            # (the C oracle's Calc_Fly_Power with A_j, xi_j set per agent agrees)
            assert np.abs(orc["energy"][idx] - ref).max() <= 1e-12 * np.abs(ref).max()
        e = np.abs(np.asarray(out["energy"])[idx] - ref) / np.abs(ref)
        _worst(stats, "energy", e.max(), ENERGY_RTOL)
        assert e.max() <= ENERGY_RTOL, ("energy", e.max(), idx[e.argmax()])
    m["stats"] = stats
    return m


# ------------------------------------------------------------------------------------------------ the device-free stand-in
MUTATIONS = ("any_member_done", "one_launch_late", "mask_not_shifted", "team_is_the_wave", "slot_is_i_div_U", "waiting_redrawn_early",
             "masked_done_not_counted")


def wave_restart(U, agent_done, done_before, active, mutation=None):
    """The restart decision as a wavefront takes it, lane by lane (64 lanes, ballot over the lanes below N), with one of the
    plausible mistakes; mutation None must equal the model."""
    n = len(agent_done)
    act = np.ones(n, bool) if active is None else np.asarray(active).astype(bool)
    src = done_before if mutation == "one_launch_late" else agent_done
    if mutation == "masked_done_not_counted":
        src = src & act
    out = np.zeros(n, bool)
    full = (1 << 64) - 1
    for w0 in range(0, n, 64):
        dm = sum(1 << l for l in range(min(64, n - w0)) if src[w0 + l])
        for l in range(min(64, n - w0)):
            g0 = l & ~(U - 1)
            gm = full if U >= 64 else ((1 << U) - 1) << (0 if mutation == "mask_not_shifted" else g0)
            if mutation == "team_is_the_wave":
                gm = full
            out[w0 + l] = (dm & gm) != 0 if mutation == "any_member_done" else (dm & gm) == gm
    if mutation == "waiting_redrawn_early":
        out |= np.asarray(done_before).astype(bool) & act
    return out


class HostEnv:
    """VecPathPlanEnv's reset / set_state / step on the host: the C oracle for the transition, the team model (or a mutant of
    it) for who steps and who restarts, reset_draws for the restarts."""

    def __init__(self, ctx, mutation=None):
        self.ctx, self.mutation, self.tick, self.seed = ctx, mutation, 0, 0

    def reset(self, seed):
        self.seed = seed
        (self.st, self.sub, self.alias), _ = fresh_state(self.ctx, seed, 0)
        self.tick = 1

    def state(self):
        return self.st.copy(), self.sub.copy(), self.alias.copy()

    def expire(self, who):
        """uavenv_set_state of these agents with Step = max_step - 1: clears done and the scores, keeps the rest."""
        self.st[who, 9] = self.ctx.max_step - 1
        self.st[who, 10] = 0
        self.st[who, 12:16] = 0

    def step(self, steer, flags, active=None):
        ctx, U = self.ctx, self.ctx.U
        pre = self.state()
        done = pre[0][:, 10] != 0
        orc = oracle_step(ctx, pre, steer)
        m = tm.launch(U, flags, done, orc["reward"], orc["ret_done"], orc["info"], orc["done_after"], active)
        s = m["stepping"]
        for mine, theirs in zip((self.st, self.sub, self.alias), orc["post"]):
            mine[s] = theirs[s]
        nk = self.st[:, 11].astype(int)
        self.sub[np.arange(self.sub.shape[1])[None, :] >= nk[:, None]] = 0.0            # get_state pads the list with zeros
        j = np.arange(ctx.N) // U if self.mutation == "slot_is_i_div_U" else tm.uav_slot(np.arange(ctx.N), U)
        energy = tm.fly_power_many(ctx.power, self.st[:, 5], j)
        restart = np.zeros(ctx.N, bool)
        if flags & tm.AUTO_RESET:
            restart = wave_restart(U, m["agent_done"] != 0, done, active,
                                   None if self.mutation == "slot_is_i_div_U" else self.mutation)
        (f_st, f_sub, f_alias), _ = fresh_state(ctx, self.seed, self.tick)
        self.st[restart], self.sub[restart], self.alias[restart] = f_st[restart], f_sub[restart], f_alias[restart]
        out = {k: m[k] for k in ("reward", "ret_done", "agent_done", "info", "valid")}
        out["energy"] = energy
        out["obs"] = oracle_obs(ctx, self.state())
        rec = dict(flags=flags, active=active, seed=self.seed, tick=self.tick, steer=np.asarray(steer, dtype=np.float64), pre=pre,
                   post=self.state(), out=out)
        self.tick += 1
        return rec


def scripted_steer(U, t):
    """The steering of scripted launch t (launch -1 = the plain first step): index actions 0 / 1 / 2 -> -1 / 0 / +1."""
    n = U * N_ENVS[U]
    return -1.0 + np.random.default_rng(100 * U + t + 1).integers(0, 3, n).astype(np.float64)


def run_script(env, U, variant, form, check=None):
    """The script on anything with HostEnv's interface: reset, one plain step, LAUNCHES scripted launches.  check(rec, t) is
    called after every launch.  -> the records."""
    env.reset(SEED)
    recs = [env.step(scripted_steer(U, -1), FLAGS if form != "noskip" else tm.AUTO_RESET)]
    if check:
        check(recs[-1], -1)
    for t in range(LAUNCHES):
        done = env.state()[0][:, 10] != 0
        env.expire(expire_mask(U, variant, form, t, done))
        flags, active = launch_args(U, form, t)
        recs.append(env.step(scripted_steer(U, t), flags, active))
        if check:
            check(recs[-1], t)
    return recs
