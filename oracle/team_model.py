"""Host model of what binds the U agents of one env together in a step launch, written from the reference and
include/uavenv.h (not from the kernels):

  * who steps     Envs/PathPlan_City.py:365-366: a finished agent waits for its team-mates (UAVENV_STEP_SKIP_DONE); an agent the
                  `active` mask leaves out is not touched either.  Both report info SKIPPED, valid 0, ret_done = done;
  * who restarts  PathPlan_City.py:252-259, 416-417: the env restarts when ALL of its U agents are done, and under
                  UAVENV_STEP_AUTO_RESET it does so in the launch that completes it -- every agent of it, the waiting and the masked
                  ones included, is then a fresh UAV.reset() (oracle.philox.reset_draws at the launch's tick).  A masked agent that
                  is done counts towards its team being complete; a masked agent that is not done blocks the restart;
  * whose power   Agents/UAV.py:55,58: UAV j of a team flies with A + 0.03 j and xi = 0.8 + 0.02 j, j = agent index mod U.

Agent i belongs to env i // U.  Pure numpy, no torch, no device; one function per launch (launch)."""
from __future__ import annotations

import math

import numpy as np

AUTO_RESET, SKIP_DONE = 1, 2          # UAVENV_STEP_AUTO_RESET, UAVENV_STEP_SKIP_DONE
INFO_SKIPPED = 3                      # UAVENV_INFO_SKIPPED
TEAM_SIZES = (1, 2, 4, 8, 16, 32, 64)


def _mask(active, n):
    return np.ones(n, bool) if active is None else np.asarray(active).astype(bool)


def who_steps(flags: int, done, active=None):
    """bool [N]: the agents update_PathPlan is called for."""
    done = np.asarray(done).astype(bool)
    waits = done if flags & SKIP_DONE else np.zeros(len(done), bool)
    return _mask(active, len(done)) & ~waits


def launch(U: int, flags: int, done, reward, ret_done, info, done_after, active=None) -> dict:
    """One step launch.  done: the agents' done flags BEFORE it; reward / ret_done / info / done_after [N]: each agent's transition
    as the C oracle gives it (read only where the agent steps).  -> dict of [N] arrays stepping, info, valid, ret_done, agent_done,
    reward, restarted (the agents whose post-step state must be a fresh reset) and restart_envs [N / U]."""
    done = np.asarray(done).astype(bool)
    n = len(done)
    assert U in TEAM_SIZES and n % U == 0
    step = who_steps(flags, done, active)
    agent_done = np.where(step, np.asarray(done_after).astype(bool), done)
    envs = agent_done.reshape(-1, U).all(axis=1) if flags & AUTO_RESET else np.zeros(n // U, bool)
    return dict(stepping=step,
                info=np.where(step, np.asarray(info), INFO_SKIPPED).astype(np.uint8),
                valid=step.astype(np.uint8),
                ret_done=np.where(step, np.asarray(ret_done) != 0, done).astype(np.uint8),
                agent_done=agent_done.astype(np.uint8),
                reward=np.where(step, np.asarray(reward, dtype=np.float64), 0.0),
                restart_envs=envs, restarted=np.repeat(envs, U))


def uav_slot(i, U: int):
    """j of agent i: its place in its team (Agents/UAV.py: self.j)."""
    return np.asarray(i) % U


def slot_power_params(power8, j):
    """(A_j, xi_j) of UAV j, Agents/UAV.py:55,58; power8 = P_i v_0 d_0 rho s A P_b F_b."""
    j = np.asarray(j, dtype=np.float64)
    return float(power8[5]) + 0.03 * j, 0.8 + 0.02 * j


def fly_power(power8, V: float, j: int) -> float:
    """Calc_Fly_Power of UAV j at speed V (already clamped), Agents/UAV.py:239-245 in Python floats (float64)."""
    P_i, v_0, d_0, rho, s, _, P_b, F_b = (float(x) for x in power8[:8])
    A, xi = float(power8[5]) + 0.03 * int(j), 0.8 + 0.02 * int(j)
    V = float(V)
    induced = P_i * math.sqrt(math.sqrt(1 + (V ** 4) / (4 * (v_0 ** 4))) - (V ** 2) / (2 * (v_0 ** 2)))
    parasite = 0.5 * d_0 * rho * s * A * (V ** 3)
    blade = xi * P_b * (1 + 3 * (V ** 2) / (F_b ** 2))
    return induced + parasite + blade


def fly_power_many(power8, V, j) -> np.ndarray:
    return np.array([fly_power(power8, v, jj) for v, jj in zip(np.asarray(V).ravel(), np.asarray(j).ravel())])
