"""Generate tests/golden/federated_choice.npz by EXECUTING the reference's Federated_Learning_choice
(Envs/PathPlan_City.py:644-684) on a scratch copy (oracle/ref_harness.RefSession): FIVE DuelingDQN_Trainers -- VAnet2 100-64-3, the
only reference trainer with replace_param; with five, two others are chosen and the divisor is 3, the one that tells a true
division from a multiplication by the reciprocal -- with injected q_local / q_target weights, hung on the env's Agents list.
Each trainer's replay_memory is a stub whose sample(10) returns 10 injected observation rows: rows the reference's own
state_PathPlan produced (tests/golden/episodes.npz), so they are packed-representable and the device kernel can read EXACTLY
the inputs the executed method saw.

The q_local weights are a one-parameter family base + c_j * D with well-separated c_j: merges stay inside the family, so the
distances of every step stay well apart (tests/test_federated_choice.py asserts the gap in float64) and the executed choice
does not hang on rounding.

Recorded: every q_local and q_target before and after; the states; per step p -- recomputed inside the stub's sample(), i.e. on
the models as step p finds them, with the reference's own torch operations -- the distances and the chosen indices.

TEST INFRASTRUCTURE: run where the reference tree exists, never on a GPU machine."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
from ref_harness import RefSession  # noqa: E402

N_AGENTS, N_STATES, W, HID, A = 5, 10, 100, 64, 3
C_J = (0.0, 1.0, 2.6, 4.9, 8.3)          # the family's coordinates: no two differences |c_p - c_j| close to each other


def sd_to_np(sd):
    return {k: v.detach().cpu().numpy().copy() for k, v in sd.items()}


def main():
    s = RefSession()
    try:
        from FactoryClass.TrainerFactory import TrainerFactory
        param = {"Trainer_Type": "DuelingDQN_Trainer", "NetWork": "VAnet2", "w": str(W), "hiden_dim": str(HID), "output": str(A),
                 "h": "1", "channel": "1", "Batch_Size": "64", "LEARNING_RATE": "0.001", "gamma": "0.99", "replay_size": "1000",
                 "save_loop": str(10 ** 9), "Update_loop": "3", "Is_Train": "1", "name": "golden"}
        ep = np.load(os.path.join(OUT, "episodes.npz"))
        rng = np.random.default_rng(31)
        pick = rng.choice(len(ep["obs"]), N_AGENTS * N_STATES, replace=False)
        states = ep["obs"][pick].astype(np.float32).reshape(N_AGENTS, N_STATES, W)
        g = torch.Generator().manual_seed(4242)
        agents, out, dist, chosen = [], {}, np.zeros((N_AGENTS, N_AGENTS), np.float32), []
        base = direction = None

        class StubMemory:
            """replay_memory.sample(10) -> UAV p's injected rows; the call happens at the top of step p (:655), so the distances
            recomputed here see the models exactly as the step does."""

            def __init__(self, p):
                self.p = p

            def sample(self, n):
                assert n == N_STATES
                x = torch.from_numpy(states[self.p])
                mse = torch.nn.MSELoss()
                with torch.no_grad():
                    q_p = agents[self.p].Trainer.q_local(x)
                    pairs = []
                    for j in range(N_AGENTS):
                        if j != self.p:
                            d = mse(q_p, agents[j].Trainer.q_local(x))
                            dist[self.p, j] = float(d)
                            pairs.append([j, d])
                srt = sorted(pairs, key=lambda t: t[1])
                chosen.append([t[0] for t in srt[:len(srt) // 2]])
                zero = torch.zeros(1, 1)
                return [(x[i:i + 1], zero, zero, x[i:i + 1], zero) for i in range(N_STATES)]

        for j in range(N_AGENTS):
            tr = TrainerFactory().Create_Trainer(dict(param, name=f"golden{j}"))
            assert tr is not None and hasattr(tr, "replace_param")
            if base is None:
                base = [torch.randn(p.shape, generator=g) * 0.15 for p in tr.q_local.parameters()]
                direction = [torch.randn(p.shape, generator=g) * 0.02 for p in tr.q_local.parameters()]
            with torch.no_grad():
                for p, b, d in zip(tr.q_local.parameters(), base, direction):
                    p.copy_(b + np.float32(C_J[j]) * d)
                for p in tr.q_target.parameters():
                    p.copy_(torch.randn(p.shape, generator=g) * 0.12)
            for pref, sd in ((f"l{j}_before_", tr.q_local.state_dict()), (f"t{j}_before_", tr.q_target.state_dict())):
                for k, v in sd_to_np(sd).items():
                    out[pref + k] = v
            tr.replay_memory = StubMemory(j)
            agents.append(types.SimpleNamespace(Trainer=tr))
        env = s.env
        env.Agents = agents
        type(env).Federated_Learning_choice(env)                  # Envs/PathPlan_City.py:644-684
        for j, a in enumerate(agents):
            for pref, sd in ((f"l{j}_after_", a.Trainer.q_local.state_dict()), (f"t{j}_after_", a.Trainer.q_target.state_dict())):
                for k, v in sd_to_np(sd).items():
                    out[pref + k] = v
        keys = list(agents[0].Trainer.q_local.state_dict().keys())
        print("chosen:", chosen)
        print("distances:\n", dist)
        print("targets unchanged:", all(np.array_equal(out[f"t{j}_before_{k}"], out[f"t{j}_after_{k}"])
                                        for j in range(N_AGENTS) for k in keys))
        out.update(n_agents=np.int64(N_AGENTS), states=states, episode_rows=pick, dist=dist,
                   chosen=np.array(chosen, dtype=np.int64), keys=np.array(keys), c_j=np.array(C_J))
        np.savez_compressed(os.path.join(OUT, "federated_choice.npz"), **out)
    finally:
        s.close()


if __name__ == "__main__":
    main()
