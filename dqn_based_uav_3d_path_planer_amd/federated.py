"""The federated merge of the per-UAV trainers that PathPlan_City.run_eposide fires every FL_Loop episodes when Is_FL is set
(Envs/PathPlan_City.py:469-475): Federated_Learning_AC (:590-601) for actor-critic trainers -- the actors of all UAVs are
added up in agent order into a deep copy of agent 0's and every UAV takes the result through replace_param
(Trainer/SAC_Trainer.py:456-459; optimizers, critics and targets stay as they are).

What the reference EXECUTES differs from its comment: the division by len(Agents) at :597 assigns into the dict state_dict()
returned and never reaches the model, so the merged model is the SUM of the actors (tests/golden/federated_ac.npz, generated
by oracle/gen_golden_federated.py, pins that).  `aggregate`:
  "reference"  the sum, as executed -- the drop-in default (<FL_Aggregate> absent);
  "mean"       the sum / number of UAVs -- what the comment at :597 intends and what keeps training stable.

For DQN-family trainers (Is_AC = 0) the reference calls Federated_Learning (:604-640), whose get_policy_DFRL / SPN_param /
Update_SPN_Soft exist on no trainer in the tree (it raises AttributeError): there is no executed behaviour to match, so the
same merge is applied to q_local (replace_param of Trainer/DuelingDQN_Trainer.py:204-207 writes q_local only).

The DQN-family merge the reference DOES execute is Federated_Learning_choice (:644-684; train_off_policy_FL calls it at :706-708,
the commented alternative at :474) -- a SELECTIVE merge, <FL_Aggregate>choice</FL_Aggregate> here: for p = 0 .. U-1 in order, each
step on the models as the earlier steps left them, UAV p forwards 10 of its own replayed states through every q_local, sorts the
other UAVs by mean((q_p - q_j)^2) (stable), and becomes the mean of itself and the closest (U-1)//2 of them: f32 adds in that order,
then a true division.  q_local only (replace_param); the q_target average the reference also computes is thrown away.
tests/golden/federated_choice.npz (scripts/gen_golden_fl_choice.py) pins it; choice_merge_modules is the torch form,
choice_merge_blocks the one-launch device form (csrc/fed.hip: uavenv_fed_choice).

Fused trainers (flat f32 parameter blocks in HBM) merge in ONE launch (csrc/fed.hip: uavenv_fed_aggregate, summation in the
reference's agent order -> bit-identical to torch's f32 adds); anything else merges through torch on whatever device it is."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

AGGREGATES = ("reference", "mean")
SELECTIVE = ("choice",)            # merges that pick their partners: not a scale of the sum, so _scale refuses them
CHOICE_STATES = 10                 # replay_memory.sample(10), :655


def _scale(aggregate: str, n: int) -> float:
    if aggregate not in AGGREGATES:
        raise ValueError(f"FL_Aggregate {aggregate!r}: expected one of {AGGREGATES}")
    return 1.0 if aggregate == "reference" else 1.0 / n


def merge_blocks(blocks: Sequence[torch.Tensor], scale: float, n_floats: int = None) -> None:
    """Every flat f32 block <- scale * (blocks[0] + blocks[1] + ...) on the device, one launch (uavenv_fed_aggregate).
    Fails loudly without the HIP library / a GPU: there is no CPU path here (merge_modules is the torch form)."""
    from . import _lib
    lib = _lib.load()
    n = len(blocks)
    if not 1 <= n <= _lib.FED_MAX_BLOCKS:
        raise ValueError(f"{n} blocks: uavenv_fed_aggregate takes 1..{_lib.FED_MAX_BLOCKS}")
    n_floats = int(blocks[0].numel() if n_floats is None else n_floats)
    for b in blocks:
        if not (b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and b.numel() >= n_floats and b.device == blocks[0].device):
            raise ValueError("blocks must be contiguous f32 CUDA tensors of one device")
    arr = (C.c_void_p * n)(*[b.data_ptr() for b in blocks])
    _lib.check(lib.uavenv_fed_aggregate(arr, n, n_floats, float(scale), torch.cuda.current_stream(blocks[0].device).cuda_stream),
               "uavenv_fed_aggregate")


def merge_modules(modules: Sequence[torch.nn.Module], scale: float) -> None:
    """The same merge through torch, parameter by parameter in agent order (:593-596), written back with copy_ (:458-459)."""
    with torch.no_grad():
        for ps in zip(*[list(m.parameters()) for m in modules]):
            total = ps[0].detach().clone()
            for p in ps[1:]:
                total += p.detach().to(total.device)
            if scale != 1.0:
                total *= scale
            for p in ps:
                p.copy_(total.to(p.device))


def federated_learning_ac(trainers: Sequence, aggregate: str = "reference") -> str:
    """Federated_Learning_AC over `trainers` (objects with .actor, optionally .learner with the fused flat blocks).
    -> "device" when the one-launch kernel ran, "torch" otherwise."""
    scale = _scale(aggregate, len(trainers))
    learners = [getattr(t, "learner", None) for t in trainers]
    if len(trainers) <= 8 and all(getattr(t, "fused", False) and hasattr(L, "_blocks") for t, L in zip(trainers, learners)) \
            and len({L._blocks.device for L in learners}) == 1 and len({id(L) for L in learners}) == len(learners):
        from . import _lib
        merge_blocks([L._blocks[0] for L in learners], scale, n_floats=_lib.SAC_ACTOR_PARAMS)
        return "device"
    merge_modules([t.actor for t in trainers], scale)
    return "torch"


def federated_learning_q(trainers: Sequence, aggregate: str = "reference") -> str:
    """The merge applied to q_local of DQN-family trainers (see the module docstring)."""
    scale = _scale(aggregate, len(trainers))
    learners = [getattr(t, "learner", None) for t in trainers]
    if len(trainers) <= 8 and all(getattr(t, "fused", False) and hasattr(L, "flat") and hasattr(L, "P") for t, L in zip(trainers, learners)) \
            and len({L.flat.device for L in learners}) == 1 and len({L.P for L in learners}) == 1 \
            and len({id(L) for L in learners}) == len(learners):
        merge_blocks([L.flat[0] for L in learners], scale, n_floats=learners[0].P)
        return "device"
    merge_modules([t.q_local for t in trainers], scale)
    return "torch"


def choice_merge_modules(modules: Sequence[torch.nn.Module], states: Sequence[torch.Tensor]) -> list:
    """Federated_Learning_choice (:644-684) through torch on whatever device the modules live: states[p] is the [S, w] float
    batch UAV p replayed.  Sequential in p (step p sees what steps 0 .. p-1 wrote), MSELoss distances, a stable sort, adds in
    chosen order, and a division by a TENSOR: torch divides by a Python scalar on the GPU by multiplying with its reciprocal,
    which differs from the reference's CPU division in about a third of the elements when the divisor is 3.
    Writes the modules' parameters in place; -> the chosen lists, one per module."""
    U = len(modules)
    if len(states) != U:
        raise ValueError(f"{len(states)} state batches for {U} modules: one per UAV")
    chosen_all = []
    with torch.no_grad():
        params = [list(m.parameters()) for m in modules]
        for p in range(U):
            dev = params[p][0].device
            x = states[p].to(dev)
            q_p = modules[p](x)
            others = [j for j in range(U) if j != p]
            if others:
                d = torch.stack([torch.nn.functional.mse_loss(q_p, modules[j](x.to(params[j][0].device)).to(dev))
                                 for j in others]).tolist()
            else:
                d = []
            order = sorted(range(len(others)), key=lambda i: d[i])           # stable: ties keep the index order
            chosen = [others[i] for i in order[:len(others) // 2]]
            chosen_all.append(chosen)
            if not chosen:
                continue                                                     # t / 1 is t
            for i, w in enumerate(params[p]):
                t = w.detach().clone()
                for j in chosen:
                    t += params[j][i].detach().to(dev)
                w.copy_(t / t.new_full((1,), float(len(chosen) + 1)))
    return chosen_all


def draw_slot_pairs(ring, n_slots: int, batch: int, seed: int, counter: int) -> torch.Tensor:
    """`batch` (frame, agent) pairs per UAV slot over the VALID rows of a multi-UAV ring, one launch (uavenv_replay_draw_slots):
    int32 [n_slots, batch, 2] on the ring's device.  Does not synchronise."""
    from . import _lib
    lib = _lib.load()
    n = int(ring.obs.shape[1])
    if n % n_slots or ring.filled <= 0 or batch <= 0:
        raise ValueError("draw_slot_pairs: an empty ring, or agents that do not divide into the slots")
    out = torch.empty((n_slots, batch, 2), dtype=torch.int32, device=ring.obs.device)
    _lib.check(lib.uavenv_replay_draw_slots(ring.frames, n // n_slots, ring.head, ring.filled, batch, n_slots, ring.valid.data_ptr(),
                                            _lib.DRAW_MAX_TRIES, int(seed) & (2 ** 64 - 1), int(counter), out.data_ptr(),
                                            torch.cuda.current_stream(out.device).cuda_stream), "uavenv_replay_draw_slots")
    return out


def choice_merge_blocks(learners, obs: torch.Tensor, pairs: torch.Tensor):
    """The selective merge on the device, ONE launch (uavenv_fed_choice): learners = one FusedDQNLearner per UAV slot, obs = the
    packed ring rows (int32 [frames, n_agents, 20]), pairs = int32 [U, S, 2] (frame, agent) of the S <= 16 states UAV p replays
    (draw_slot_pairs' layout).  Every argument is checked before anything is enqueued.  -> (dist f32 [U, U], chosen int32 [U, U]
    padded with -1, status int32 [1]) on the device: status 1 = a pair out of range, nothing merged.  Does not synchronise."""
    from . import _lib
    from .learner import check_slot_learners
    ls = check_slot_learners(learners)
    U = len(ls)
    if not (torch.is_tensor(obs) and obs.is_cuda and obs.dtype == torch.int32 and obs.dim() == 3 and obs.shape[2] == _lib.PACKED_DWORDS
            and obs.is_contiguous() and obs.shape[0] > 0 and obs.shape[1] > 0):
        raise ValueError("choice_merge_blocks takes contiguous packed ring rows (int32 [frames, n_agents, 20]) on the GPU")
    if not (torch.is_tensor(pairs) and pairs.dtype == torch.int32 and pairs.dim() == 3 and pairs.shape[0] == U and pairs.shape[2] == 2
            and 1 <= pairs.shape[1] <= _lib.FED_CHOICE_MAX_STATES and pairs.is_contiguous() and pairs.device == obs.device):
        raise ValueError(f"pairs: contiguous int32 [{U}, 1..{_lib.FED_CHOICE_MAX_STATES}, 2] on the device of obs")
    if any(L.flat.device != obs.device for L in ls):
        raise ValueError("the learners' parameter blocks and obs must live on one device")
    if len({L.flat.data_ptr() for L in ls}) != U:
        raise ValueError("two learners share a parameter block")
    lib = _lib.load()
    nets = (C.POINTER(_lib.UavDqnNet) * U)(*[C.pointer(L.net) for L in ls])
    dist = torch.zeros((U, U), dtype=torch.float32, device=obs.device)
    chosen = torch.full((U, U), -1, dtype=torch.int32, device=obs.device)
    status = torch.zeros(1, dtype=torch.int32, device=obs.device)
    _lib.check(lib.uavenv_fed_choice(obs.data_ptr(), int(obs.shape[0]), int(obs.shape[1]), pairs.data_ptr(), int(pairs.shape[1]), nets, U,
                                     dist.data_ptr(), chosen.data_ptr(), status.data_ptr(),
                                     torch.cuda.current_stream(obs.device).cuda_stream), "uavenv_fed_choice")
    return dist, chosen, status


def federated_learning_choice(trainers: Sequence, *, states=None, obs=None, pairs=None, info: dict = None) -> str:
    """Federated_Learning_choice over `trainers` (objects with .q_local, optionally .learner).  The device form when every trainer is
    fused with distinct f32-MFMA FusedDQNLearners of one head on one device and `obs` / `pairs` are given (-> "device"; info, when a
    dict, receives the dist / chosen / status device tensors), the torch form on `states` otherwise (-> "torch"; info["chosen"] = the
    chosen lists)."""
    learners = [getattr(t, "learner", None) for t in trainers]
    if obs is not None and pairs is not None and 1 <= len(trainers) <= 8 \
            and all(getattr(t, "fused", False) and all(hasattr(L, a) for a in ("net", "flat", "n_actions", "dueling", "mfma"))
                    for t, L in zip(trainers, learners)) \
            and all(L.mfma == "f32" for L in learners) and len({id(L) for L in learners}) == len(learners) \
            and len({(L.n_actions, bool(L.dueling)) for L in learners}) == 1 and len({L.flat.device for L in learners}) == 1:
        dist, chosen, status = choice_merge_blocks(learners, obs, pairs)
        if info is not None:
            info.update(dist=dist, chosen=chosen, status=status)
        return "device"
    if states is None:
        raise ValueError("federated_learning_choice: the torch form needs `states` (one [S, w] batch per trainer)")
    chosen = choice_merge_modules([t.q_local for t in trainers], states)
    if info is not None:
        info.update(chosen=chosen)
    return "torch"
