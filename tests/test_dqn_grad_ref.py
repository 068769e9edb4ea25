"""oracle/dqn_grad_ref.py -- the float64 gradient bucket every DQN gradient kernel is held against in
tests/test_dqn_grad_kernels_gpu.py -- pinned on the CPU two ways:
  * against torch autograd in float64 on random nets and batches (every kind, MSE / Huber, with and without importance
    weights, some valid = 0 rows): 1e-12 relative;
  * against the EXECUTED reference trainers (tests/golden/learner_*.npz, learner_*_packed.npz): seven updates of the f64 bucket
    + adam_step_f64 with a hard target copy every 3 reproduce the golden losses (2e-5 relative) and weights (5e-6), the bars
    the kernels meet."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle.dqn_grad_ref import adam_step_f64, dqn_grad_f64, layout, sample_contribution, unflatten

KINDS = [("dqn", False), ("ddqn", False), ("dueling", True)]


def _torch_bucket(b, local, target, kind, dueling, A, gamma, huber, isw):
    """The same bucket by autograd on float64 tensors: sum_s w_s valid_s loss_s, differentiated."""
    n2 = A + (1 if dueling else 0)
    W1, b1, W2, b2 = (torch.tensor(x, requires_grad=True) for x in unflatten(local, 100, 64, n2))
    T1, c1, T2, c2 = (torch.tensor(x) for x in unflatten(target, 100, 64, n2))

    def q(X, W1, b1, W2, b2):
        out = torch.relu(X @ W1.T + b1) @ W2.T + b2
        if dueling:
            return out[:, A:A + 1] + out[:, :A] - out[:, :A].mean(1, keepdim=True)
        return out
    X, X2 = torch.tensor(b["s"]), torch.tensor(b["s2"])
    act = torch.tensor(b["actions"]).long().view(-1, 1)
    qa = q(X, W1, b1, W2, b2).gather(1, act).view(-1)
    with torch.no_grad():
        qt = q(X2, T1, c1, T2, c2)
        if kind == "dqn":
            qn = qt.max(1)[0]
        else:
            qn = qt.gather(1, q(X2, W1, b1, W2, b2).max(1)[1].view(-1, 1)).view(-1)
        y = torch.tensor(b["rewards"]) + gamma * qn * (1 - torch.tensor(b["dones"]))
    if huber:
        per = torch.nn.functional.smooth_l1_loss(qa, y, reduction="none")
    else:
        per = (qa - y) ** 2
    sc = torch.tensor(b["valid"]) * (torch.ones_like(per) if isw is None else torch.tensor(isw))
    loss = (per * sc).sum()
    loss.backward()
    g = torch.cat([W1.grad.reshape(-1), b1.grad, W2.grad.reshape(-1), b2.grad]).numpy()
    return g, float(loss.detach()), (qa - y).detach().abs().numpy()


@pytest.mark.parametrize("kind,dueling", KINDS)
@pytest.mark.parametrize("huber", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_bucket_matches_float64_autograd(kind, dueling, huber, weighted):
    rng = np.random.default_rng([("dqn", "ddqn", "dueling").index(kind), int(huber), int(weighted)])
    A, B, gamma = 3, 96, 0.99
    n2 = A + (1 if dueling else 0)
    P = layout(100, 64, n2)[3]
    local = rng.normal(0, 0.1, P)
    target = local + rng.normal(0, 0.05, P)
    b = dict(s=rng.normal(0, 1, (B, 100)), s2=rng.normal(0, 1, (B, 100)), actions=rng.integers(0, A, B),
             rewards=rng.normal(0, 2, B), dones=(rng.random(B) < 0.25).astype(np.float64),
             valid=(rng.random(B) < 0.8).astype(np.float64))
    isw = rng.uniform(0.1, 1.0, B) if weighted else None
    kw = dict(kind=kind, dueling=dueling, n_actions=A, gamma=gamma, huber=huber)
    r = dqn_grad_f64(b["s"], b["s2"], b["actions"], b["rewards"], b["dones"], b["valid"], local, target, is_weights=isw,
                     per_sample=True, **kw)
    g, loss, abs_td = _torch_bucket(b, local, target, kind, dueling, A, gamma, huber, isw)
    if huber:     # both branches of smooth-L1 are present
        assert (abs_td < 1).any() and (abs_td >= 1).any()
    assert np.abs(r["grad"] - g).max() <= 1e-12 * np.abs(g).max()
    assert abs(r["loss"] - loss) <= 1e-12 * abs(loss)
    assert r["count"] == b["valid"].sum()
    assert np.allclose(r["abs_td"], abs_td, rtol=1e-12, atol=0)
    # the bounds' ingredients: M bounds |grad| componentwise; per-sample contributions add up to the bucket, and the one
    # of sample i is what sample_contribution returns
    assert np.all(np.abs(r["grad"]) <= r["M"] * (1 + 1e-12))
    assert np.abs(r["per_sample_grad"].sum(0) - r["grad"]).max() <= 1e-12 * np.abs(g).max()
    bb = dict(b, is_weights=isw)
    c = sample_contribution(bb, 5, local=local, target=target, **kw)
    assert np.abs(c["grad"] - r["per_sample_grad"][5]).max() <= 1e-14 * np.abs(g).max()
    # the root-sum-square sensitivities to errors in the deltas, by brute force (MSE: contribution_s is linear in delta_s); the
    # dueling head's |.|-backward sums |coef_a W2_aj| over a, an upper bound
    if not huber:
        dd = r["per_sample_grad"] / r["abs_td"][:, None] * r["q_abs"][:, None]
        u = rng.normal(0, 1, g.size)
        want_n2, want_dir = (dd ** 2).sum(0), np.abs(dd) @ np.abs(u)
        sm, sd, _ = r["dir_sens"](u)
        if dueling:
            assert np.all(r["N2"] >= want_n2 * (1 - 1e-10)) and np.all(sd >= want_dir * (1 - 1e-10))
        else:
            assert np.allclose(r["N2"], want_n2, rtol=1e-10, atol=0)
            assert np.allclose(sd, want_dir, rtol=1e-10, atol=0)
        assert np.array_equal(sm, r["M"] * np.abs(u))
    # with valid = 0 a row contributes nothing, whatever it holds
    v0 = int(np.flatnonzero(b["valid"] == 0)[0])
    b2 = {k: v.copy() for k, v in b.items()}
    b2["s"][v0] *= 3.0
    b2["rewards"][v0] = 150.0
    r2 = dqn_grad_f64(b2["s"], b2["s2"], b2["actions"], b2["rewards"], b2["dones"], b2["valid"], local, target,
                      is_weights=isw, **kw)
    assert np.abs(r2["grad"] - r["grad"]).max() <= 1e-14 * np.abs(g).max() and r2["count"] == r["count"]


def test_ddqn_tie_takes_the_first_maximum():
    """Q_local(s') tied exactly between actions 0 and 1 (identical fc2 rows and biases): a' = 0, as torch.max."""
    rng = np.random.default_rng(3)
    P = layout(100, 64, 3)[3]
    local = rng.normal(0, 0.1, P)
    o_w2, o_b2 = layout(100, 64, 3)[1:3]
    local[o_w2 + 64:o_w2 + 128] = local[o_w2:o_w2 + 64]
    local[o_b2 + 1] = local[o_b2]
    local[o_b2 + 2] = -50.0
    target = local.copy()
    target[o_b2 + 1] += 5.0                       # picking action 1 would move y by 0.99 * 5
    B = 8
    s2 = rng.normal(0, 1, (B, 100))
    r = dqn_grad_f64(rng.normal(0, 1, (B, 100)), s2, np.zeros(B), np.zeros(B), np.zeros(B), np.ones(B), local, target,
                     kind="ddqn", dueling=False, n_actions=3, gamma=0.99, huber=False)
    assert np.all(r["a_next"] == 0)
    r_tie = dqn_grad_f64(rng.normal(0, 1, (B, 100)), s2, np.zeros(B), np.zeros(B), np.zeros(B), np.ones(B), local, target,
                         kind="ddqn", dueling=False, n_actions=3, gamma=0.99, huber=False, tie_eps=2.0 ** -16)
    assert r_tie["near_tie"].all() and np.allclose(r_tie["td_amb"], 0.99 * 5.0)


GOLDEN = [("DQN_Trainer", "dqn", False), ("DDQN_Trainer", "ddqn", False), ("DuelingDQN_Trainer", "dueling", True)]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("ref_name,kind,dueling", GOLDEN)
def test_reference_replays_the_executed_trainers(ref_name, kind, dueling, packed):
    g = load_golden(f"learner_{ref_name}{'_packed' if packed else ''}.npz")
    keys = ["fc1.weight", "fc1.bias"] + (["fc_A.weight", "fc_V.weight", "fc_A.bias", "fc_V.bias"] if dueling
                                         else ["fc2.weight", "fc2.bias"])

    def flat(pref):
        return np.concatenate([g[pref + k].astype(np.float64).ravel() for k in keys])
    w, t = flat("l0_"), flat("t0_")
    m, v = np.zeros_like(w), np.zeros_like(w)
    B = len(g["actions"])
    losses = []
    for epoch in range(1, len(g["losses"]) + 1):
        r = dqn_grad_f64(g["states"], g["next_states"], g["actions"], g["rewards"], g["dones"], np.ones(B), w, t,
                         kind=kind, dueling=dueling, n_actions=3, gamma=0.99, huber=False)
        losses.append(r["loss"] / r["count"])
        hard = epoch % 3 == 0
        w, m, v, t = adam_step_f64(w, m, v, r["grad"] / r["count"], epoch, 1e-3, hard=hard, target=t)
    assert epoch == int(g["epoch"])
    assert np.allclose(losses, g["losses"], rtol=2e-5, atol=0), (losses, g["losses"])
    assert np.abs(w - flat("l1_")).max() <= 5e-6
    assert np.abs(t - flat("t1_")).max() <= 5e-6


def test_adam_step_matches_torch_adam_in_float64():
    rng = np.random.default_rng(7)
    n = 50
    p = torch.tensor(rng.normal(0, 1, n), requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3)
    w, m, v = p.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        gr = rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 2, n)
        p.grad = torch.tensor(gr)
        opt.step()
        w, m, v, _ = adam_step_f64(w, m, v, gr, t, 1e-3)
    assert np.allclose(w, p.detach().numpy(), rtol=1e-12, atol=1e-15)
    assert np.allclose(m, opt.state[p]["exp_avg"].numpy(), rtol=1e-12, atol=0)
    assert np.allclose(v, opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
