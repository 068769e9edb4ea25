"""uavenv_fed_choice (k_fed_choice, csrc/fed.hip): the selective federated merge of the DQN slot learners in one launch, held to
float64 (tests/fed_choice_ref.py, oracle.dqn_grad_ref.forward_f64), to the executed reference
(tests/golden/federated_choice.npz) and to a host f32 replay.

Cases: U in {1, 2, 3, 5, 8} (k = 0, 0, 1, 2, 3; divisors 1, 1, 2, 3, 4) x S in {1, 10, 16} x heads 3 plain / 3 dueling / 9 dueling,
nets from the one-parameter family base + c_j D, on two rings:
  "episodes"  rows the reference's state_PathPlan produced, packed into a [3, 40] ring -- known without a GPU, so the gap condition
              (c) of every case is asserted in tests/test_federated_choice.py on exactly these rows;
  "pool"      the packed ring the environment itself wrote (tests/dqn_fixtures.Pool: 5 frames x 2048 agents, wrapped); its rows
              exist on the GPU only, so their gap condition is asserted here, on the float64 forward, before the choice is compared
              (smallest margin seen: 4.56 bars of 4; the episodes ring: 5.50).
The pairs touch frame 0, the last frame, agent 0 and agent n_agents - 1.
 (a) every distance against float64 at the bar |d_out - d| <= mean(2 |e| beta + beta^2) + 2^-16 d of fed_choice_ref;
 (b) chosen_out[p] = the stable sort of the kernel's OWN dist_out[p], exactly, padded with -1;
 (c) with the gap condition, (a) and (b) pin the choice to the float64 choice;
 (d) every `local` block = a host f32 replay on the kernel's own chosen lists (sequential in p, adds in chosen order, a true
     division), torch.equal; target / m / v and 132 sentinel floats behind every block untouched; on the golden's inputs every
     agent's after-state is the executed reference's, bit for bit;
 (e) exact ties; (f) status, every refusal, nullable outputs; (g) the plugin's fused-slots path.
Worst |d_out - d| / bar seen on an MI355X (the module prints them at its end): episodes 0.0010, pool 0.0011, golden 0.0002 -- the
bar is the forward's worst-case bound on |q|-mass, the kernel's f32 forward sits three orders of magnitude inside it."""
import ctypes as C
import re
import types

import numpy as np
import pytest
import torch

import fed_choice_ref as R
from conftest import load_golden, pack_obs_rows
from dqn_fixtures import Pool, golden_flat
from test_federated_choice import refusals

pytestmark = pytest.mark.gpu

SENT, PAD = 7.25, 132                                            # sentinel floats behind every block (a multiple of 4: alignment)
WORST = {}


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    print("worst |d_out - d| / bar:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    p.env.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def episodes():
    rows = R.episode_ring(load_golden("episodes.npz")["obs"])
    packed = pack_obs_rows(rows.reshape(-1, 100)).reshape(R.RING_FRAMES, R.RING_AGENTS, 20)
    return rows, torch.tensor(packed, device="cuda").contiguous()


class Blocks:
    """U nets of one head: local / target / m / v blocks on the device, each followed by PAD sentinel floats."""

    def __init__(self, flats, A, dueling, mfma=None):
        L = _lib()
        self.U, self.A, self.dueling, self.P = len(flats), A, dueling, flats[0].size
        self.stride = ((self.P + 3) & ~3) + PAD
        rng = np.random.default_rng(9)
        host = np.full((self.U, 4, self.stride), SENT, dtype=np.float32)
        for j, f in enumerate(flats):
            host[j, 0, :self.P] = f
            host[j, 1:, :self.P] = rng.normal(0, 1, (3, self.P)).astype(np.float32)
        self.before = host.copy()
        self.buf = torch.tensor(host, device="cuda")
        self.nets = [L.UavDqnNet(*[self.buf[j, r].data_ptr() for r in range(4)], 100, 64, A, 1 if dueling else 0,
                                 L.MFMA_F32 if mfma is None else mfma, 0) for j in range(self.U)]

    def array(self):
        return (C.POINTER(_lib().UavDqnNet) * self.U)(*[C.pointer(n) for n in self.nets])

    def host(self):
        return self.buf.cpu().numpy()

    def locals(self, host=None):
        host = self.before if host is None else host
        return [host[j, 0, :self.P].copy() for j in range(self.U)]

    def check_rest(self, after):
        """target, m, v and every sentinel are what they were."""
        assert np.array_equal(after[:, 1:], self.before[:, 1:]) and np.array_equal(after[:, 0, self.P:], self.before[:, 0, self.P:])


def run(blocks, obs, pairs, want=True, expect=0, n_states=None):
    """-> (dist [U, U], chosen [U, U], status) as numpy; outputs sentinel-filled, with a guard row behind them."""
    L, U = _lib(), blocks.U
    pr = torch.tensor(np.ascontiguousarray(pairs, dtype=np.int32), device="cuda")
    dist = torch.full((U + 1, U), float("nan"), device="cuda")
    chosen = torch.full((U + 1, U), -7, dtype=torch.int32, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    rc = L.load().uavenv_fed_choice(obs.data_ptr(), int(obs.shape[0]), int(obs.shape[1]), pr.data_ptr(),
                                    int(pairs.shape[1]) if n_states is None else n_states, blocks.array(), U,
                                    dist.data_ptr() if want else None, chosen.data_ptr() if want else None, status.data_ptr(), stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    d, c, s = dist.cpu().numpy(), chosen.cpu().numpy(), status.cpu().numpy()
    assert np.isnan(d[U]).all() and (c[U] == -7).all() and s[1] == -7, "written past the outputs"
    return d[:U], c[:U], int(s[0])


def hold(key, blocks, rows, pairs, dist, chosen, status, need_gap):
    """(a) .. (d) of one launch.  rows: the ring as [frames, n_agents, 100] f32 on the host."""
    U, A, dueling = blocks.U, blocks.A, blocks.dueling
    k = (U - 1) // 2
    assert status == 0
    states = R.states_of(rows, pairs)
    flats, worst, margin = blocks.locals(), 0.0, np.inf
    for p in range(U):
        d64, bar = R.step_distances(flats, p, states[p], A, dueling)
        margin = min(margin, R.gap_margin(d64, bar, p))
        assert dist[p, p] == 0.0
        for j in range(U):
            if j != p:                                                              # (a)
                ratio = abs(float(dist[p, j]) - d64[j]) / bar[j]
                worst = max(worst, ratio)
                assert ratio <= 1.0, (key, p, j, float(dist[p, j]), d64[j], bar[j])
        own = R.stable_choice(dist[p], p)                                           # (b)
        assert chosen[p].tolist() == own + [-1] * (U - k), (key, p, chosen[p], own)
        if need_gap:                                                                # (c)
            assert R.gap_margin(d64, bar, p) > 1.0, (key, p)
        if R.gap_margin(d64, bar, p) > 1.0:
            assert own == R.stable_choice(d64, p), (key, p)
        R.merge_f32(flats, p, own)                                                  # (d): the replay the next step's f64 reads
    after = blocks.host()
    for j in range(U):
        assert np.array_equal(after[j, 0, :blocks.P], flats[j]), (key, j)
    blocks.check_rest(after)
    return worst, margin


@pytest.mark.parametrize("ring", ["episodes", "pool"])
@pytest.mark.parametrize("U,S,A,dueling", R.CASES)
def test_choice_against_float64_and_the_host_replay(pool, episodes, ring, U, S, A, dueling):
    rows, obs = episodes if ring == "episodes" else (pool.obs, pool.ring.obs)
    pairs = R.case_pairs(U, S, A, obs.shape[0], obs.shape[1])
    blocks = Blocks(R.family(A, dueling, U), A, dueling)
    key = "%s U%d S%d A%d%s" % (ring, U, S, A, "d" if dueling else "")
    worst, margin = hold(key, blocks, rows, pairs, *run(blocks, obs, pairs), need_gap=True)
    WORST[ring] = max(WORST.get(ring, 0.0), worst)
    print(key, "worst ratio %.4f gap margin %.2f" % (worst, margin))
    if U <= 2:                                                  # nobody chosen: every bit stays
        assert np.array_equal(blocks.host(), blocks.before)


def test_the_golden_inputs_give_the_executed_reference(pool):
    g = load_golden("federated_choice.npz")
    U, S = 5, 10
    rows = g["states"].reshape(1, U * S, 100)
    obs = torch.tensor(pack_obs_rows(rows.reshape(-1, 100)).reshape(1, U * S, 20), device="cuda").contiguous()
    pairs = np.stack([np.zeros(U * S, np.int32), np.arange(U * S, dtype=np.int32)], 1).reshape(U, S, 2)
    blocks = Blocks([golden_flat(g, f"l{j}_before_", True) for j in range(U)], 3, True)
    dist, chosen, status = run(blocks, obs, pairs)
    worst, margin = hold("golden", blocks, rows, pairs, dist, chosen, status, need_gap=True)
    WORST["golden"] = worst
    assert chosen[:, :2].tolist() == g["chosen"].tolist()
    after = blocks.host()
    for j in range(U):
        assert np.array_equal(after[j, 0, :blocks.P], golden_flat(g, f"l{j}_after_", True)), j      # bit for bit


def test_exact_ties(episodes):
    rows, obs = episodes
    A, dueling, U, S = 3, True, 5, 10
    fam = R.family(A, dueling, 3)
    pairs = R.case_pairs(U, S, A, obs.shape[0], obs.shape[1])
    # nets 1, 3, 4 bit-identical, net 2 far away: for p = 0 the twins tie bit for bit and the lower indices win
    blocks = Blocks([fam[0], fam[2], fam[1], fam[2].copy(), fam[2].copy()], A, dueling)
    dist, chosen, status = run(blocks, obs, pairs)
    assert status == 0 and dist[0, 1] == dist[0, 3] == dist[0, 4] and dist[0, 1] < dist[0, 2]
    assert chosen[0].tolist() == [1, 3, -1, -1, -1]
    # ... and for p = 1 its twins are at distance exactly 0 (net 0 has moved by then; 3 and 4 have not)
    assert dist[1, 3] == 0.0 and dist[1, 4] == 0.0 and chosen[1].tolist() == [3, 4, -1, -1, -1]
    flats = blocks.locals()
    for p in range(U):
        R.merge_f32(flats, p, [c for c in chosen[p].tolist() if c >= 0])
    after = blocks.host()
    assert all(np.array_equal(after[j, 0, :blocks.P], flats[j]) for j in range(U))
    blocks.check_rest(after)


def test_status_refusals_and_nullable_outputs(episodes):
    L = _lib()
    rows, obs = episodes
    A, dueling, U, S = 3, False, 3, 10
    F, N = obs.shape[0], obs.shape[1]
    good = R.case_pairs(U, S, A, F, N)
    for where, bad in (((2, 9), (F, 0)), ((0, 0), (0, N)), ((1, 4), (-1, 3)), ((1, 5), (1, -1)), ((2, 0), (2 ** 30, 2 ** 30))):
        pairs = good.copy()
        pairs[where] = bad
        blocks = Blocks(R.family(A, dueling, U), A, dueling)
        dist, chosen, status = run(blocks, obs, pairs)
        assert status == 1 and np.array_equal(blocks.host(), blocks.before), bad           # no block is written
    # every refusal: UAVENV_EINVAL with nothing enqueued -- the blocks and the status word stay as they were
    blocks = Blocks(R.family(A, dueling, U), A, dueling)
    pr = torch.tensor(good, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    lib = L.load()

    def call(nets=None, n_nets=None, o=obs.data_ptr(), frames=F, n_agents=N, p=pr.data_ptr(), s=S, st=status.data_ptr()):
        arr = blocks.array() if nets is None else (C.POINTER(L.UavDqnNet) * max(len(nets), 1))(*[None if n is None else C.pointer(n) for n in nets])
        return lib.uavenv_fed_choice(o, frames, n_agents, p, s, arr, (blocks.U if nets is None else len(nets)) if n_nets is None else n_nets,
                                     None, None, st, stream())

    def variant(j, **kw):
        n = blocks.nets[j]
        f = dict(local=n.local, target=n.target, m=n.m, v=n.v, w=n.w, hid=n.hid, n_actions=n.n_actions, dueling=n.dueling,
                 mfma_dtype=n.mfma_dtype, reserved0=0)
        f.update(kw)
        return L.UavDqnNet(*[f[k] for k in ("local", "target", "m", "v", "w", "hid", "n_actions", "dueling", "mfma_dtype", "reserved0")])

    n0, n1, n2 = blocks.nets
    E = L.EINVAL
    assert call(n_nets=0) == E and call(nets=[n0] * 9) == E and call(nets=[n0, None, n2]) == E
    assert call(s=0) == E and call(s=17) == E
    assert call(o=None) == E and call(p=None) == E and call(st=None) == E
    assert call(nets=[n0, variant(1, local=n1.local + 4), n2]) == E and call(o=obs.data_ptr() + 4) == E
    assert call(nets=[n0, n1, variant(0)]) == E                                             # two nets, one local block
    assert call(nets=[n0, variant(1, mfma_dtype=L.MFMA_F16), n2]) == E
    assert call(nets=[n0, variant(1, n_actions=4), n2]) == E and call(nets=[n0, variant(1, dueling=1), n2]) == E
    assert call(nets=[variant(j, n_actions=1) for j in range(3)]) == E
    assert call(nets=[variant(j, n_actions=14, dueling=1) for j in range(3)]) == E
    assert call(nets=[variant(j, w=96) for j in range(3)]) == E
    assert call(frames=0) == E and call(n_agents=0) == E
    assert len(refusals()) == 20                                                            # the CPU file's list, none dropped
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == -7 and np.array_equal(blocks.host(), blocks.before)
    # dist_out and chosen_out both NULL: the same blocks
    a, b = Blocks(R.family(A, dueling, U), A, dueling), Blocks(R.family(A, dueling, U), A, dueling)
    _, _, sa = run(a, obs, good)
    _, _, sb = run(b, obs, good, want=False)
    assert sa == 0 and sb == 0 and np.array_equal(a.host(), b.host()) and not np.array_equal(a.host(), a.before)


def test_choice_merge_blocks_checks_before_it_enqueues(episodes):
    from dqn_based_uav_3d_path_planer_amd import federated
    rows, obs = episodes
    blocks = Blocks(R.family(3, False, 3), 3, False)
    Ls = [types.SimpleNamespace(net=blocks.nets[j], flat=blocks.buf[j, :, :blocks.P], n_actions=3, dueling=False, mfma="f32") for j in range(3)]
    pairs = torch.tensor(R.case_pairs(3, 10, 3, obs.shape[0], obs.shape[1]), device="cuda")
    for bad in (dict(obs=obs.view(-1, 20)), dict(obs=obs.float()), dict(obs=obs.cpu()), dict(pairs=pairs[:2]), dict(pairs=pairs.long()),
                dict(pairs=pairs.cpu()), dict(pairs=torch.zeros((3, 17, 2), dtype=torch.int32, device="cuda")),
                dict(ls=Ls[:2] + [Ls[0]]), dict(ls=[]), dict(ls=Ls[:2] + [types.SimpleNamespace(**dict(vars(Ls[2]), mfma="f16"))])):
        with pytest.raises(ValueError):
            federated.choice_merge_blocks(bad.get("ls", Ls), bad.get("obs", obs), bad.get("pairs", pairs))
    torch.cuda.synchronize()
    assert np.array_equal(blocks.host(), blocks.before)
    dist, chosen, status = federated.choice_merge_blocks(Ls, obs, pairs)
    want = Blocks(R.family(3, False, 3), 3, False)
    d2, c2, s2 = run(want, obs, pairs.cpu().numpy())
    assert int(status.cpu()[0]) == 0 and s2 == 0 and np.array_equal(dist.cpu().numpy(), d2) and np.array_equal(chosen.cpu().numpy(), c2)
    assert np.array_equal(blocks.host(), want.host())


# ---- (g) the plugin's fused-slots path -------------------------------------------------------------------------------------------

U_PLUGIN = 4        # the env takes a power of two UAVs per env: 4 is the smallest count that chooses a partner


def _config(tmp_path, **env_tags):
    from dqn_based_uav_3d_path_planer_amd import driver
    xml = driver.make_config_dir(str(tmp_path), "DQN", num_envs=512, num_uav=U_PLUGIN)
    s = open(xml).read()
    for k, v in dict(env_tags, fused_slots=1).items():
        if re.search(rf"<{k}>[^<]*</{k}>", s):
            s = re.sub(rf"<{k}>[^<]*</{k}>", f"<{k}>{v}</{k}>", s)
        else:
            s = s.replace("<seed>42</seed>", f"<seed>42</seed>\n        <{k}>{v}</{k}>")
    open(xml, "w").write(s)
    return xml


def test_plugin_fused_slots_choice_merge(tmp_path, monkeypatch):
    from dqn_based_uav_3d_path_planer_amd import driver, federated
    monkeypatch.chdir(tmp_path)
    env = driver.simulator(_config(tmp_path, Is_FL=1, FL_Loop=1, FL_Aggregate="choice")).env
    assert env is not None and env.fast_slots and env.Is_FL == 1 and env.FL_Aggregate == "choice"
    saved = {}
    real = federated.choice_merge_blocks

    def spy(learners, obs, pairs):
        saved["flat"] = [L.flat.detach().clone() for L in learners]
        saved["pairs"], saved["obs"] = pairs.clone(), obs
        return real(learners, obs, pairs)

    monkeypatch.setattr(federated, "choice_merge_blocks", spy)
    env.run_eposide(0.5)
    Ls = [u.Trainer.learner for u in env.Agents]
    assert env.fl_merges == 1 and env.fl_skipped == 0 and env.fl_merged_on == "device"
    assert torch.is_tensor(env.fl_chosen) and env.fl_chosen.is_cuda and int(env._fl_info["status"].cpu()[0]) == 0
    after = [L.flat.detach().clone() for L in Ls]
    # the same merge replayed on the saved copies with the same pairs
    L0 = Ls[0]
    P = L0.P
    blocks = Blocks([f[0].cpu().numpy() for f in saved["flat"]], L0.n_actions, bool(L0.dueling))
    dist, chosen, status = run(blocks, saved["obs"], saved["pairs"].cpu().numpy())
    assert status == 0 and np.array_equal(chosen, env.fl_chosen.cpu().numpy())
    assert (chosen[:, 0] >= 0).all() and (chosen[:, 1:] == -1).all()                       # U = 4: (U - 1) // 2 = one partner each
    host = blocks.host()
    for j in range(U_PLUGIN):
        assert np.array_equal(after[j][0].cpu().numpy(), host[j, 0, :P]), j                  # slot j's block after the merge
        assert torch.equal(after[j][1:], saved["flat"][j][1:])                               # target, m, v: untouched
    assert any(not torch.equal(after[j][0], saved["flat"][j][0]) for j in range(U_PLUGIN))
    pr = saved["pairs"].cpu().numpy()
    assert pr.shape == (U_PLUGIN, 10, 2) and all((pr[j, :, 1] % U_PLUGIN == j).all() for j in range(U_PLUGIN))    # slot j replays ITS rows
    env.run_eposide(0.5)                                                                     # the next episode trains on from it
    assert env.fl_merges == 2 and env.Check_uav_Done()
    for j, L in enumerate(Ls):
        assert torch.isfinite(L.flat).all() and not torch.equal(L.flat[0], after[j][0])
