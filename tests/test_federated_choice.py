"""The selective federated merge of DQN-family trainers (Federated_Learning_choice, Envs/PathPlan_City.py:644-684;
<FL_Aggregate>choice</FL_Aggregate>) against the EXECUTED reference: tests/golden/federated_choice.npz
(scripts/gen_golden_fl_choice.py: five DuelingDQN_Trainers with injected weights, stub replay memories).  Host side here -- the
golden's shape, federated.choice_merge_modules bit for bit, the plugin on the oracle-backed fake env, the new C entry's
declaration / binding / refusals -- and the float64 gap condition (tests/fed_choice_ref.py) of every case the GPU file
(tests/test_federated_choice_gpu.py) runs on its "episodes" ring: rows the reference's own state_PathPlan produced
(tests/golden/episodes.npz), the same rows through the same pairs.  (Its second ring is written by the environment on the GPU and
cannot be known here; the GPU file asserts the condition for those rows itself, on the float64 forward.)"""
import copy
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fed_choice_ref as R
from conftest import ROOT, load_golden
from dqn_based_uav_3d_path_planer_amd import _lib, driver, factories, federated  # noqa: F401  (factories puts plugins/ on sys.path)
from dqn_fixtures import golden_flat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_backend  # noqa: E402

VA = {"NetWork": "VAnet2", "w": "100", "hiden_dim": "64", "output": "3"}


@pytest.fixture(scope="module")
def g():
    return load_golden("federated_choice.npz")


def _flats(g, pref, when):
    return [golden_flat(g, f"{pref}{j}_{when}_", True) for j in range(int(g["n_agents"]))]


def _modules(g, when="before"):
    from dqn_based_uav_3d_path_planer_amd.nets import create_network
    ms = [create_network(VA) for _ in range(int(g["n_agents"]))]
    for j, m in enumerate(ms):
        m.load_state_dict({str(k): torch.tensor(g[f"l{j}_{when}_{k}"]) for k in g["keys"]})
    return ms


def test_the_golden_is_the_sequential_selective_mean(g):
    """What the executed reference does: sequential in p, (U - 1) // 2 = 2 closest others, f32 adds in sorted order, a true
    division by 3; q_local only."""
    U = int(g["n_agents"])
    assert U == 5 and g["chosen"].shape == (5, 2) and g["states"].shape == (5, 10, 100)
    flats = _flats(g, "l", "before")
    chosen, D, B, margin = R.restate(flats, g["states"], 3, True)
    assert chosen == g["chosen"].tolist()
    assert margin > 1.0, margin                                  # the executed choice does not hang on rounding
    for p in range(U):
        for j in range(U):
            if j != p:                                           # the reference's own f32 distances sit inside the bar
                assert abs(float(g["dist"][p, j]) - D[p, j]) <= B[p, j], (p, j)
    for j, (got, want) in enumerate(zip(flats, _flats(g, "l", "after"))):
        assert np.array_equal(got, want), j
    assert any(not np.array_equal(a, b) for a, b in zip(_flats(g, "l", "before"), _flats(g, "l", "after")))
    for a, b in zip(_flats(g, "t", "before"), _flats(g, "t", "after")):
        assert np.array_equal(a, b)                              # the q_target average is computed and thrown away
    # the mutation the divisor 3 is there for: multiplying by the reciprocal is a different result
    mut = _flats(g, "l", "before")
    R.restate(mut, g["states"], 3, True, reciprocal=True)
    assert any(not np.array_equal(a, b) for a, b in zip(mut, _flats(g, "l", "after")))


def test_choice_merge_modules_equals_the_executed_reference(g):
    ms = _modules(g)
    chosen = federated.choice_merge_modules(ms, [torch.tensor(x) for x in g["states"]])
    assert chosen == g["chosen"].tolist()
    for j, m in enumerate(ms):
        for k, v in m.state_dict().items():
            assert np.array_equal(v.numpy(), g[f"l{j}_after_{k}"]), (j, k)      # bit for bit, all five agents
    # the same code dividing by multiplication with the reciprocal (what a scalar division becomes on the GPU) is told apart
    ms = _modules(g)
    third = torch.full((1,), 1.0) / torch.full((1,), 3.0)
    with torch.no_grad():
        params = [list(m.parameters()) for m in ms]
        for p, ch in enumerate(g["chosen"].tolist()):
            for i, w in enumerate(params[p]):
                t = w.detach().clone()
                for j in ch:
                    t += params[j][i]
                w.copy_(t * third)
    differs = sum(int((m.state_dict()[str(k)].numpy() != g[f"l{j}_after_{k}"]).sum()) for j, m in enumerate(ms) for k in g["keys"])
    total = sum(g[f"l0_after_{k}"].size for k in g["keys"]) * 5
    print("reciprocal form: %d of %d elements differ" % (differs, total))
    assert differs > total // 10


def test_small_cases_and_ties():
    from dqn_based_uav_3d_path_planer_amd.nets import create_network
    torch.manual_seed(3)
    x = [torch.randn(10, 100) for _ in range(5)]
    for U in (1, 2):                                             # (U - 1) // 2 = 0: nobody is chosen, every bit stays
        ms = [create_network(VA) for _ in range(U)]
        before = [copy.deepcopy(m.state_dict()) for m in ms]
        assert federated.choice_merge_modules(ms, x[:U]) == [[]] * U
        for m, b in zip(ms, before):
            assert all(torch.equal(v, b[k]) for k, v in m.state_dict().items())
    # two bit-identical others: equal distances, the stable sort keeps the lower index first
    ms = [create_network(VA) for _ in range(5)]
    ms[3].load_state_dict(ms[1].state_dict())
    ms[4].load_state_dict(ms[1].state_dict())
    with torch.no_grad():
        for p in ms[2].parameters():
            p.mul_(40.0)                                         # far from everybody
    twin = copy.deepcopy(ms[1])
    w0 = [p.detach().clone() for p in ms[0].parameters()]
    chosen = federated.choice_merge_modules(ms, x)
    assert chosen[0] == [1, 3]
    for p, a, b in zip(ms[0].parameters(), w0, twin.parameters()):
        assert torch.equal(p, ((a + b) + b) / torch.full((1,), 3.0))
    with pytest.raises(ValueError):
        federated.choice_merge_modules(ms, x[:4])
    assert federated.SELECTIVE == ("choice",) and "choice" not in federated.AGGREGATES
    with pytest.raises(ValueError):
        federated._scale("choice", 4)


def _dueling_env(tmp_path, monkeypatch, num_uav=3, **tags):
    import _backend
    monkeypatch.setattr(_backend, "make_backend", lambda n, b, **kw: fake_backend.OracleVecEnv(n, b, **kw))
    monkeypatch.chdir(tmp_path)
    xml = driver.make_config_dir(str(tmp_path), "DuelingDQN", num_envs=2, num_uav=num_uav)
    s = open(xml).read().replace("<Is_FL>0</Is_FL>", "<Is_FL>1</Is_FL>").replace("<FL_Loop>3</FL_Loop>", "<FL_Loop>1</FL_Loop>")
    for k, v in tags.items():
        if re.search(rf"<{k}>[^<]*</{k}>", s):
            s = re.sub(rf"<{k}>[^<]*</{k}>", f"<{k}>{v}</{k}>", s, count=1)
        else:
            s = s.replace("<num_UAV>", f"<{k}>{v}</{k}>\n        <num_UAV>", 1)
    open(xml, "w").write(s)
    return driver.simulator(xml).env


def test_plugin_choice_merge(tmp_path, monkeypatch):
    env = _dueling_env(tmp_path, monkeypatch, FL_Aggregate="choice")
    assert env is not None and env.FL_Aggregate == "choice" and env.Is_FL == 1 and not env.fast_slots
    trs = [u.Trainer for u in env.Agents]
    torch.manual_seed(0)
    with torch.no_grad():
        for t in trs:
            for p in t.q_local.parameters():
                p.copy_(torch.randn_like(p) * 0.2)
    env.epoch = 1
    env._federated_merge()                                       # empty replays: the reference would raise in random.sample
    assert env.fl_merges == 0 and env.fl_skipped == 1
    for t in trs:
        mem = t.replay_memory
        n = 12
        mem.add_batch(torch.randn(n, 100), torch.zeros(n, dtype=torch.int64), torch.zeros(n), torch.randn(n, 100), torch.zeros(n))
    copies = [copy.deepcopy(t.q_local) for t in trs]
    tgt = [[p.detach().clone() for p in t.q_target.parameters()] for t in trs]
    torch.manual_seed(11)
    env._federated_merge()
    assert env.fl_merges == 1 and env.fl_skipped == 1 and env.fl_merged_on == "torch"
    torch.manual_seed(11)
    states = [t.replay_memory.states[torch.randperm(t.replay_memory.size)[:10]] for t in trs]
    want = federated.choice_merge_modules(copies, states)
    assert env.fl_chosen == want and [len(c) for c in want] == [1, 1, 1]
    for t, c, tg in zip(trs, copies, tgt):
        assert all(torch.equal(a, b) for a, b in zip(t.q_local.parameters(), c.parameters()))
        assert all(torch.equal(a, b) for a, b in zip(t.q_target.parameters(), tg))       # replace_param writes q_local only
    assert not all(torch.equal(a, b) for a, b in zip(trs[0].q_local.parameters(), trs[1].q_local.parameters()))   # not a plain mean


def test_plugin_choice_needs_dqn_family_and_defaults_stay(tmp_path, monkeypatch):
    import _backend
    monkeypatch.setattr(_backend, "make_backend", lambda n, b, **kw: fake_backend.OracleVecEnv(n, b, **kw))
    monkeypatch.chdir(tmp_path)
    xml = driver.make_config_dir(str(tmp_path), "SAC", num_envs=2, num_uav=4)
    s = open(xml).read()
    s = re.sub(r"<Is_AC>[^<]*</Is_AC>", "<Is_AC>4</Is_AC>", s, count=1) if "<Is_AC>" in s else s.replace("<num_UAV>", "<Is_AC>4</Is_AC>\n        <num_UAV>", 1)
    s = s.replace("<num_UAV>", "<FL_Aggregate>choice</FL_Aggregate>\n        <num_UAV>", 1)
    open(xml, "w").write(s)
    from PathPlan_City import PathPlan_City
    from dqn_based_uav_3d_path_planer_amd.compat import XML2Dict
    param = XML2Dict(xml).get("simulator").get("env")        # (the factory would print the error and hand back None)
    with pytest.raises(ValueError, match="Is_AC = 0"):
        PathPlan_City(param)
    d2 = tmp_path / "b"
    d2.mkdir()
    for tag in (None, "mean"):                                   # tag absent or `mean`: the mean of all, as before
        d3 = d2 / str(tag)
        d3.mkdir()
        env = _dueling_env(d3, monkeypatch, **({} if tag is None else {"FL_Aggregate": tag}))
        assert env.FL_Aggregate == ("mean" if tag else "reference") and env.fl_skipped == 0 and env.fl_chosen is None
        trs = [u.Trainer for u in env.Agents]
        torch.manual_seed(0)
        with torch.no_grad():
            for t in trs:
                for p in t.q_local.parameters():
                    p.copy_(torch.randn_like(p))
        want = [sum(ps).detach() / 3 for ps in zip(*[list(t.q_local.parameters()) for t in trs])]
        env.epoch = 1
        env._federated_merge()
        assert env.fl_merges == 1
        for t in trs:
            assert all(torch.allclose(p, w, rtol=0, atol=1e-6) for p, w in zip(t.q_local.parameters(), want))


def test_the_new_symbol_is_declared_bound_and_exported(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert _lib.ABI_VERSION == 5 and "#define UAVENV_ABI_VERSION 5" in hdr       # additive: the version stays
    lib = _lib.load()
    assert lib.uavenv_abi_version() == 5
    assert "uavenv_fed_choice" in _lib.SYMBOLS and re.search(r"\bint\s+uavenv_fed_choice\s*\(", code)
    f = lib.uavenv_fed_choice
    assert f.restype is C.c_int and len(f.argtypes) == 11
    src = tmp_path / "proto.c"
    src.write_text('#include "uavenv.h"\n'
                   'int (*f)(const void *, int32_t, int32_t, const int32_t *, int32_t, const UavDqnNet *const *, int32_t, float *, '
                   'int32_t *, int32_t *, void *) = uavenv_fed_choice;\n')
    subprocess.run(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "proto.o")],
                   check=True)


def _net(k, A=3, dueling=0, mfma=_lib.MFMA_F32, w=100, off=0):
    base = 0x100000 * (k + 1) + off
    return _lib.UavDqnNet(base, base + 0x10000, base + 0x20000, base + 0x30000, w, 64, A, dueling, mfma, 0)


def _arr(nets):
    return (C.POINTER(_lib.UavDqnNet) * max(len(nets), 1))(*[None if n is None else C.pointer(n) for n in nets])


def refusals():
    """(name, keyword arguments of call()) of every UAVENV_EINVAL uavenv_fed_choice documents."""
    two = [_net(0), _net(1)]
    return [("no nets", dict(nets=[], n_nets=0)), ("nine nets", dict(nets=[_net(k) for k in range(9)])),
            ("nets NULL", dict(nets=two, nets_arg=False)), ("a NULL net", dict(nets=[_net(0), None])),
            ("no states", dict(nets=two, S=0)), ("17 states", dict(nets=two, S=17)),
            ("obs NULL", dict(nets=two, obs=None)), ("pairs NULL", dict(nets=two, pairs=None)), ("status NULL", dict(nets=two, status=None)),
            ("local off 16 bytes", dict(nets=[_net(0), _net(1, off=4)])), ("obs off 16 bytes", dict(nets=two, obs=0x9000004)),
            ("a shared local block", dict(nets=[_net(0), _net(1), _net(0)])),
            ("an f16-MFMA net", dict(nets=[_net(0), _net(1, mfma=_lib.MFMA_F16)])),
            ("n_actions differ", dict(nets=[_net(0), _net(1, A=4)])), ("heads differ", dict(nets=[_net(0), _net(1, dueling=1)])),
            ("one action", dict(nets=[_net(0, A=1), _net(1, A=1)])), ("15 + 2 outputs", dict(nets=[_net(0, A=14, dueling=1), _net(1, A=14, dueling=1)])),
            ("w != 100", dict(nets=[_net(0, w=96), _net(1, w=96)])),
            ("no frames", dict(nets=two, frames=0)), ("no agents", dict(nets=two, n_agents=0))]


def call(lib, nets, n_nets=None, nets_arg=True, obs=0x9000000, frames=4, n_agents=128, pairs=0x8000000, S=10, dist=None, chosen=None,
         status=0x8800000, stream=None):
    return lib.uavenv_fed_choice(obs, frames, n_agents, pairs, S, _arr(nets) if nets_arg else None, len(nets) if n_nets is None else n_nets,
                                 dist, chosen, status, stream)


def test_host_side_refusals():
    """Every argument is checked before anything is enqueued: none of these pointers is ever dereferenced."""
    lib = _lib.load()
    for name, kw in refusals():
        assert call(lib, **kw) == _lib.EINVAL, name


@pytest.mark.parametrize("U,S,A,dueling", R.CASES)
def test_gap_condition_of_the_gpu_cases(U, S, A, dueling):
    """The family nets of the GPU file on reference-produced rows: at every step the float64 distances that decide the choice lie
    more than 4 bars apart, so a kernel inside the bar can only make the float64 choice."""
    ring = R.episode_ring(load_golden("episodes.npz")["obs"])
    states = R.states_of(ring, R.case_pairs(U, S, A, R.RING_FRAMES, R.RING_AGENTS))
    flats = R.family(A, dueling, U)
    chosen, D, B, margin = R.restate(flats, states, A, dueling)
    assert [len(c) for c in chosen] == [(U - 1) // 2] * U
    assert margin > 1.0, (margin, D)
