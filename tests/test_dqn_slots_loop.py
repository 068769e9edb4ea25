"""CPU checks of the one-learner-per-UAV-slot DQN loop (uavenv_dqn_act_slots, uavenv_replay_draw_slots, uavenv_dqn_slots_loop_*):
the entries are declared and bound and the ABI version did not move, the new structs lay out as gcc sees them while the old ones
stay where they were, the Python wrappers refuse bad learner lists before anything reaches the library, and on the fake backend
<fused_slots> leaves the general path alone."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from dqn_based_uav_3d_path_planer_amd import _lib, driver, factories  # noqa: F401  (factories puts plugins/ on sys.path)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_backend  # noqa: E402

NEW = ("uavenv_dqn_act_slots", "uavenv_replay_draw_slots", "uavenv_dqn_slots_loop_create", "uavenv_dqn_slots_loop_destroy",
       "uavenv_dqn_slots_loop_set_eps", "uavenv_dqn_slots_loop_run", "uavenv_dqn_slots_loop_get")


def test_the_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert _lib.ABI_VERSION == 5 and "#define UAVENV_ABI_VERSION 5" in hdr       # additive: the version stays
    lib = _lib.load()
    assert lib.uavenv_abi_version() == 5
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(r"\bint\s+%s\s*\(" % name, code), name
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and f.argtypes is not None, name
    assert re.search(r"int uavenv_dqn_act_slots\(const UavDqnNet \*const \*nets, int32_t n_nets, const void \*obs_dev,\s*"
                     r"int32_t obs_dtype, int32_t n_envs,\s*float eps, uint64_t seed,\s*uint64_t counter, int32_t \*index_out_dev, "
                     r"float \*q_out_dev, void \*stream\);", code)
    assert len(lib.uavenv_dqn_act_slots.argtypes) == 11 and len(lib.uavenv_replay_draw_slots.argtypes) == 12
    # the image form the loop calls is exported beside the ABI, not declared in it
    assert hasattr(lib, "uavenv_dqn_act_slots_img") and "uavenv_dqn_act_slots_img" not in hdr
    assert len(lib.uavenv_dqn_act_slots_img.argtypes) == 12


def test_struct_layouts_as_gcc_sees_them(tmp_path):
    new = {"UavDqnSlotsLoopSlot": _lib.UavDqnSlotsLoopSlot, "UavDqnSlotsLoopConfig": _lib.UavDqnSlotsLoopConfig,
           "UavDqnSlotsLoopCursor": _lib.UavDqnSlotsLoopCursor}
    old = {"UavLoopConfig": _lib.UavLoopConfig, "UavDqnNet": _lib.UavDqnNet, "UavReplayRing": _lib.UavReplayRing}
    structs = dict(new, **old)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "uavenv.h"', 'int main(void){']
    for name, ct in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines.append('printf("slots %d\\n", UAVENV_DQN_MAX_SLOTS);')
    protos = [
        'int (*f1)(const UavDqnNet *const *, int32_t, const void *, int32_t, int32_t, float, uint64_t, uint64_t, int32_t *, float *, '
        'void *) = uavenv_dqn_act_slots;',
        'int (*f2)(int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, const uint8_t *, int32_t, uint64_t, uint64_t, int32_t *, '
        'void *) = uavenv_replay_draw_slots;',
        'int (*f3)(const UavDqnSlotsLoopConfig *, UavDqnSlotsLoop **) = uavenv_dqn_slots_loop_create;',
        'int (*f4)(UavDqnSlotsLoop *) = uavenv_dqn_slots_loop_destroy;',
        'int (*f5)(UavDqnSlotsLoop *, float) = uavenv_dqn_slots_loop_set_eps;',
        'int (*f6)(UavDqnSlotsLoop *, int32_t, void *) = uavenv_dqn_slots_loop_run;',
        'int (*f7)(const UavDqnSlotsLoop *, UavDqnSlotsLoopCursor *) = uavenv_dqn_slots_loop_get;',
        '(void)f1; (void)f2; (void)f3; (void)f4; (void)f5; (void)f6; (void)f7;']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + protos + ['return 0;}']))
    subprocess.run(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "layout.o")],
                   check=True)                                                   # the prototypes
    src.write_text("\n".join(lines + ['return 0;}']))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {l.split()[0]: l.split()[1:] for l in out}
    for name, ct in structs.items():
        assert int(got[name][0]) == ctypes.sizeof(ct), name
        for fname, _ in ct._fields_:
            assert int(got[f"{name}.{fname}"][0]) == getattr(ct, fname).offset, (name, fname)
    assert int(got["slots"][0]) == _lib.DQN_MAX_SLOTS == 8
    # the structs that existed before are where they were
    assert ctypes.sizeof(_lib.UavDqnNet) == 56 and ctypes.sizeof(_lib.UavReplayRing) == 64
    assert [getattr(_lib.UavDqnNet, f).offset for f, _ in _lib.UavDqnNet._fields_] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]
    assert [getattr(_lib.UavReplayRing, f).offset for f, _ in _lib.UavReplayRing._fields_] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56]
    assert ctypes.sizeof(_lib.UavLoopConfig) == 416 and _lib.UavLoopConfig.moved_dev.offset == 408
    assert _lib.UavLoopConfig.net.offset == 72 and _lib.UavLoopConfig.per.offset == 264
    # ... and the new ones embed them
    assert ctypes.sizeof(_lib.UavDqnSlotsLoopSlot) == 56 + 24
    assert _lib.UavDqnSlotsLoopConfig.slot.offset % 8 == 0
    assert ctypes.sizeof(_lib.UavDqnSlotsLoopConfig) == _lib.UavDqnSlotsLoopConfig.slot.offset + 8 * 80
    assert ctypes.sizeof(_lib.UavDqnSlotsLoopCursor) == 16 + 8 * 4


class _L:
    """What the checks may look at of a learner; anything else fails."""

    def __init__(self, n_actions=3, dueling=False, mfma="f32", kind="dqn", lr=1e-3):
        self.net, self.flat = object(), object()
        self.n_actions, self.dueling, self.mfma, self.kind = n_actions, dueling, mfma, kind
        self.huber, self.update_loop, self.gamma, self.lr, self.betas, self.eps = 0, 3, 0.99, lr, (0.9, 0.999), 1e-8

    def __getattr__(self, name):
        raise AssertionError(f"the learner was touched ({name}) before the list was checked")


class _Env:
    uav_per_env, packed = 4, True

    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the arguments were checked")


class _Ring:
    discrete = True

    def __init__(self, env=None, discrete=True):
        self.env, self.discrete = env or _Env(), discrete

    def __getattr__(self, name):
        raise AssertionError(f"the ring was touched ({name}) before the arguments were checked")


@pytest.fixture()
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)


def test_slots_loop_refuses_bad_learner_lists_before_any_library_call(no_library):
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    four = [_L() for _ in range(4)]
    cases = {
        "three learners for four slots": four[:3],
        "five learners for four slots": four + [_L()],
        "none": [],
        "one learner twice": [four[0], four[1], four[2], four[0]],
        "n_actions differ": four[:3] + [_L(n_actions=4)],
        "head shapes differ": four[:3] + [_L(dueling=True, kind="dueling")],
        "kinds differ": four[:3] + [_L(kind="ddqn")],
        "hyper-parameters differ": four[:3] + [_L(lr=2e-3)],
        "f16 MFMA": four[:3] + [_L(mfma="f16")],
        "not a fused learner": four[:3] + [object()],
    }
    for name, ls in cases.items():
        with pytest.raises(ValueError):
            DQNSlotsHotLoop(_Ring(), ls, 64, seed=1)
    with pytest.raises(ValueError):
        DQNSlotsHotLoop(_Ring(discrete=False), four, 64, seed=1)                # a continuous ring

    class F32Env(_Env):
        packed = False
    with pytest.raises(ValueError):
        DQNSlotsHotLoop(_Ring(F32Env()), four, 64, seed=1)                       # rows that are not packed
    with pytest.raises(ValueError):
        DQNSlotsHotLoop(_Ring(), four, 65, seed=1)                               # batch % 64
    with pytest.raises(ValueError):
        DQNSlotsHotLoop(_Ring(), four, 64, seed=1, skip_done=False, valid_draws=True)
    with pytest.raises(AssertionError, match="library was loaded"):              # a good list gets as far as the library
        DQNSlotsHotLoop(_Ring(), four, 64, seed=1)


def test_act_slots_refuses_bad_arguments_before_any_library_call(no_library):
    from dqn_based_uav_3d_path_planer_amd.learner import act_slots, check_slot_learners
    two = [_L(), _L()]
    obs = torch.zeros((8, 20), dtype=torch.int32)
    idx = torch.zeros(8, dtype=torch.int32)
    for ls in ([], None, [two[0], two[0]], [two[0], _L(n_actions=4)], [two[0], _L(dueling=True)], [two[0], _L(mfma="f16")],
               [_L() for _ in range(9)], [two[0], 3]):
        with pytest.raises(ValueError):
            act_slots(ls, obs, 0.1, 1, 2, idx)
    bad = [dict(obs=torch.zeros((8, 100))), dict(obs=torch.zeros((8, 20), dtype=torch.int32)[:, :19]),
           dict(obs=torch.zeros((7, 20), dtype=torch.int32), idx=torch.zeros(7, dtype=torch.int32)),
           dict(obs=torch.zeros((0, 20), dtype=torch.int32), idx=torch.zeros(0, dtype=torch.int32)),
           dict(idx=None), dict(idx=torch.zeros(8)), dict(idx=torch.zeros(6, dtype=torch.int32)),
           dict(q=torch.zeros((8, 2))), dict(q=torch.zeros((8, 3), dtype=torch.float64)), dict(images=[None])]
    for kw in bad:
        with pytest.raises(ValueError):
            act_slots(two, kw.get("obs", obs), 0.1, 1, 2, kw.get("idx", idx), q_out=kw.get("q"), images=kw.get("images"))
    assert check_slot_learners(two) == two and check_slot_learners(two, 2) == two
    with pytest.raises(ValueError):
        check_slot_learners(two, 4)
    with pytest.raises(AssertionError, match="library was loaded"):
        act_slots(two, obs, 0.1, 1, 2, idx)


@pytest.fixture()
def cfg_dir(tmp_path, monkeypatch):
    import _backend                                    # plugins/_backend.py (on sys.path via factories)
    monkeypatch.setattr(_backend, "make_backend", lambda n, b, **kw: fake_backend.OracleVecEnv(n, b, **kw))
    monkeypatch.chdir(tmp_path)
    return tmp_path


@pytest.mark.parametrize("tag", [None, "0", "1"])
def test_fused_slots_absent_or_unqualified_leaves_the_general_path(cfg_dir, tag):
    """Without the tag, with <fused_slots>0, and with <fused_slots>1 where the path does not qualify (no GPU: the trainers are
    not fused, the rows not packed) the env has fast_slots False and run_eposide is the general loop."""
    import random
    xml = driver.make_config_dir(str(cfg_dir), "DQN", num_envs=3, num_uav=2)
    if tag is not None:
        s = open(xml).read()
        open(xml, "w").write(s.replace("<seed>42</seed>", f"<seed>42</seed>\n        <fused_slots>{tag}</fused_slots>"))
    env = driver.simulator(xml).env
    assert env is not None and env.fast_slots is False and not env.fast and not env.fast_sac
    assert env._ring is None and env._slots_hot is None and not getattr(env.backend, "packed", False)
    assert not any(getattr(u.Trainer, "fused", False) for u in env.Agents)
    random.seed(1)
    torch.manual_seed(1)
    res = env.run_eposide(0.9)
    assert env.Check_uav_Done() and res["lose"] + res["success"] >= 6
    assert all(u.Trainer.epoch > 50 for u in env.Agents) and env._slots_hot is None
