"""CPU checks of prioritised replay in the per-slot DQN loop (uavenv_per_*_slots, uavenv_dqn_grad_slots_w,
uavenv_dqn_slots_loop_set_per / _get_per): the entries are declared, bound and exported and the ABI version did not move, the
prototypes are what gcc reads in the header, the pinned structs are where they were and UavDqnSlotsPer lays out as its ctypes
mirror, every refusal that needs no device comes back as UAVENV_EINVAL, and DQNSlotsHotLoop(pers=...) and
learner.update_slots(is_weights=...) refuse bad arguments before anything reaches the library.  (The refusals of
uavenv_dqn_slots_loop_set_per that need a loop -- and so a device -- are in tests/test_dqn_slots_per_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from dqn_based_uav_3d_path_planer_amd import _lib
from test_dqn_slots_loop import _L, _Env, _Ring, no_library  # noqa: F401  (the stand-ins that fail when touched too early)
from test_dqn_update_slots import _arr, _net, _ptrs, _ring

PER = ("uavenv_per_fill_frame_slots", "uavenv_per_rebuild_slots", "uavenv_per_sample_slots", "uavenv_per_weights_slots",
       "uavenv_per_set_f32_slots_gated")
NEW = PER + ("uavenv_dqn_grad_slots_w", "uavenv_dqn_slots_loop_set_per", "uavenv_dqn_slots_loop_get_per")


def test_the_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "uavenv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert _lib.ABI_VERSION == 5 and "#define UAVENV_ABI_VERSION 5" in hdr       # additive: the version stays
    lib = _lib.load()
    assert lib.uavenv_abi_version() == 5
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(r"\bint\s+%s\s*\(" % name, code), name
        f = getattr(lib, name)
        assert f.restype is C.c_int and f.argtypes is not None, name
    assert [len(getattr(lib, n).argtypes) for n in NEW] == [8, 8, 8, 11, 11, 16, 2, 2]
    # the image form the loop calls is exported beside the ABI, not declared in it
    internal = open(os.path.join(ROOT, "dqn_based_uav_3d_path_planer_amd", "csrc", "dqn_slots_internal.hpp")).read()
    assert hasattr(lib, "uavenv_dqn_grad_slots_w_img") and "uavenv_dqn_grad_slots_w_img" not in hdr
    assert "uavenv_dqn_grad_slots_w_img" not in _lib.SYMBOLS and "uavenv_dqn_grad_slots_w_img" in internal
    assert len(lib.uavenv_dqn_grad_slots_w_img.argtypes) == 17
    # dqn_internal.hpp, whose list tests/test_abi.py pins, gained nothing
    assert "slots" not in open(os.path.join(ROOT, "dqn_based_uav_3d_path_planer_amd", "csrc", "dqn_internal.hpp")).read()


def test_prototypes_as_gcc_reads_them_and_the_struct_layouts(tmp_path):
    per_head = 'int (*%s)(const UavPer *const *, int32_t, '
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "uavenv.h"', 'int main(void){']
    protos = [
        per_head % 'f1' + 'int64_t, int64_t, double, const uint8_t *, int64_t, void *) = uavenv_per_fill_frame_slots;',
        per_head % 'f2' + 'int64_t, int64_t, double, const uint8_t *, int64_t, void *) = uavenv_per_rebuild_slots;',
        per_head % 'f3' + 'int32_t, uint64_t, uint64_t, int64_t *, double *, void *) = uavenv_per_sample_slots;',
        per_head % 'f4' + 'const int64_t *, double *, int32_t, int64_t, double, int32_t, float *, int32_t *, void *) = '
        'uavenv_per_weights_slots;',
        per_head % 'f5' + 'const int64_t *, const float *, int32_t, double, double, double, const uint32_t *, uint32_t, void *) = '
        'uavenv_per_set_f32_slots_gated;',
        'int (*f6)(const UavReplayRing *, int32_t, int32_t, int32_t, uint64_t, uint64_t, const int32_t *, const UavDqnNet *const *, '
        'int32_t, int32_t, float, int32_t, const float *, float *, float *const *, void *) = uavenv_dqn_grad_slots_w;',
        'int (*f7)(UavDqnSlotsLoop *, const UavDqnSlotsPer *) = uavenv_dqn_slots_loop_set_per;',
        'int (*f8)(const UavDqnSlotsLoop *, double *) = uavenv_dqn_slots_loop_get_per;',
        '(void)f1; (void)f2; (void)f3; (void)f4; (void)f5; (void)f6; (void)f7; (void)f8;']
    structs = {"UavDqnSlotsPer": _lib.UavDqnSlotsPer, "UavPer": _lib.UavPer, "UavDqnSlotsLoopConfig": _lib.UavDqnSlotsLoopConfig,
               "UavDqnSlotsLoopSlot": _lib.UavDqnSlotsLoopSlot, "UavDqnSlotsLoopCursor": _lib.UavDqnSlotsLoopCursor,
               "UavLoopConfig": _lib.UavLoopConfig}
    for name, ct in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + protos + ['return 0;}']))
    subprocess.run(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "layout.o")],
                   check=True)                                                   # the prototypes
    src.write_text("\n".join(lines + ['return 0;}']))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out}
    for name, ct in structs.items():
        assert got[name] == C.sizeof(ct), name
        for fname, _ in ct._fields_:
            assert got[f"{name}.{fname}"] == getattr(ct, fname).offset, (name, fname)
    # the new struct: eight trees, four buffers, five doubles; the pinned ones as before
    assert C.sizeof(_lib.UavPer) == 48 and C.sizeof(_lib.UavDqnSlotsPer) == 8 * 48 + 4 * 8 + 5 * 8
    assert C.sizeof(_lib.UavDqnNet) == 56 and C.sizeof(_lib.UavReplayRing) == 64 and C.sizeof(_lib.UavLoopConfig) == 416
    assert C.sizeof(_lib.UavDqnSlotsLoopSlot) == 80 and C.sizeof(_lib.UavDqnSlotsLoopCursor) == 48
    assert C.sizeof(_lib.UavDqnSlotsLoopConfig) == _lib.UavDqnSlotsLoopConfig.slot.offset + 8 * 80


# ---- host-side refusals: every argument is checked before anything is enqueued, so none of these needs a device ---------------

def _per(k, capacity=1800, rot=0, group=True):
    """A UavPer whose (never dereferenced) arrays are distinct per k."""
    base = 0x40000000 + 0x1000000 * k
    return _lib.UavPer(base, base + 0x100000, base + 0x200000, capacity, rot, base + 0x300000 if group else None)


def _tab(pers):
    return (C.POINTER(_lib.UavPer) * max(len(pers), 1))(*[None if p is None else C.pointer(p) for p in pers])


SLOTS, PRIO, W, ABS, PAIRS, VALID = 0x5000000, 0x5100000, 0x5200000, 0x5300000, 0x5400000, 0x5500000


def _calls(lib, pers, n=None, batch=64, n_entries=100, first=0, count=200, retire=200, tab=True):
    """The five calls on one table: {name: return code}."""
    t = _tab(pers) if tab else None
    n = len(pers) if n is None else n
    return {
        "fill": lib.uavenv_per_fill_frame_slots(t, n, first, count, 0.5, VALID, retire, None),
        "rebuild": lib.uavenv_per_rebuild_slots(t, n, first, count, 0.5, VALID, retire, None),
        "sample": lib.uavenv_per_sample_slots(t, n, batch, 1, 2, SLOTS, PRIO, None),
        "weights": lib.uavenv_per_weights_slots(t, n, SLOTS, PRIO, batch, n_entries, 0.4, 200, W, PAIRS, None),
        "set": lib.uavenv_per_set_f32_slots_gated(t, n, SLOTS, ABS, batch, 0.01, 0.6, 1.0, None, 0, None),
    }


def test_per_slots_host_side_refusals():
    lib, E = _lib.load(), _lib.EINVAL
    two = [_per(0), _per(1)]

    def all_refused(pers, **kw):
        got = _calls(lib, pers, **kw)
        assert all(rc == E for rc in got.values()), (got, kw)

    all_refused(two, tab=False)                                       # no table
    all_refused(two, n=0)                                             # 1 .. 8 trees
    all_refused([_per(k) for k in range(9)])
    all_refused([two[0], None])                                       # none NULL
    for field in ("prio", "chunk_sum", "chunk_prefix"):               # per_ok each
        bad = _per(1)
        setattr(bad, field, None)
        all_refused([two[0], bad])
    all_refused([two[0], _per(1, capacity=0)])
    all_refused([two[0], _per(1, capacity=1801)])                     # equal capacities
    all_refused([two[0], _per(1, rot=1)])                             # rot == 0
    all_refused([_per(0, rot=3), _per(1, rot=3)])
    all_refused([two[0], _per(1, group=False)])                       # group sums on all trees or on none
    all_refused([_per(0, group=False), two[1]])
    twin = _per(5)
    twin.prio = two[0].prio
    all_refused([two[0], twin])                                       # distinct prio arrays
    # batch > 0, n_entries > 0, the frame inside the tree
    got = _calls(lib, two, batch=0)
    assert got["sample"] == E and got["weights"] == E and got["set"] == E
    got = _calls(lib, two, batch=-64)
    assert got["sample"] == E and got["weights"] == E and got["set"] == E
    assert _calls(lib, two, n_entries=0)["weights"] == E and _calls(lib, two, n_entries=-5)["weights"] == E
    for kw in (dict(first=-1), dict(count=-1), dict(first=1700), dict(retire=1700), dict(retire=-200)):
        got = _calls(lib, two, **kw)
        assert got["fill"] == E and got["rebuild"] == E, kw
    # NULL buffers
    t = _tab(two)
    assert lib.uavenv_per_sample_slots(t, 2, 64, 1, 2, None, PRIO, None) == E
    assert lib.uavenv_per_weights_slots(t, 2, None, PRIO, 64, 100, 0.4, 200, W, PAIRS, None) == E
    assert lib.uavenv_per_weights_slots(t, 2, SLOTS, None, 64, 100, 0.4, 200, W, PAIRS, None) == E
    assert lib.uavenv_per_weights_slots(t, 2, SLOTS, PRIO, 64, 100, 0.4, 200, None, PAIRS, None) == E
    assert lib.uavenv_per_weights_slots(t, 2, SLOTS, PRIO, 64, 100, 0.4, 0, W, PAIRS, None) == E          # pairs need n_envs
    assert lib.uavenv_per_set_f32_slots_gated(t, 2, None, ABS, 64, 0.01, 0.6, 1.0, None, 0, None) == E
    assert lib.uavenv_per_set_f32_slots_gated(t, 2, SLOTS, None, 64, 0.01, 0.6, 1.0, None, 0, None) == E
    # a good table with an empty frame is accepted and enqueues nothing (what uavenv_dqn_slots_loop_set_per asks)
    assert lib.uavenv_per_fill_frame_slots(t, 2, 0, 0, 0.5, None, 0, None) == _lib.OK
    assert lib.uavenv_per_fill_frame_slots(_tab([_per(0, group=False), _per(1, group=False)]), 2, 0, 0, 0.5, None, 0, None) == _lib.OK


def _grad_w(lib, nets, parts, w=W, a=ABS, n_nets=None, ring=None, pairs=0x8000000, batch=64):
    ring = ring or _ring()
    return lib.uavenv_dqn_grad_slots_w(C.byref(ring), 1, 2, batch, 0, 0, pairs, _arr(nets), len(nets) if n_nets is None else n_nets,
                                       0, 0.99, 0, w, a, _ptrs(parts), None)


def test_grad_slots_w_and_loop_setter_host_side_refusals():
    lib, E = _lib.load(), _lib.EINVAL
    nets, parts = [_net(0), _net(1)], [0x7000000, 0x7100000]
    # the two new pointers are mandatory and f32-aligned
    assert _grad_w(lib, nets, parts, w=None) == E and _grad_w(lib, nets, parts, a=None) == E
    assert _grad_w(lib, nets, parts, w=W + 2) == E and _grad_w(lib, nets, parts, a=ABS + 1) == E
    # ... and everything uavenv_dqn_grad_slots refuses
    assert _grad_w(lib, nets, parts, n_nets=0) == E and _grad_w(lib, [_net(k) for k in range(9)], [0x7000000 + 0x100000 * k for k in range(9)]) == E
    assert _grad_w(lib, [nets[0], None], parts) == E and _grad_w(lib, nets, [parts[0], None]) == E
    assert _grad_w(lib, nets, parts, pairs=None) == E and _grad_w(lib, nets, parts, pairs=0x8000004) == E
    assert _grad_w(lib, nets, parts, ring=_ring(_lib.OBS_F32)) == E and _grad_w(lib, nets, parts, ring=_ring(_lib.OBS_F16)) == E
    assert _grad_w(lib, [nets[0], _net(1, mfma=_lib.MFMA_F16)], parts) == E
    assert _grad_w(lib, [_net(0, A=5), _net(1, A=5)], parts) == E                        # the packed8 family only
    assert _grad_w(lib, [_net(0, A=4, dueling=1), _net(1, A=4, dueling=1)], parts) == E
    assert _grad_w(lib, [nets[0], _net(1, A=4)], parts) == E and _grad_w(lib, [nets[0], _net(1, dueling=1)], parts) == E
    twin = _net(5)
    twin.local = nets[0].local
    assert _grad_w(lib, [nets[0], twin], parts) == E and _grad_w(lib, nets, [parts[0], parts[0]]) == E
    assert _grad_w(lib, nets, [parts[0], parts[1] + 8]) == E
    assert _grad_w(lib, nets, parts, batch=65) == E and _grad_w(lib, nets, parts, batch=0) == E
    no_target = _net(1)
    no_target.target = None
    assert _grad_w(lib, [nets[0], no_target], parts) == E
    # the loop's setter and getter without a loop
    cfg = _lib.UavDqnSlotsPer()
    beta = C.c_double(7.0)
    assert lib.uavenv_dqn_slots_loop_set_per(None, C.byref(cfg)) == E and lib.uavenv_dqn_slots_loop_set_per(None, None) == E
    assert lib.uavenv_dqn_slots_loop_get_per(None, C.byref(beta)) == E and beta.value == 7.0


# ---- DQNSlotsHotLoop(pers=...) / learner.update_slots(is_weights=...): checked before the library is loaded -------------------

class _P:
    """What the checks may look at of a DevicePER; anything else fails."""

    class _CPer:
        def __init__(self, rot):
            self.rot = rot

    def __init__(self, capacity=9 * 50, rot=0, alpha=0.6, beta=0.4, beta_inc=0.001, epsilon=0.01, clip=1.0):
        self.capacity, self._c = capacity, _P._CPer(rot)
        self.alpha, self.beta, self.beta_inc, self.epsilon, self.clip = alpha, beta, beta_inc, epsilon, clip

    def __getattr__(self, name):
        raise AssertionError(f"the tree was touched ({name}) before the arguments were checked")


class _SizedEnv(_Env):
    N = 200                       # 50 envs x 4 UAV slots


class _SizedRing(_Ring):
    frames = 9


def test_slots_loop_refuses_bad_trees_before_any_library_call(no_library):  # noqa: F811
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    four = [_L() for _ in range(4)]
    good = [_P() for _ in range(4)]
    ring = lambda: _SizedRing(_SizedEnv())  # noqa: E731
    cases = {
        "three trees for four slots": good[:3],
        "five trees": good + [_P()],
        "some slots only": good[:3] + [None],
        "one tree twice": good[:3] + [good[0]],
        "another capacity": good[:3] + [_P(capacity=9 * 200)],
        "tree order": good[:3] + [_P(rot=62)],
        "alpha differs": good[:3] + [_P(alpha=0.7)],
        "beta differs": good[:3] + [_P(beta=0.5)],
        "beta_inc differs": good[:3] + [_P(beta_inc=0.002)],
        "epsilon differs": good[:3] + [_P(epsilon=0.02)],
        "clip differs": good[:3] + [_P(clip=2.0)],
    }
    for name, pers in cases.items():
        with pytest.raises(ValueError):
            DQNSlotsHotLoop(ring(), four, 64, seed=1, pers=pers)
    with pytest.raises(ValueError, match="needs a batch"):
        DQNSlotsHotLoop(ring(), four, 0, seed=1, pers=good)
    wide = [_L(n_actions=5) for _ in range(4)]
    with pytest.raises(ValueError, match="at most 4"):
        DQNSlotsHotLoop(ring(), wide, 64, seed=1, pers=good)
    with pytest.raises(ValueError):                                              # the learner list is still checked first
        DQNSlotsHotLoop(ring(), four[:3] + [_L(lr=2e-3)], 64, seed=1, pers=good)
    # a good list gets as far as the library; so does "no tree anywhere", which is the uniform loop
    with pytest.raises(AssertionError, match="library was loaded"):
        DQNSlotsHotLoop(ring(), four, 64, seed=1, pers=good)
    with pytest.raises(AssertionError, match="library was loaded"):
        DQNSlotsHotLoop(ring(), four, 64, seed=1, pers=[None] * 4)
    with pytest.raises(AssertionError, match="library was loaded"):
        DQNSlotsHotLoop(ring(), four, 64, seed=1, pers=good, multi_update=False)


def test_update_slots_refuses_bad_weights_before_any_library_call(no_library):  # noqa: F811
    from dqn_based_uav_3d_path_planer_amd.learner import update_slots
    two = [_L(), _L()]
    pairs = torch.zeros((2, 64, 2), dtype=torch.int32)
    ring = _Ring()
    w, a = torch.ones((2, 64)), torch.zeros((2, 64))
    with pytest.raises(ValueError, match="come together"):
        update_slots(two, ring, 64, pairs, is_weights=w)
    with pytest.raises(ValueError, match="come together"):
        update_slots(two, ring, 64, pairs, abs_td_out=a)
    bad = {
        "f64": torch.ones((2, 64), dtype=torch.float64), "flat": torch.ones(128), "another batch": torch.ones((2, 128)),
        "another U": torch.ones((3, 64)), "not contiguous": torch.ones((2, 128))[:, ::2], "not a tensor": [1.0] * 128,
    }
    assert tuple(bad["not contiguous"].shape) == (2, 64)
    for name, t in bad.items():
        with pytest.raises(ValueError, match="is_weights must be"):
            update_slots(two, ring, 64, pairs, is_weights=t, abs_td_out=a)
        with pytest.raises(ValueError, match="abs_td_out must be"):
            update_slots(two, ring, 64, pairs, is_weights=w, abs_td_out=t)
    with pytest.raises(ValueError, match="at most 4"):
        update_slots([_L(n_actions=5), _L(n_actions=5)], ring, 64, pairs, is_weights=w, abs_td_out=a)
    with pytest.raises(ValueError):                                              # the list's own checks come first
        update_slots([two[0], _L(lr=2e-3)], ring, 64, pairs, is_weights=w, abs_td_out=a)
    # everything above passed for these arguments: what is left is that nothing is on a device (there is none here)
    with pytest.raises(ValueError, match="on the device"):
        update_slots(two, ring, 64, pairs, is_weights=w, abs_td_out=a)
