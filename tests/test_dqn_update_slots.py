"""CPU checks of the one-launch update of every UAV slot's learner (uavenv_dqn_grad_slots, uavenv_dqn_reduce_adam_slots,
uavenv_dqn_slots_loop_set_multi_update): the entries are declared, bound and exported and the ABI version did not move, their
image forms are exported beside the ABI, the prototypes are what gcc reads in the header, the pinned structs are where they
were, every refusal that needs no device comes back as UAVENV_EINVAL, and learner.update_slots refuses bad arguments before
anything reaches the library."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from dqn_based_uav_3d_path_planer_amd import _lib
from test_dqn_slots_loop import _L, _Env, _Ring, no_library  # noqa: F401  (the stand-ins that fail when touched too early)

NEW = ("uavenv_dqn_grad_slots", "uavenv_dqn_reduce_adam_slots", "uavenv_dqn_slots_loop_set_multi_update")
IMG = ("uavenv_dqn_grad_slots_img", "uavenv_dqn_reduce_adam_slots_img")


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
    assert len(lib.uavenv_dqn_grad_slots.argtypes) == 14 and len(lib.uavenv_dqn_reduce_adam_slots.argtypes) == 14
    assert len(lib.uavenv_dqn_slots_loop_set_multi_update.argtypes) == 2
    # the image forms the loop calls are exported beside the ABI, not declared in it
    internal = open(os.path.join(ROOT, "dqn_based_uav_3d_path_planer_amd", "csrc", "dqn_slots_internal.hpp")).read()
    for name in IMG:
        assert hasattr(lib, name) and name not in hdr and name not in _lib.SYMBOLS and name in internal, name
    assert len(lib.uavenv_dqn_grad_slots_img.argtypes) == 15 and len(lib.uavenv_dqn_reduce_adam_slots_img.argtypes) == 16
    # dqn_internal.hpp, whose list tests/test_abi.py pins, gained nothing
    assert "slots" not in open(os.path.join(ROOT, "dqn_based_uav_3d_path_planer_amd", "csrc", "dqn_internal.hpp")).read()


def test_prototypes_as_gcc_reads_them_and_the_pinned_structs(tmp_path):
    protos = [
        '#include "uavenv.h"',
        'int (*f1)(const UavReplayRing *, int32_t, int32_t, int32_t, uint64_t, uint64_t, const int32_t *, const UavDqnNet *const *, '
        'int32_t, int32_t, float, int32_t, float *const *, void *) = uavenv_dqn_grad_slots;',
        'int (*f2)(const UavDqnNet *const *, int32_t, float *const *, int32_t, float, float, float, float, const int32_t *, '
        'const int32_t *, float *const *, const uint32_t *, uint32_t, void *) = uavenv_dqn_reduce_adam_slots;',
        'int (*f3)(UavDqnSlotsLoop *, int32_t) = uavenv_dqn_slots_loop_set_multi_update;',
        'int sizes[] = {(int)sizeof(UavDqnSlotsLoopConfig), (int)sizeof(UavDqnSlotsLoopSlot), (int)sizeof(UavLoopConfig), '
        '(int)sizeof(UavDqnNet), (int)sizeof(UavReplayRing), (int)sizeof(UavDqnSlotsLoopCursor)};']
    src = tmp_path / "protos.c"
    src.write_text("\n".join(protos) + "\n")
    subprocess.run(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "protos.o")],
                   check=True)
    # the structs the slots loop's tests pin: sizes as before
    assert C.sizeof(_lib.UavDqnNet) == 56 and C.sizeof(_lib.UavReplayRing) == 64 and C.sizeof(_lib.UavLoopConfig) == 416
    assert C.sizeof(_lib.UavDqnSlotsLoopSlot) == 80 and C.sizeof(_lib.UavDqnSlotsLoopCursor) == 48
    assert C.sizeof(_lib.UavDqnSlotsLoopConfig) == _lib.UavDqnSlotsLoopConfig.slot.offset + 8 * 80


# ---- host-side refusals: every argument is checked before anything is enqueued, so none of these needs a device ---------------

def _net(k, A=3, dueling=0, mfma=_lib.MFMA_F32):
    """A UavDqnNet whose (never dereferenced) blocks are distinct per k and 16-byte aligned."""
    base = 0x100000 * (k + 1)
    return _lib.UavDqnNet(base, base + 0x10000, base + 0x20000, base + 0x30000, 100, 64, A, dueling, mfma, 0)


def _ring(dtype=_lib.OBS_PACKED):
    return _lib.UavReplayRing(0x9000000, 0x9100000, 0x9200000, 0x9300000, 0x9400000, 4, 128, dtype, 1, None)


def _arr(nets):
    return (C.POINTER(_lib.UavDqnNet) * max(len(nets), 1))(*[None if n is None else C.pointer(n) for n in nets])


def _ptrs(vals):
    return (C.c_void_p * max(len(vals), 1))(*vals)


def _grad(lib, nets, parts, n_nets=None, ring=None, pairs=0x8000000, batch=64, nets_arg=True, parts_arg=True):
    ring = ring or _ring()
    return lib.uavenv_dqn_grad_slots(C.byref(ring), 1, 2, batch, 0, 0, pairs, _arr(nets) if nets_arg else None,
                                     len(nets) if n_nets is None else n_nets, 0, 0.99, 0, _ptrs(parts) if parts_arg else None, None)


def _adam(lib, nets, parts, steps, n_nets=None, nets_arg=True, parts_arg=True, steps_arg=True, hard_arg=True, n_partials=2):
    U = len(nets)
    st = (C.c_int32 * max(U, 1))(*steps)
    hd = (C.c_int32 * max(U, 1))(*([0] * U))
    return lib.uavenv_dqn_reduce_adam_slots(_arr(nets) if nets_arg else None, U if n_nets is None else n_nets,
                                            _ptrs(parts) if parts_arg else None, n_partials, 1e-3, 0.9, 0.999, 1e-8,
                                            st if steps_arg else None, hd if hard_arg else None, None, None, 0, None)


def test_host_side_refusals():
    lib, E = _lib.load(), _lib.EINVAL
    nets = [_net(0), _net(1)]
    parts = [0x7000000, 0x7100000]
    # null lists
    assert _grad(lib, nets, parts, nets_arg=False) == E and _grad(lib, nets, parts, parts_arg=False) == E
    assert _grad(lib, nets, parts, pairs=None) == E
    assert lib.uavenv_dqn_grad_slots(None, 1, 2, 64, 0, 0, 0x8000000, _arr(nets), 2, 0, 0.99, 0, _ptrs(parts), None) == E
    assert _adam(lib, nets, parts, [1, 1], nets_arg=False) == E and _adam(lib, nets, parts, [1, 1], parts_arg=False) == E
    assert _adam(lib, nets, parts, [1, 1], steps_arg=False) == E and _adam(lib, nets, parts, [1, 1], hard_arg=False) == E
    # 1 .. 8 nets
    nine = [_net(k) for k in range(9)]
    nine_parts = [0x7000000 + 0x100000 * k for k in range(9)]
    assert _grad(lib, nets, parts, n_nets=0) == E and _grad(lib, nine, nine_parts) == E
    assert _adam(lib, nets, parts, [1, 1], n_nets=0) == E and _adam(lib, nine, nine_parts, [1] * 9) == E
    # a NULL net or partials entry
    assert _grad(lib, [nets[0], None], parts) == E and _grad(lib, nets, [parts[0], None]) == E
    assert _adam(lib, [nets[0], None], parts, [1, 1]) == E and _adam(lib, nets, [parts[0], None], [1, 1]) == E
    # the packed8 family only: packed rows, f32 MFMA, at most 4 layer-2 outputs, one head shape
    assert _grad(lib, nets, parts, ring=_ring(_lib.OBS_F32)) == E and _grad(lib, nets, parts, ring=_ring(_lib.OBS_F16)) == E
    assert _grad(lib, [nets[0], _net(1, mfma=_lib.MFMA_F16)], parts) == E
    assert _grad(lib, [_net(0, A=5), _net(1, A=5)], parts) == E and _grad(lib, [_net(0, A=4, dueling=1), _net(1, A=4, dueling=1)], parts) == E
    assert _grad(lib, [nets[0], _net(1, A=4)], parts) == E and _grad(lib, [nets[0], _net(1, dueling=1)], parts) == E
    assert _adam(lib, [nets[0], _net(1, A=4)], parts, [1, 1]) == E
    # two slots sharing `local` or a partials buffer
    twin = _net(5)
    twin.local = nets[0].local
    assert _grad(lib, [nets[0], twin], parts) == E and _grad(lib, nets, [parts[0], parts[0]]) == E
    assert _adam(lib, [nets[0], twin], parts, [1, 1]) == E and _adam(lib, nets, [parts[0], parts[0]], [1, 1]) == E
    # update counts start at 1; no moments; no rows
    assert _adam(lib, nets, parts, [1, 0]) == E and _adam(lib, nets, parts, [-2, 1]) == E
    no_m = _net(1)
    no_m.m = None
    assert _adam(lib, [nets[0], no_m], parts, [1, 1]) == E and _adam(lib, nets, parts, [1, 1], n_partials=0) == E
    # misaligned pointers: pairs off 8 bytes, partials / local / target off 16
    assert _grad(lib, nets, parts, pairs=0x8000004) == E and _grad(lib, nets, [parts[0], parts[1] + 8]) == E
    off = _net(1)
    off.local = off.local + 4
    assert _grad(lib, [nets[0], off], parts) == E
    off = _net(1)
    off.target = off.target + 8
    assert _grad(lib, [nets[0], off], parts) == E
    assert _adam(lib, nets, [parts[0], parts[1] + 4], [1, 1]) == E
    # what uavenv_dqn_grad refuses of the ring and the batch
    assert _grad(lib, nets, parts, batch=65) == E and _grad(lib, nets, parts, batch=0) == E
    bad = _ring()
    bad.action_is_index = 0
    assert _grad(lib, nets, parts, ring=bad) == E
    bad = _ring()
    bad.frames = 1
    assert _grad(lib, nets, parts, ring=bad) == E
    no_target = _net(1)
    no_target.target = None
    assert _grad(lib, [nets[0], no_target], parts) == E
    # the setter
    assert lib.uavenv_dqn_slots_loop_set_multi_update(None, 1) == E


# ---- learner.update_slots / DQNSlotsHotLoop(multi_update=True): the Python objects are checked before the library is loaded -----

def test_update_slots_refuses_bad_arguments_before_any_library_call(no_library):  # noqa: F811
    from dqn_based_uav_3d_path_planer_amd.learner import update_slots
    from dqn_based_uav_3d_path_planer_amd.loop import DQNSlotsHotLoop
    two = [_L(), _L()]
    pairs = torch.zeros((2, 64, 2), dtype=torch.int32)
    ring = _Ring()
    lists = {
        "none": None, "empty": [], "nine": [_L() for _ in range(9)], "one learner twice": [two[0], two[0]],
        "n_actions differ": [two[0], _L(n_actions=4)], "head shapes differ": [two[0], _L(dueling=True, kind="dueling")],
        "f16 MFMA": [two[0], _L(mfma="f16")], "not a fused learner": [two[0], 3],
        "kinds differ": [two[0], _L(kind="ddqn")], "hyper-parameters differ": [two[0], _L(lr=2e-3)],
    }
    for name, ls in lists.items():
        with pytest.raises(ValueError):
            update_slots(ls, ring, 64, pairs)
    with pytest.raises(ValueError, match="pairs must be a contiguous"):          # the list's length is the pairs' first dimension
        update_slots(two + [_L()], ring, 64, pairs)
    bad_pairs = {
        "dtype": torch.zeros((2, 64, 2), dtype=torch.int64), "float": torch.zeros((2, 64, 2)),
        "another batch": torch.zeros((2, 128, 2), dtype=torch.int32), "flat": torch.zeros((128, 2), dtype=torch.int32),
        "three columns": torch.zeros((2, 64, 3), dtype=torch.int32),
        "not contiguous": torch.zeros((2, 64, 4), dtype=torch.int32)[:, :, ::2], "none": None,
    }
    assert tuple(bad_pairs["not contiguous"].shape) == (2, 64, 2)
    for name, p in bad_pairs.items():
        with pytest.raises(ValueError, match="pairs must be a contiguous"):
            update_slots(two, ring, 64, p)
    for batch in (65, 0, -64):
        with pytest.raises(ValueError, match="batch % 64"):
            update_slots(two, ring, batch, torch.zeros((2, max(batch, 0), 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="packed ring"):
        update_slots(two, _Ring(discrete=False), 64, pairs)

    class F32Env(_Env):
        packed = False
    with pytest.raises(ValueError, match="packed ring"):
        update_slots(two, _Ring(F32Env()), 64, pairs)
    with pytest.raises(ValueError, match="one per learner"):
        update_slots(two, ring, 64, pairs, images=[None])
    # everything above passed for these arguments: what is left is that the pairs are not on a device (there is none here)
    with pytest.raises(ValueError, match="on the device"):
        update_slots(two, ring, 64, pairs)
    # the loop's option changes nothing about its checks: a good list gets as far as the library, a bad one does not
    four = [_L() for _ in range(4)]
    with pytest.raises(AssertionError, match="library was loaded"):
        DQNSlotsHotLoop(_Ring(), four, 64, seed=1, multi_update=True)
    with pytest.raises(ValueError):
        DQNSlotsHotLoop(_Ring(), four[:3] + [_L(lr=2e-3)], 64, seed=1, multi_update=True)
