"""k_dqn_reduce_adam takes the operands of its loads -- the gate word among them -- as its first 14 dwords of kernel arguments, which
gfx950 hands a wavefront in scalar registers when it starts (kernel-argument preload), requests the gate word first and tests it
behind the issue of every other load.  It is held, byte for byte, against a twin whose arguments travel another way -- so that a
mis-ordered or mis-aligned leading argument cannot cancel out --: k_dqn_reduce_adam_slots with one slot, which takes a table in a
struct (never preloaded) and shares the body text.

 * uavenv_dqn_reduce_adam_img against uavenv_dqn_reduce_adam_slots_img with one slot: 1, 3 and 256 partial rows, hard update off and
   on, with an image, no gate and a gate word that matches: parameters, target, moments, loss, column sums, both image halves;
 * with a gate word that does not match, every one of those is left bit for bit as it was by both kernels (the loads now run ahead
   of the test; no store may), and the partial rows are never written.

(The step and gradient kernels take their arguments as the parent commit's do: leading arguments for them were measured and dropped,
profiles/kernarg_preload_ab.txt.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_dqn_act_kernels_gpu import Net, fresh_flat
from test_dqn_slots_loop_gpu import net_array, stream
from test_dqn_update_slots_gpu import adam_state, bits, ptrs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gate", ["none", "match", "miss"])
@pytest.mark.parametrize("hard", [0, 1])
@pytest.mark.parametrize("rows", [1, 3, 256])
def test_reduce_adam_equals_one_slot_and_a_missed_gate_stores_nothing(rows, hard, gate):
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng([rows, hard])
    lr, b1, b2, eps, step_t = 1e-3, 0.9, 0.999, 1e-8, 4
    word = torch.tensor([77], dtype=torch.int32, device="cuda")
    go, go_value = (None, 0) if gate == "none" else (word.data_ptr(), 77 if gate == "match" else 78)
    one = Net(fresh_flat(3, False, 5), 3, False, "f32")
    one.buf[1].mul_(1.0 + 1.0 / 64.0)                                       # a target that differs from the parameters
    parts = adam_state([one], rng, rows, 64.0)[0]                           # (sets non-zero moments too)
    twin = Net(one.flat, 3, False, "f32")
    twin.buf.copy_(one.buf)
    P = one.flat.size
    img, twin_img = one.image(), twin.image()
    start, start_img, start_parts = one.buf.clone(), img.clone(), parts.clone()
    assert not torch.equal(img[:L.DQN_IMAGE_FLOATS], img[L.DQN_IMAGE_FLOATS:])
    loss = [torch.full((), -5.0, device="cuda") for _ in range(2)]
    raw = [torch.full((P + 2,), -5.0, device="cuda") for _ in range(2)]
    assert lib.uavenv_dqn_reduce_adam_img(C.byref(one.net), parts.data_ptr(), rows, lr, b1, b2, eps, step_t, hard, loss[0].data_ptr(),
                                          raw[0].data_ptr(), go, go_value, img.data_ptr(), stream()) == 0
    st, hd = (C.c_int32 * 1)(step_t), (C.c_int32 * 1)(hard)
    assert lib.uavenv_dqn_reduce_adam_slots_img(net_array([twin]), 1, ptrs([parts]), rows, lr, b1, b2, eps, st, hd, ptrs(loss[1:]),
                                                ptrs(raw[1:]), go, go_value, ptrs([twin_img]), stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(one.buf), bits(twin.buf))                    # local, target, m, v
    assert np.array_equal(bits(loss[0]), bits(loss[1])) and np.array_equal(bits(raw[0]), bits(raw[1]))
    assert np.array_equal(bits(img), bits(twin_img))                        # both halves
    assert np.array_equal(bits(parts), bits(start_parts))
    if gate == "miss":
        for t in (one, twin):
            assert np.array_equal(bits(t.buf), bits(start))
        for t in (img, twin_img):
            assert np.array_equal(bits(t), bits(start_img))
        for t in loss + raw:
            assert np.all(bits(t) == np.float32(-5.0).view(np.uint32))
    else:
        assert not torch.equal(one.buf[0, :P], start[0, :P]) and not torch.equal(one.buf[2:, :P], start[2:, :P])
        assert not torch.equal(img[:L.DQN_IMAGE_FLOATS], start_img[:L.DQN_IMAGE_FLOATS])
        assert torch.equal(one.buf[1, :P], one.buf[0, :P]) == bool(hard)
        assert torch.equal(img[L.DQN_IMAGE_FLOATS:], img[:L.DQN_IMAGE_FLOATS]) == bool(hard)
        assert float(loss[0]) != -5.0 and np.isfinite(raw[0].cpu().numpy()).all()
