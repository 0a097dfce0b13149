"""Guard-band cases (tests/_guard.py) for the launch functions of include/dd_augment.h (csrc/libdd_augment.so): every per-sample
input an operand of its own with 64 KiB of 0xFF around it, at the alignment the header promises to accept and no more -- bytes at
1, fp32 views at 4, outputs at 16.  What a case asserts: tests/test_gpu_guard_dense.py.

The arena places nothing below 2 bytes, so in the minimal mode a byte operand carries one leading byte and starts behind it: an
odd address.  None of the launchers picks a kernel by alignment (one kernel serves every address), so the two modes are compared
bit for bit.  tests/test_augment_surface.py checks, without a GPU, that every function of the header is the subject of a case here.

An over-read whose value is discarded cannot be seen by these tests."""
import ctypes as C

import pytest
import torch

import _augment_ref as ref
from _guard import Case, Check, ptr_table, run_case

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import augment
    augment.lib()
    return torch.device("cuda:0")


CASES = []
B = 3
FLAGS = [1 | (1 << 12), 0, 1]      # mirrored with view 4 blanked; plain; mirrored
COLOR = torch.tensor([[[1.0, 0.0], [3.0, 0.25], [0.625, -0.125], [1.0, 0.0], [2.5, -0.5], [1.0, 0.375]][(i + v) % 6]
                      for i in range(B) for v in range(6)]).reshape(B, 6, 2)


def case(name, entry, **kw):
    def deco(fn):
        CASES.append(Case(name, entry, fn, **kw))
        return fn
    return deco


def put_bytes(arena, mode, t, name):
    """A byte operand at 1-byte alignment: in the minimal mode one leading byte in front of it, which is skipped (an odd address)."""
    off = 1 if mode == "minimal" else 0
    flat = torch.cat([torch.zeros(off, dtype=torch.uint8), t.contiguous().view(torch.uint8).flatten()])
    out = arena.put(flat, 2, name)[off:]
    assert (out.data_ptr() % 2 == 1) == (mode == "minimal")
    return out


def host(flags, color=None):
    cflags = (C.c_uint32 * len(flags))(*flags)
    return cflags if color is None else (cflags, (C.c_float * color.numel())(*color.flatten().tolist()))


def _views(u8, h, w):
    def fn(arena, mode):
        from driving_dirty_amd import augment
        if u8:
            x0 = (synth.hash_uniform((B, 6, h, w, 3), synth.key_salt("gaugf"), 0.0, 1.0) * 255).round().to(torch.uint8)
            samples = [put_bytes(arena, mode, x0[i], f"frames{i}") for i in range(B)]
        else:
            x0 = synth.hash_uniform((B, 6, 3, h, w), synth.key_salt("gaugv"))
            samples = [arena.put(x0[i], 4, f"views{i}") for i in range(B)]
        out = arena.out((B, 6, 3, h, w), torch.float32, 16, "out")
        augment.launch("dd_aug_views_u8_ptrs" if u8 else "dd_aug_views_ptrs", ptr_table(samples), *host(FLAGS, COLOR), out, B, h, w)
        return [Check("out", arena.verify()["out"], ref.views(x0, FLAGS, COLOR), how="exact")]
    return fn


for _h, _w in ((2, 3), (5, 7), (16, 22)):      # the flat kernel, with a scalar tail at (5, 7) (18 H W % 4 != 0); the plane kernel at (16, 22)
    case(f"dd_aug_views_u8_ptrs[{B},{_h},{_w}]", "dd_aug_views_u8_ptrs")(_views(True, _h, _w))
    case(f"dd_aug_views_ptrs[{B},{_h},{_w}]", "dd_aug_views_ptrs")(_views(False, _h, _w))


def _masks(h, w):
    def fn(arena, mode):
        from driving_dirty_amd import augment
        m0 = (synth.hash_uniform((B, h, w), synth.key_salt("gaugm"), 0.0, 1.0) * 255).round().to(torch.uint8)
        masks = [put_bytes(arena, mode, m0[i], f"mask{i}") for i in range(B)]
        out = arena.out((B, h, w), torch.uint8, 16, "out")
        augment.launch("dd_aug_masks_u8_ptrs", ptr_table(masks), host(FLAGS), out, B, h, w)
        return [Check("out", arena.verify()["out"], ref.masks(m0, FLAGS), how="exact")]
    return fn


for _h, _w in ((3, 4), (5, 7), (8, 8), (40, 40)):      # (5, 7): 105 bytes, a byte tail; (8, 8) / (40, 40): whole words, loaded as words where aligned
    case(f"dd_aug_masks_u8_ptrs[{B},{_h},{_w}]", "dd_aug_masks_u8_ptrs")(_masks(_h, _w))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
