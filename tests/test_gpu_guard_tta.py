"""Guard-band cases (tests/_guard.py) for the launch functions of include/dd_tta.h (csrc/libdd_tta.so): both inputs and the output
operands of their own with 64 KiB of 0xFF around them, at the 16-byte alignment the header states and no more.  What a case asserts:
tests/test_gpu_guard_dense.py.

Neither launcher picks a kernel by alignment (the shape alone decides: w % 16, w % 4), so the two modes are compared bit for bit.
The shapes: (3,5,7) the scalar form with an odd h and a tail, (3,4,8) four columns per lane, (2,6,16) sixteen columns per lane in the
byte form.  tests/test_tta_surface.py checks, without a GPU, that every function of the header is the subject of a case here.

An over-read whose value is discarded cannot be seen by these tests."""
import pytest
import torch

import _tta_ref as ref
from _guard import Case, Check, run_case

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = ((3, 5, 7), (3, 4, 8), (2, 6, 16))      # all far inside the arena's 8 MiB
TAU = 0.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import tta
    tta.lib()
    return torch.device("cuda:0")


CASES = []


def inputs(shape, from_logits):
    lo, hi = (-12.0, 12.0) if from_logits else (0.0, 1.0)
    return (synth.hash_uniform(shape, synth.key_salt("gttaa"), lo, hi), synth.hash_uniform(shape, synth.key_salt("gttam"), lo, hi))


def _case(entry, shape, from_logits):
    def fn(arena, mode):
        from driving_dirty_amd import tta
        a0, m0 = inputs(shape, from_logits)
        a, m = arena.put(a0, 16, "a"), arena.put(m0, 16, "m")
        want = ref.mean_prob(a0.to(arena.dev), m0.to(arena.dev), from_logits)
        if entry == "dd_tta_mean_prob":
            out = arena.out(shape, torch.float32, 16, "out")
            tta.launch(entry, a, m, out, *shape, int(from_logits))
            return [Check("out", arena.verify()["out"], want.cpu(), how="exact")]
        out = arena.out(shape, torch.uint8, 16, "out")
        tta.launch(entry, a, m, TAU, out, *shape, int(from_logits))
        return [Check("out", arena.verify()["out"], ref.gt(want, TAU).to(torch.uint8).cpu(), how="exact")]
    return fn


for _entry in ("dd_tta_mean_prob", "dd_tta_mean_gt"):
    for _shape in SHAPES:
        for _logits in (False, True):
            CASES.append(Case(f"{_entry}[{','.join(map(str, _shape))}]{'[logits]' if _logits else '[probs]'}", _entry,
                              _case(_entry, _shape, _logits)))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
