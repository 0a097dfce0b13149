"""Guard-band cases (tests/_guard.py) for the launch functions of include/dd_head_mean.h (csrc/libdd_head_mean.so): the latents, the
weight, the bias and the output operands of their own with 64 KiB of 0xFF around them, at the 16-byte alignment the header states and
no more (the bias at 4).  What a case asserts: tests/test_gpu_guard_dense.py.

Neither launcher picks a kernel by alignment (the shape alone decides: the rows of a launch, n % 4, n % 16), so the two modes are
compared bit for bit.  The shapes (scenes, S, n, k), the smallest of tests/test_gpu_head_mean.py: (3,3,16,4) one row tile, 16-byte
stores both ways; (5,16,130,68) 80 rows = two launches of two row tiles and of one, a ragged second column block, n % 4 != 0: the
element-wise fp32 store and the byte-wise map; (70,1,100,64) S = 1 past 64 rows, n % 16 != 0.  tests/test_head_mean_surface.py checks,
without a GPU, that every function of the header is the subject of a case here.

An over-read whose value is discarded cannot be seen by these tests."""
import pytest
import torch

import _head_mean_ref as ref
from _guard import Case, Check, run_case

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = ((3, 3, 16, 4), (5, 16, 130, 68), (70, 1, 100, 64))      # all far inside the arena's 8 MiB
TAU = 0.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import mc
    mc.lib()
    return torch.device("cuda:0")


CASES = []


def inputs(scenes, samples, n, k):
    a = 3.0 / k ** 0.5
    return (synth.hash_uniform((scenes * samples, k), synth.key_salt("ghmx"), -1.0, 1.0), synth.hash_uniform((n, k), synth.key_salt("ghmw"), -a, a),
            synth.hash_uniform((n,), synth.key_salt("ghmb"), -0.5, 0.5))


def _case(entry, shape):
    scenes, samples, n, k = shape

    def fn(arena, mode):
        from driving_dirty_amd import mc
        x0, w0, b0 = inputs(*shape)
        x, w, b = arena.put(x0, 16, "x"), arena.put(w0, 16, "w"), arena.put(b0, 4, "bias")
        want64, bound = ref.mean_prob64(x0, w0, b0, samples, with_bound=True)
        if entry == "dd_head_mean_prob":
            out = arena.out((scenes, n), torch.float32, 16, "out")
            mc.launch(entry, x, w, b, out, scenes, samples, n, k)
            return [Check("out", arena.verify()["out"], want64, bound, how="abs")]
        out = arena.out((scenes, n), torch.uint8, 16, "out")
        mc.launch(entry, x, w, b, TAU, out, scenes, samples, n, k)
        got = arena.verify()["out"]
        sure = (want64 - TAU).abs() > bound      # where fp32 cannot land on the other side
        assert bool((got <= 1).all()) and bool(sure.float().mean() > 0.99) and torch.equal(got.bool()[sure], (want64 > TAU)[sure])
        return [Check("out", got, (want64 > TAU).to(torch.uint8), how="asserted")]
    return fn


for _entry in ("dd_head_mean_prob", "dd_head_mean_gt"):
    for _shape in SHAPES:
        CASES.append(Case(f"{_entry}[{','.join(map(str, _shape))}]", _entry, _case(_entry, _shape)))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
