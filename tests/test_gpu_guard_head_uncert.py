"""Guard-band cases (tests/_guard.py) for the launch function of include/dd_head_uncert.h (csrc/libdd_head_uncert.so): the latents, the
weight, the bias, every requested map, the partials and the scores as operands of their own with 64 KiB of 0xFF around them, at the
alignment the header states and no more (16 bytes; the bias 4; the fp64 operands 8).  What a case asserts: tests/test_gpu_guard_dense.py.

The launcher picks its kernel by the rows of a launch alone, so the two modes are compared bit for bit.  The shapes (scenes, S, n, k),
the smallest of tests/_head_uncert_cases.py: (3,3,16,4) one row tile, 16-byte stores; (5,16,130,68) 80 rows = two launches of two row
tiles and of one, a ragged second column block, n % 4 != 0: the element-wise stores; (33,2,100,64) more than 8 scenes to a launch and
a second launch of one scene, n % 16 != 0.  Each with every output, with the scores alone and with one map alone.  ``partials`` is
exactly ceil(n / 128) * scenes * 3 doubles and has to come back finite: every triple of it is written.

An over-read whose value is discarded cannot be seen by these tests."""
import pytest
import torch

import _head_uncert_ref as ref
from _guard import Case, Check, run_case

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = ((3, 3, 16, 4), (5, 16, 130, 68), (33, 2, 100, 64))      # all far inside the arena's 8 MiB
REQUESTS = ((("mean", "entropy", "mi", "var"), True), ((), True), (("mi",), False))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import uncertainty
    uncertainty.lib()
    return torch.device("cuda:0")


CASES = []


def inputs(scenes, samples, n, k):
    a = 3.0 / k ** 0.5
    return (synth.hash_uniform((scenes * samples, k), synth.key_salt("ghux"), -1.0, 1.0), synth.hash_uniform((n, k), synth.key_salt("ghuw"), -a, a),
            synth.hash_uniform((n,), synth.key_salt("ghub"), -0.5, 0.5))


def _case(shape, maps, scores):
    scenes, samples, n, k = shape

    def fn(arena, mode):
        from driving_dirty_amd import uncertainty
        x0, w0, b0 = inputs(*shape)
        x, w, b = arena.put(x0, 16, "x"), arena.put(w0, 16, "w"), arena.put(b0, 4, "bias")
        want, bound = ref.stats64(x0.numpy(), w0.numpy(), b0.numpy(), samples)
        out = {m: arena.out((scenes, n), torch.float32, 16, m) for m in maps}
        if scores:
            out["partials"] = arena.out(((n + uncertainty.BLOCK - 1) // uncertainty.BLOCK, scenes, 3), torch.float64, 8, "partials")
            out["scores"] = arena.out((scenes, 3), torch.float64, 8, "scores")
        uncertainty.launch("dd_head_uncert", x, w, b, *(out.get(m) for m in uncertainty.MAPS), out.get("partials"), out.get("scores"), scenes,
                           samples, n, k)
        got = arena.verify()
        checks = []
        for name in maps + (("scores",) if scores else ()):
            err = (got[name].double() - torch.from_numpy(getattr(want, name))).abs()
            assert bool((err <= torch.from_numpy(getattr(bound, name))).all()), (name, float(err.max()))      # element by element, at its own bound
            checks.append(Check(name, got[name], getattr(want, name), how="asserted"))
        return checks
    return fn


for _shape in SHAPES:
    for _maps, _scores in REQUESTS:
        CASES.append(Case(f"dd_head_uncert[{','.join(map(str, _shape))};{'+'.join(_maps) or 'none'};{'scores' if _scores else 'maps'}]",
                          "dd_head_uncert", _case(_shape, _maps, _scores)))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
