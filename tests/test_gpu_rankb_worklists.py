"""GPU tests of the rank-B optimizer pass (``dd_adam_step_rankb``, csrc/adam_rankb.hip) where no other test compares it with fp64: 33 to 63
batch rows (a partly filled second 32-row chunk), row counts above 16 that are no multiple of 8 (rows past M fetched through the
wave-uniform offset of the load), more than one tile per workgroup in the ``short`` and ``wide`` forms, pieces of the work list that
change their dY tile in the middle, workgroups that come up empty, and the four ``devscale_*`` kernels.  The cases and their classes:
tests/_rankb_ref.py (``CASES``; tests/test_rankb_ref.py holds each to ``plan``, the launcher's host arithmetic restated).

Per case, signed and unsigned factors, with and without the bias:
(a) one step from zero moments, every element of m, v, bias_m, bias_v inside the bounds derived in tests/_rankb_ref.py;
(b) three steps under the bounds of tests/test_gpu_round5.py::test_adam_rankb_matches_fp64 (m, v, bias_m 2e-6 of peak; p 1e-6 of peak
    on unsigned factors, 0.2 lr on signed ones), and the same 2e-6 for bias_v and 1e-6 for the bias on unsigned factors;
(c) ``dd_adam_step_rankb_dev`` with a device scale of 0.37 gives the bits of the by-value call;
(d) a second launch on the same operands gives the same bits;
and the ``wide`` cases agree bit for bit with one workgroup per CU (the ``lds<1,2>`` form), as
tests/test_gpu_round5.py::test_adam_rankb_wide_tiles_for_the_pass_by_itself_equal_the_budgeted_kernel.

Observed on an MI355X: the worst fractions of the derived bounds used in (a) over all cases are recorded in DESIGN.md 3.2b."""
import functools

import pytest
import torch

import _rankb_ref as ref

pytestmark = pytest.mark.gpu

LR, EPS = 1e-3, 1e-8
B1, B2 = float(torch.tensor(0.9, dtype=torch.float32)), float(torch.tensor(0.999, dtype=torch.float32))      # the kernels' fp32 betas
IDS = [f"rows{c[0]}-{c[1]}x{c[2]}-blocks{c[3]}-spare{c[4]}-{cls[0]}" for c, cls in ref.CASES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _adam64(p, m, v, g, step):
    """torch.optim.Adam's arithmetic in fp64 (tests/test_gpu_round5.py::_adam64)."""
    m.mul_(B1).add_(g, alpha=1 - B1)
    v.mul_(B2).addcmul_(g, g, value=1 - B2)
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    p.addcdiv_(m, (v.sqrt() / bc2 ** 0.5).add_(EPS), value=-LR / bc1)


@functools.lru_cache(maxsize=1)
def _reference(rows, n, k, signed):
    """The factors of three steps and the fp64 state after them: computed once per (shape, signedness), shared by the runs with and
    without the bias (the weight's state does not depend on it) and never written to."""
    gen = torch.Generator().manual_seed(n * 7 + k + rows)
    p0, b0 = torch.rand(n, k, generator=gen) - 0.5, torch.rand(n, generator=gen) - 0.5
    pr, mr, vr = p0.double(), torch.zeros(n, k, dtype=torch.float64), torch.zeros(n, k, dtype=torch.float64)
    br, bmr, bvr = b0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    steps = []
    for step in (1, 2, 3):
        x, dy = ref.factors(rows, n, k, signed, step, gen)
        gw, gb = ref.grad64(dy, x)
        _adam64(pr, mr, vr, gw, step)
        _adam64(br, bmr, bvr, gb, step)
        steps.append((x, dy))
    return p0, b0, steps, (pr, mr, vr, br, bmr, bvr)


def _bits_equal(a, b):
    return all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("case,cls", ref.CASES, ids=IDS)
def test_rankb_worklist_case(dev, case, cls, signed, with_bias):
    from driving_dirty_amd import _lib, ops
    lib = _lib.lib()
    rows, n, k, blocks, spare = case
    p0, b0, steps, (pr, mr, vr, br, bmr, bvr) = _reference(rows, n, k, signed)
    on_dev = [(x.to(dev), dy.to(dev)) for x, dy in steps]

    def fresh():
        w = [p0.to(dev), torch.zeros(n, k, device=dev), torch.zeros(n, k, device=dev)]
        b = [b0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
        return w, b

    def launch(w, b, step, scale=1.0):
        x, dy = on_dev[min(step, 3) - 1]
        ops.adam_step_rankb(*w, dy, x, *(b if with_bias else (None, None, None)), LR, 0.9, 0.999, EPS, step, scale)

    def three_steps():
        w, b = fresh()
        first = None
        for step in (1, 2, 3):
            launch(w, b, step)
            if step == 1:
                first = [t.clone() for t in w + b]
        return w, b, first

    assert lib.dd_set_adam_blocks_per_cu(blocks) == 0 and lib.dd_set_adam_spare_cus(spare) == 0
    try:
        w, b, first = three_steps()
        # (d) the first step again, on the same operands
        w2, b2 = fresh()
        launch(w2, b2, 1)
        # (c) a fourth step from the state after the first, the scale by value and from device memory
        sdev = torch.tensor([0.37], device=dev, dtype=torch.float32)
        by_value, by_dev = [t.clone() for t in first], [t.clone() for t in first]
        launch(by_value[:3], by_value[3:], 4, float(sdev.item()))
        launch(by_dev[:3], by_dev[3:], 4, sdev)
        narrow = None
        if cls[0] == "wide":
            assert lib.dd_set_adam_blocks_per_cu(1) == 0
            narrow = three_steps()
    finally:
        assert lib.dd_set_adam_blocks_per_cu(1) == 0 and lib.dd_set_adam_spare_cus(0) == 0
    torch.cuda.synchronize()

    # (a) one step from zero moments: every element inside its derived bound
    x1, dy1 = steps[0]
    frac = ref.first_step_fractions(dy1, x1, first[1], first[2], first[4] if with_bias else None, first[5] if with_bias else None)
    print(f"{cls[0]} rows {rows} {n}x{k} signed {signed} bias {with_bias}: fraction of the derived bounds used "
          + ", ".join(f"{key} {f:.3f}" for key, f in frac.items()))
    assert all(f <= 1.0 for f in frac.values()), frac
    assert set(frac) == ({"m", "v", "bias_m", "bias_v"} if with_bias else {"m", "v"})
    # (b) three steps
    rel = lambda a, r: float((a.double().cpu() - r).abs().max() / r.abs().max().clamp_min(1e-30))
    assert rel(w[1], mr) < 2e-6 and rel(w[2], vr) < 2e-6
    if signed:
        assert float((w[0].double().cpu() - pr).abs().max()) < 0.2 * LR
    else:
        assert rel(w[0], pr) < 1e-6
    if with_bias:
        assert rel(b[1], bmr) < 2e-6 and rel(b[2], bvr) < 2e-6
        assert signed or rel(b[0], br) < 1e-6
    else:
        assert torch.equal(b[0].cpu(), b0) and float(b[1].abs().max()) == 0.0 and float(b[2].abs().max()) == 0.0
    # (c) the device scale's kernel gives the by-value kernel's bits, and both moved
    assert _bits_equal(by_value, by_dev)
    assert not torch.equal(by_value[0], first[0]) and torch.equal(by_value[3], first[3]) == (not with_bias)
    # (d)
    assert _bits_equal(w2 + b2, first)
    if narrow is not None:
        assert _bits_equal(narrow[0] + narrow[1], w + b) and _bits_equal(narrow[2], first)
