"""GPU tests of the two kernels of include/dd_tta.h (csrc/libdd_tta.so) against tests/_tta_ref.py, on raw bits: the feature is built
from exact pieces (one sigmoid shared bit for bit, one rounded add, an exact halving, a strict comparison), so there is no tolerance.

Shapes: (1,1,4) one group; (2,3,4) an odd h, the middle row pairs with itself; (3,5,7) the scalar form with a tail; (2,8,8) four
columns per lane; (2,6,16) one 16-column group per row in the byte form; (70,2,4) many samples (the launchers cut nothing into
chunks: one launch serves any batch); (2,800,800) the real plane once, more than one workgroup and the grid-stride loop."""
import pytest
import torch

import _tta_ref as ref

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4), (2, 3, 4), (3, 5, 7), (2, 8, 8), (2, 6, 16), (70, 2, 4), (2, 800, 800)]
TAUS = (0.5, 0.25, 250 / 256)
INF, NAN = float("inf"), float("nan")
PLANTED = [INF, -INF, 88.0, -88.0, 104.0, -104.0, 1e-40, -1e-40, 0.0, -0.0, NAN]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import tta
    tta.lib()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def inputs(shape, kind, dev):
    """(a, m) on the device.  ``planted``: the special logits at the front of ``a`` (as many as fit) and, shifted by three, at the end
    of ``m``, so that they meet ordinary values and each other."""
    lo, hi = (0.0, 1.0) if kind == "probs" else (-12.0, 12.0)
    a = synth.hash_uniform(shape, synth.key_salt("ttaa"), lo, hi)
    m = synth.hash_uniform(shape, synth.key_salt("ttam"), lo, hi)
    if kind == "planted":
        k = min(len(PLANTED), a.numel())
        a.reshape(-1)[:k] = torch.tensor(PLANTED[:k])
        m.reshape(-1)[-k:] = torch.tensor((PLANTED[3:] + PLANTED[:3])[:k])
    return a.to(dev), m.to(dev)


@pytest.fixture(scope="module")
def cases(dev):
    """{(shape, kind): (a, m, reference mean)}, computed once and left unchanged."""
    out = {}
    for shape in SHAPES:
        for kind in ("probs", "logits", "planted"):
            a, m = inputs(shape, kind, dev)
            out[shape, kind] = (a, m, ref.mean_prob(a, m, kind != "probs"))
    return out


@pytest.mark.parametrize("kind", ["probs", "logits", "planted"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_equal_the_reference_on_bits(dev, cases, shape, kind):
    from driving_dirty_amd import tta
    a, m, want = cases[shape, kind]
    a0, m0 = a.clone(), m.clone()
    got = tta.mean_prob(a, m, kind != "probs")
    assert got.dtype == torch.float32 and tuple(got.shape) == shape and got.is_contiguous()
    assert torch.equal(bits(got), bits(want))
    if kind == "probs":
        assert torch.equal(bits(got), bits(ref.mean_prob_cpu(a.cpu(), m.cpu()).to(dev)))      # without any kernel of the package
    if kind == "planted" and a.numel() >= len(PLANTED):
        assert int(torch.isnan(got).sum()) == 2 and float(got[~torch.isnan(got)].max()) <= 1.0
    for tau in TAUS:
        mask = tta.mean_gt(a, m, tau, kind != "probs")
        assert mask.dtype == torch.bool and tuple(mask.shape) == shape
        assert int(mask.view(torch.uint8).max()) <= 1, "the byte output holds only 0 and 1"
        assert torch.equal(mask, ref.gt(want, tau)), tau
        assert torch.equal(mask, got > tau), "element for element what mean_prob(...) > tau gives"
        assert not bool(mask[torch.isnan(got)].any()), "a NaN mean is not set"
    assert torch.equal(bits(a), bits(a0)) and torch.equal(bits(m), bits(m0))


@pytest.mark.parametrize("kind", ["probs", "planted"])
@pytest.mark.parametrize("shape", [(2, 3, 4), (3, 5, 7), (2, 6, 16), (2, 800, 800)], ids=lambda s: "x".join(map(str, s)))
def test_swap_symmetry(dev, cases, shape, kind):
    """fp32 addition commutes: mean(a, m)[b,r,c] and mean(m, a)[b,h-1-r,c] are the same bits."""
    from driving_dirty_amd import tta
    a, m, _ = cases[shape, kind]
    logits = kind != "probs"
    assert torch.equal(bits(tta.mean_prob(a, m, logits)), bits(tta.mean_prob(m, a, logits).flip(1)))
    assert torch.equal(tta.mean_gt(a, m, 0.5, logits), tta.mean_gt(m, a, 0.5, logits).flip(1))


@pytest.mark.parametrize("shape", [(2, 3, 4), (3, 5, 7), (2, 6, 16)], ids=lambda s: "x".join(map(str, s)))
def test_a_mean_of_exactly_tau_is_not_set_and_the_next_fp32_above_is(dev, shape):
    from driving_dirty_amd import tta
    b, h, w = shape
    a, m = torch.zeros(shape), torch.zeros(shape)
    for r in range(h):      # every row, the middle one of an odd h included (it pairs with itself: 0.5 + 0.5)
        a[b - 1, r, 0], m[b - 1, h - 1 - r, 0] = 0.25, 0.75                      # mean exactly 0.5
        a[b - 1, r, w - 1], m[b - 1, h - 1 - r, w - 1] = 0.25 + 2.0 ** -23, 0.75      # sum 1 + 2^-23: the mean is the next fp32 above 0.5
    if h % 2:
        mid = h // 2
        a[0, mid, 1] = m[0, mid, 1] = 0.5
    a, m = a.to(dev), m.to(dev)
    mean = tta.mean_prob(a, m, False)
    above = torch.nextafter(torch.tensor(0.5), torch.tensor(1.0)).item()
    assert bool((mean[b - 1, :, 0] == 0.5).all()) and bool((mean[b - 1, :, w - 1] == above).all())
    mask = tta.mean_gt(a, m, 0.5, False)
    assert not bool(mask[b - 1, :, 0].any()), "mean == tau: NOT set (strictly greater)"
    assert bool(mask[b - 1, :, w - 1].all()), "the next fp32 above tau: set"
    assert int(mask.sum()) == h
    assert bool(tta.mean_gt(a, m, above, False).sum() == 0) and int(tta.mean_gt(a, m, 0.25, False).sum()) == 2 * h + (h % 2)
    # tau is rounded to fp32 on its way in: 0.5 + 2^-30 is 0.5 there
    assert torch.equal(tta.mean_gt(a, m, 0.5 + 2.0 ** -30, False), mask)


def test_the_wrappers_check_their_operands_before_any_launch(dev, monkeypatch):
    from driving_dirty_amd import tta
    launched = []
    monkeypatch.setattr(tta, "launch", lambda *args: launched.append(args))
    a = torch.zeros(2, 4, 8, device=dev)
    for bad in (a.cpu(), a.double(), a.transpose(1, 2), a[:, :, :4], a.reshape(2, 32), a[:0]):
        with pytest.raises(tta.HotpathError):
            tta.mean_prob(bad, bad, False)
    with pytest.raises(tta.HotpathError):
        tta.mean_gt(a, a[:1], 0.5, True)
    with pytest.raises(tta.HotpathError):
        tta.mean_gt(a, a.cpu(), 0.5, True)
    assert not launched
    tta.mean_gt(a, a, 0.5, True)
    assert len(launched) == 1 and launched[0][0] == "dd_tta_mean_gt" and launched[0][-4:] == (2, 4, 8, 1)
