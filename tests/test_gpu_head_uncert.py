"""GPU tests of the sampled head's uncertainty kernel (include/dd_head_uncert.h) over the grid of tests/_head_uncert_cases.py: ``mean``
bit for bit ``mc.mean_prob``; every other map within its TIGHT bound (the formulas' rounding alone, tests/_head_uncert_ref.py) of the
fp64 statistics of the product's own logits (``ops.linear``), and within the LOOSE bound of the pure-fp64 reference; the scores within
the mean of the elements' bounds, and the same bits whatever else is written; nothing written outside the outputs or by a refused call."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _head_uncert_cases as cases  # noqa: E402
import _head_uncert_ref as ref  # noqa: E402

SENTINEL = 0xA5
BAND = 4096      # bytes of sentinel on either side of an output
STAT_MAPS = ("entropy", "mi", "var")
LN2 = float(np.log(2.0))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import mc, uncertainty
    mc.lib()
    uncertainty.lib()
    return torch.device("cuda:0")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def product_logits(x, w, b):
    """``ops.linear(x, w, b)`` [M, N] for any N (the weight padded with zero rows to a multiple of 4, the result cut back): the kernel's
    own logit bits."""
    from driving_dirty_amd import ops
    n = w.shape[0]
    pad = (-n) % 4
    if pad:
        w = torch.cat([w, torch.zeros((pad, w.shape[1]), device=w.device)])
        b = None if b is None else torch.cat([b, torch.zeros(pad, device=b.device)])
    with torch.no_grad():
        return ops.linear(x, w.contiguous(), b)[:, :n].contiguous()


class Banded:
    """Outputs of one launch, each inside a band of 0xA5 bytes."""

    def __init__(self, dev, scenes, n, maps, scores):
        from driving_dirty_amd import uncertainty
        self.bufs, self.views = {}, {}
        sizes = {m: (scenes * n * 4, torch.float32, (scenes, n)) for m in maps}
        if scores:
            nblk = (n + uncertainty.BLOCK - 1) // uncertainty.BLOCK
            sizes["partials"] = (nblk * scenes * 3 * 8, torch.float64, (nblk, scenes, 3))
            sizes["scores"] = (scenes * 3 * 8, torch.float64, (scenes, 3))
        for name, (nbytes, dtype, shape) in sizes.items():
            buf = torch.full((BAND + nbytes + BAND,), SENTINEL, dtype=torch.uint8, device=dev)      # BAND keeps the payload 16-byte aligned
            self.bufs[name], self.views[name] = buf, buf[BAND:BAND + nbytes].view(dtype).view(shape)

    def get(self, name):
        return self.views.get(name)

    def bands_intact(self):
        return all(bool((b[:BAND] == SENTINEL).all()) and bool((b[-BAND:] == SENTINEL).all()) for b in self.bufs.values())

    def untouched(self):
        return all(bool((b == SENTINEL).all()) for b in self.bufs.values())


def run(dev, x, w, b, samples, maps, scores):
    from driving_dirty_amd import uncertainty
    scenes, n, k = x.shape[0] // samples, w.shape[0], w.shape[1]
    out = Banded(dev, scenes, n, maps, scores)
    uncertainty.launch("dd_head_uncert", x, w, b, *(out.get(m) for m in uncertainty.MAPS), out.get("partials"), out.get("scores"), scenes, samples, n, k)
    torch.cuda.synchronize()
    assert out.bands_intact(), (scenes, samples, n, k, maps, scores)
    return out


@pytest.mark.parametrize("scenes,samples", cases.GROUPS, ids=[f"{b}x{s}" for b, s in cases.GROUPS])
def test_the_statistics_over_the_grid(dev, scenes, samples):
    from driving_dirty_amd import mc, uncertainty
    used = {"tight": dict.fromkeys(STAT_MAPS + ("scores",), 0.0), "loose": dict.fromkeys(("mean",) + STAT_MAPS + ("scores",), 0.0)}
    reach = 0.0
    for n, k, bias, spread in cases.shapes():
        x, w, b = cases.operands(dev, scenes, samples, n, k, bias, spread)
        where = (scenes, samples, n, k, bias, spread)
        full = run(dev, x, w, b, samples, uncertainty.MAPS, True)
        assert same_bits(full.get("mean"), mc.mean_prob(x, w, b, samples)), where
        z32 = product_logits(x, w, b).cpu().numpy()
        if spread == cases.WIDE:
            reach = max(reach, float(np.abs(z32).max()))
        want, tight = ref.stats_from_logits(z32, samples)
        want64, loose = ref.stats64(*cases.numpy_operands(x, w, b), samples)
        got = {m: full.get(m).cpu().numpy() for m in uncertainty.MAPS + ("scores",)}
        for name in STAT_MAPS + ("scores",):
            f = ref.fraction(got[name], getattr(want, name), getattr(tight, name))
            used["tight"][name] = max(used["tight"][name], f)
            assert f <= 1.0, (where, name, "tight", f)
        for name in ("mean",) + STAT_MAPS + ("scores",):
            f = ref.fraction(got[name], getattr(want64, name), getattr(loose, name))
            used["loose"][name] = max(used["loose"][name], f)
            assert f <= 1.0, (where, name, "loose", f)
        assert got["mi"].min() >= 0 and np.all(got["mi"] <= got["entropy"]) and got["entropy"].max() <= LN2 * (1 + 2.0 ** -22), where
        if samples == 1:
            assert not got["mi"].any() and not got["var"].any() and not got["scores"][:, 1:].any(), where
        # the scores' bits: a second run, no map at all, and each map alone (whose own bits must not move either)
        again = run(dev, x, w, b, samples, uncertainty.MAPS, True)
        alone = run(dev, x, w, b, samples, (), True)
        assert same_bits(again.get("scores"), full.get("scores")) and same_bits(alone.get("scores"), full.get("scores")), where
        assert all(same_bits(again.get(m), full.get(m)) for m in uncertainty.MAPS), where
        for m in uncertainty.MAPS:
            one = run(dev, x, w, b, samples, (m,), True)
            assert same_bits(one.get(m), full.get(m)) and same_bits(one.get("scores"), full.get("scores")), (where, m)
            bare = run(dev, x, w, b, samples, (m,), False)
            assert same_bits(bare.get(m), full.get(m)), (where, m)
    for kind, table in used.items():
        print(f"({scenes},{samples}) largest fraction of the {kind} bounds used: " + ", ".join(f"{k} {v:.3f}" for k, v in table.items()))
    assert reach >= 30.0, "the wide spread carries both tails"


def test_the_tensor_level_function(dev):
    from driving_dirty_amd import mc, uncertainty
    x, w, b = cases.operands(dev, 5, 4, 130, 68)
    got = uncertainty.head_uncertainty(x, w, b, 4)
    assert got._fields == ("mean", "entropy", "mi", "var", "scores") and got.scores.dtype == torch.float64 and tuple(got.scores.shape) == (5, 3)
    assert all(t.dtype == torch.float32 and tuple(t.shape) == (5, 130) for t in got[:4]) and same_bits(got.mean, mc.mean_prob(x, w, b, 4))
    for name, col in zip(uncertainty.SCORES, range(3)):
        assert abs(float(got.scores[0, col]) - float(getattr(got, name)[0].double().mean())) < 1e-12
    some = uncertainty.head_uncertainty(x, w, None, 4, maps=("var", "mi"), scores=False)
    assert some._fields == ("var", "mi") and not same_bits(some.mi, got.mi)      # no bias: other logits
    only = uncertainty.head_uncertainty(x, w, b, 4, maps=())
    assert only._fields == ("scores",) and same_bits(only.scores, got.scores)
    assert same_bits(uncertainty.head_uncertainty(x, w, b, 4, maps="mi", scores=False).mi, got.mi)
    with pytest.raises(uncertainty.HotpathError, match="scene-major"):
        uncertainty.head_uncertainty(x, w, b, 3)      # 20 rows are no multiple of 3


@pytest.mark.parametrize("scenes,samples", [(4, 1), (3, 3), (5, 16)])
def test_saturated_logits_and_a_nan_row(dev, scenes, samples):
    """Columns whose bias puts the logit at +-200 (the exponential flushed to zero): entropy, mutual information and variance finite and
    inside their caps; and one draw of scene 1 all NaN: that scene's maps and scores are NaN, the other scenes' bits are what they are
    without it."""
    from driving_dirty_amd import uncertainty
    n, k = 144, 64
    x, w, b = cases.operands(dev, scenes, samples, n, k, spread=0.5)
    b[::7] = 200.0
    b[3::7] = -200.0
    got = uncertainty.head_uncertainty(x, w, b, samples)
    for name in STAT_MAPS:
        t = getattr(got, name)
        assert bool(torch.isfinite(t).all()) and float(t.min()) >= 0, name
        assert not bool(t[:, ::7].any()) and not bool(t[:, 3::7].any()), name      # every draw exactly 1 or exactly 0: no entropy, no spread
    assert float(got.entropy.max()) <= LN2 * (1 + 2.0 ** -22) and bool((got.mi <= got.entropy).all()) and float(got.var.max()) <= 0.25
    assert bool((got.mean[:, ::7] == 1).all()) and bool((got.mean[:, 3::7] == 0).all()) and bool(torch.isfinite(got.scores).all())
    xn = x.clone()
    xn[1 * samples + samples // 2] = float("nan")
    bad = uncertainty.head_uncertainty(xn, w, b, samples)
    keep = [i for i in range(scenes) if i != 1]
    for name in uncertainty.MAPS + ("scores",):
        assert bool(torch.isnan(getattr(bad, name)[1]).all()), name
        assert same_bits(getattr(bad, name)[keep], getattr(got, name)[keep]), name


def test_refusals_write_nothing(dev):
    from driving_dirty_amd import uncertainty
    scenes, samples, n, k = 3, 4, 144, 64
    x, w, b = cases.operands(dev, scenes, samples, n, k)
    big, wbig = torch.zeros((scenes * samples, 516), device=dev), torch.zeros((n, 516), device=dev)
    out = Banded(dev, scenes, n, uncertainty.MAPS, True)

    def refused(words, **kw):
        a = dict(x=x, w=w, b=b, scenes=scenes, samples=samples, n=n, k=k, **{m: out.get(m) for m in uncertainty.MAPS + ("partials", "scores")})
        a.update(kw)
        with pytest.raises(uncertainty.HotpathError) as e:
            uncertainty.launch("dd_head_uncert", a["x"], a["w"], a["b"], a["mean"], a["entropy"], a["mi"], a["var"], a["partials"], a["scores"],
                               a["scenes"], a["samples"], a["n"], a["k"])
        assert "head_uncert" in str(e.value) and all(word in str(e.value) for word in words), str(e.value)

    refused(("samples", "0"), samples=0)
    refused(("samples", "65"), samples=65)
    refused(("multiple of 4",), k=62)
    refused(("splits K", "516"), x=big, w=wbig, k=516)
    refused(("NULL",), x=None)
    refused(("NULL",), w=None)
    refused(("non-positive",), scenes=0)
    refused(("non-positive",), n=0)
    refused(("too large", "2^31"), scenes=1 << 16, n=1 << 15)
    refused(("partials and scores",), scores=None)
    refused(("partials and scores",), partials=None)
    refused(("no output",), mean=None, entropy=None, mi=None, var=None, partials=None, scores=None)
    refused(("overlaps", "mi", "var"), mi=out.get("var"))
    refused(("overlaps", "entropy", "x"), entropy=x)
    refused(("16-byte",), var=out.get("var").flatten()[1:])
    torch.cuda.synchronize()
    assert out.untouched()
