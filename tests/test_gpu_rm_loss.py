"""The road-map loss on the device (csrc/rm_loss.hip: dd_rm_loss_fwd / _bwd and their _u8_ptrs forms; rm_loss.road_map_loss) against the
fp64 reference of tests/_rm_loss_ref.py.

Bounds.  T is exact.  S, I, A, C and the three losses: the bounds ``_rm_loss_ref`` DERIVES from the element function's bounds
(tests/_element_ref.py) and the fp32 accumulation of CHUNK / 256 terms per thread -- tests/test_rm_loss_ref.py shows, without a GPU, that
an fp32 model of the kernels meets them.  A gradient: 2e-5 of THAT SAMPLE's peak |dL/dz|, the box-loss test's figure (the automatic
weights differ by orders of magnitude between samples); exact zeros where the reference is identically zero.  Every test prints the
worst fraction of a bound it saw.

Observed on an MI355X: statistics at most 0.048 of their bounds, losses 0.025, gradients 0.025 of the 2e-5."""
import functools

import numpy as np
import pytest
import torch

import _element_ref as E
import _rm_loss_ref as ref

pytestmark = pytest.mark.gpu

POS_WEIGHTS = [None, 2.5, "auto"]
MIXES = [(1.0, 0.0), (0.0, 1.0), (0.7, 1.3)]
EPSILONS = [1.0, 0.0]
SHAPES = ref.SHAPES


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import rm_loss
    rm_loss.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(shape, dev):
    """(z, t fp32 0 / 1) on the device for one of SHAPES; built once, never written to."""
    z, t = ref.case(shape)
    return z.to(dev), t.to(dev)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """fp64 pieces of every setting for one shape, computed once on the CPU: {("bce", pos_weight): (L_bce, dL_bce/dz), ("ts", eps): (L_ts,
    dL_ts/dz), "stats": [B, 5], "bounds": [B, 5]}.  The loss is linear in them: L = alpha L_bce + beta L_ts."""
    z, t = ref.case(shape)
    out = {"stats": ref.stats(z, t).numpy(), "bounds": ref.stat_bounds(z, t)}
    for w in POS_WEIGHTS:
        _, l_bce, _, g = ref.loss_and_grad(z, t, w, 1.0, 0.0)
        out["bce", w] = (l_bce, g)
    for eps in EPSILONS:
        _, _, l_ts, g = ref.loss_and_grad(z, t, None, 0.0, 1.0, eps)
        out["ts", eps] = (l_ts, g)
    return out


def forms(t):
    """The forms a 0 / 1 target comes in: fp32, uint8, bool and the collate's tuple of per-sample masks."""
    return {"f32": t, "u8": t.to(torch.uint8), "bool": t.bool(), "tuple": tuple(t.bool().unbind(0))}


# ------------------------------------------------------------------------------------------------ every setting on every shape
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_loss_gradient_and_statistics_against_fp64(dev, shape):
    from driving_dirty_amd import rm_loss
    z, t = case(shape, dev)
    zc, tc = ref.case(shape)
    pieces = reference(shape)
    want_stats, bounds = pieces["stats"], pieces["bounds"]
    assert bool((want_stats[:, 1] + want_stats[:, 0] - want_stats[:, 2] > 0).all())      # U_b > 0: eps = 0 is defined on every sample
    worst = {"stats": 0.0, "loss": 0.0, "grad": 0.0}
    for w in POS_WEIGHTS:
        for alpha, beta in MIXES:
            for eps in EPSILONS:
                (l_bce, g_bce), (l_ts, g_ts) = pieces["bce", w], pieces["ts", eps]
                a32, b32 = ref.abi(alpha), ref.abi(beta)
                losses, stats, coef, probs = rm_loss.fwd(z, t, w, alpha, beta, eps)
                grad = rm_loss.bwd(probs, t, coef)
                what = (shape, w, alpha, beta, eps)
                got_stats = stats.cpu().numpy()
                assert np.array_equal(got_stats[:, 0], want_stats[:, 0]), (what, "T is exact")
                frac = float(E.error_fraction(np.abs(got_stats - want_stats)[:, 1:], bounds[:, 1:]).max())
                worst["stats"] = max(worst["stats"], frac)
                assert frac <= 1.0, (what, got_stats, want_stats, bounds)
                want = (a32 * l_bce + b32 * l_ts, l_bce, l_ts)
                for got, r, bd in zip(losses.tolist(), want, ref.loss_bounds(zc, tc, w, alpha, beta, eps, want_stats, bounds)):
                    frac = float(E.error_fraction(abs(got - float(r)), bd))
                    worst["loss"] = max(worst["loss"], frac)
                    assert frac <= 1.0, (what, got, float(r), bd)
                excess = ref.grad_excess(grad, a32 * g_bce + b32 * g_ts)
                worst["grad"] = max(worst["grad"], excess / ref.GRAD_OF_PEAK)
                assert excess <= ref.GRAD_OF_PEAK, (what, excess)
    print(f"rm_loss {shape}: worst fraction of its bound -- statistics {worst['stats']:.3f}, losses {worst['loss']:.3f}, "
          f"gradient {worst['grad']:.3f} (of {ref.GRAD_OF_PEAK} of the sample's peak)")


# ------------------------------------------------------------------------------------------------ the probabilities
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_probs_are_the_bits_of_ops_sigmoid(dev, shape):
    from driving_dirty_amd import ops, rm_loss
    z, t = case(shape, dev)
    want = ops.sigmoid(z)
    for name, target in forms(t).items():
        assert torch.equal(rm_loss.fwd(z, target, "auto", 0.7, 1.3)[3], want), name
    assert rm_loss.fwd(z, t, want_probs=False)[3] is None
    assert all(torch.equal(a, b) for a, b in zip(rm_loss.fwd(z, t, want_probs=False)[:3], rm_loss.fwd(z, t)[:3]))


# ------------------------------------------------------------------------------------------------ the forms of the target
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_form_of_the_target_gives_the_same_bits(dev, shape):
    """uint8, bool, fp32 0 / 1 and the tuple of per-sample masks: the pointer table up to 64 samples, stacked past it."""
    from driving_dirty_amd import rm_loss
    z, t = case(shape, dev)
    losses, stats, coef, probs = rm_loss.fwd(z, t, "auto", 0.7, 1.3)
    grad = rm_loss.bwd(probs, t, coef, 1.5)
    assert (shape[0] > rm_loss.TABLE_MAX) == (shape == (65, 260))
    for name, target in forms(t).items():
        l2, s2, c2, p2 = rm_loss.fwd(z, target, "auto", 0.7, 1.3)
        assert torch.equal(l2, losses) and torch.equal(s2, stats) and torch.equal(c2, coef) and torch.equal(p2, probs), name
        assert torch.equal(rm_loss.bwd(p2, target, c2, 1.5), grad), name


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("shape", [(65, 260), (2, 640000)], ids=str)
def test_two_launches_are_bit_identical(dev, shape):
    from driving_dirty_amd import rm_loss
    z, t = case(shape, dev)
    for target in (t, tuple(t.bool().unbind(0))):
        first, second = rm_loss.fwd(z, target, "auto", 1.0, 1.0), rm_loss.fwd(z, target, "auto", 1.0, 1.0)
        assert all(torch.equal(a, b) for a, b in zip(first, second))
        assert torch.equal(rm_loss.bwd(first[3], target, first[2]), rm_loss.bwd(second[3], target, second[2]))


# ------------------------------------------------------------------------------------------------ the edges of the element function
def test_edge_logits_give_a_finite_loss_and_gradient(dev):
    from driving_dirty_amd import rm_loss
    zc, tc = ref.edge_inputs()
    z, t = zc.to(dev), tc.to(dev)
    assert float(zc.abs().max()) > 87.0
    want_stats, bounds = ref.stats(zc, tc).numpy(), ref.stat_bounds(zc, tc)
    for w, alpha, beta, eps in ((None, 1.0, 0.0, 1.0), ("auto", 0.7, 1.3, 1.0), (2.5, 0.0, 1.0, 0.0)):
        losses, stats, coef, probs = rm_loss.fwd(z, t.bool(), w, alpha, beta, eps)
        grad = rm_loss.bwd(probs, t.bool(), coef)
        for name, x in (("loss", losses), ("stats", stats), ("coef", coef), ("probs", probs), ("gradient", grad)):
            assert bool(torch.isfinite(x).all()), (w, alpha, beta, eps, name)
        frac = float(E.error_fraction(np.abs(stats.cpu().numpy() - want_stats)[:, 1:], bounds[:, 1:]).max())
        assert frac <= 1.0, (w, frac)
        want = ref.loss_and_grad(zc, tc, w, alpha, beta, eps)
        for got, r, bd in zip(losses.tolist(), want[:3], ref.loss_bounds(zc, tc, w, alpha, beta, eps, want_stats, bounds)):
            assert abs(got - float(r)) <= bd, (w, got, float(r), bd)
        print(f"rm_loss edge logits {(w, alpha, beta, eps)}: statistics use {frac:.3f} of their bounds, the gradient "
              f"{ref.grad_excess(grad, want[3]) / ref.GRAD_OF_PEAK:.3f} of {ref.GRAD_OF_PEAK} of the sample's peak")
        assert ref.grad_excess(grad, want[3]) <= ref.GRAD_OF_PEAK


# ------------------------------------------------------------------------------------------------ the scale of the gradient
def test_grad_scale_and_an_upstream_gradient_scale_the_gradient(dev):
    from driving_dirty_amd import rm_loss
    shape = (3, ref.CHUNK + 4)
    z, t = case(shape, dev)
    zc, tc = ref.case(shape)
    kw = dict(pos_weight="auto", bce_weight=0.7, ts_weight=1.3)
    _, _, _, g = ref.loss_and_grad(zc, tc, "auto", 0.7, 1.3)
    _, _, coef, probs = rm_loss.fwd(z, t, **kw)
    one, scaled = rm_loss.bwd(probs, t, coef), rm_loss.bwd(probs, t, coef, 2.5)
    assert ref.grad_excess(one, g) <= ref.GRAD_OF_PEAK and ref.grad_excess(scaled, 2.5 * g) <= ref.GRAD_OF_PEAK
    assert float((scaled - 2.5 * one).abs().max()) <= 2.0 ** -21 * float(scaled.abs().max())      # the coefficients are rounded once more
    assert torch.equal(rm_loss.bwd(probs, t, coef, 0.0), torch.zeros_like(one))
    za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    loss, _ = rm_loss.road_map_loss(za, t, **kw)
    loss.backward()
    (2.5 * rm_loss.road_map_loss(zb, tuple(t.bool().unbind(0)), **kw)[0]).backward()
    assert torch.equal(za.grad, one)
    assert ref.grad_excess(zb.grad, 2.5 * g) <= ref.GRAD_OF_PEAK
    assert float((zb.grad - 2.5 * za.grad).abs().max()) <= 2.0 ** -22 * float(zb.grad.abs().max())      # one more fp32 rounding per element


# ------------------------------------------------------------------------------------------------ the existing kernel
@pytest.mark.parametrize("shape", [(3, ref.CHUNK + 4), (2, 640000)], ids=str)
def test_the_defaults_are_bce_with_logits_probs(dev, shape):
    from driving_dirty_amd import ops, rm_loss
    z, t = case(shape, dev)
    zc, tc = ref.case(shape)
    want, _, _, g = ref.loss_and_grad(zc, tc)
    bound = ref.loss_bounds(zc, tc, None, 1.0, 0.0, 1.0)[0]
    for target in (t, t.bool(), tuple(t.bool().unbind(0))):
        za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
        old, old_probs = ops.BceWithLogitsProbs.apply(za, target)
        new, new_probs = rm_loss.road_map_loss(zb, target)
        old.backward()
        new.backward()
        assert torch.equal(new_probs, old_probs)
        e_new, e_old = abs(float(new.detach()) - float(want)), abs(float(old.detach()) - float(want))
        print(f"rm_loss {shape} at the defaults: |new - fp64| {e_new / bound:.3f}, |BceWithLogitsProbs - fp64| {e_old / bound:.3f} of the bound")
        assert e_new <= bound and e_old <= bound
        assert ref.grad_excess(zb.grad, g) <= ref.GRAD_OF_PEAK and ref.grad_excess(za.grad, g) <= ref.GRAD_OF_PEAK
        assert ref.grad_excess(zb.grad, za.grad) <= ref.GRAD_OF_PEAK


# ------------------------------------------------------------------------------------------------ a sample does not see the batch
def test_a_batch_is_the_mean_of_its_samples(dev):
    from driving_dirty_amd import rm_loss
    z, t = case((3, ref.CHUNK + 4), dev)
    whole = rm_loss.fwd(z, t, "auto", 1.0, 1.0)
    singles = [rm_loss.fwd(z[i:i + 1].contiguous(), t[i:i + 1].contiguous(), "auto", 1.0, 1.0) for i in range(3)]
    for k in range(3):
        mean = sum(float(s[0][k]) for s in singles) / 3
        assert abs(float(whole[0][k]) - mean) <= 2.0 ** -22 * abs(mean), k      # four fp32 roundings of the same fp64 sums
    assert torch.equal(whole[1], torch.cat([s[1] for s in singles]))      # the statistics of a sample: the same bits alone and in the batch
    assert torch.equal(whole[3], torch.cat([s[3] for s in singles]))


# ------------------------------------------------------------------------------------------------ autograd
def test_autograd_surface(dev):
    from driving_dirty_amd import rm_loss
    z, t = case((3, ref.CHUNK + 4), dev)
    kw = dict(pos_weight="auto", bce_weight=0.7, ts_weight=1.3)
    za = z.clone().requires_grad_(True)
    loss, probs = rm_loss.road_map_loss(za, t, **kw)
    assert loss.dim() == 0 and loss.requires_grad and not probs.requires_grad and probs.shape == z.shape
    total, probs2, bce, ts, stats = rm_loss.road_map_loss(za, t, return_parts=True, **kw)
    assert torch.equal(total, loss.detach()) and torch.equal(probs2, probs)
    assert not bce.requires_grad and not ts.requires_grad and not stats.requires_grad and bce.dim() == ts.dim() == 0
    assert stats.shape == (3, 5) and stats.dtype == torch.float64
    assert abs(float(total.detach()) - (ref.abi(0.7) * float(bce) + ref.abi(1.3) * float(ts))) <= 2.0 ** -22 * float(total.detach())
    (loss + probs.sum() * 0).backward()      # the probabilities' gradient slot stays empty
    assert za.grad is not None and bool(torch.isfinite(za.grad).all())
    with torch.no_grad():
        quiet, _ = rm_loss.road_map_loss(za, t, **kw)
    assert torch.equal(quiet, loss.detach()) and not quiet.requires_grad
    assert torch.equal(rm_loss.road_map_loss(z, t.bool(), **kw)[0], quiet)      # no gradient asked for: the forward alone


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_entry_point(dev):
    from driving_dirty_amd import _lib, rm_loss
    z, t = case((3, ref.CHUNK + 4), dev)
    with pytest.raises(_lib.HotpathError, match="dd_rm_loss_fwd.*multiple of 4"):
        rm_loss.road_map_loss(torch.zeros(2, 6, device=dev), torch.zeros(2, 6, device=dev))
    with pytest.raises(_lib.HotpathError, match="dd_rm_loss_fwd.*pos_weight"):
        rm_loss.road_map_loss(z, t, pos_weight=0)
    with pytest.raises(_lib.HotpathError, match="dd_rm_loss_fwd_u8_ptrs.*ts_eps"):
        rm_loss.road_map_loss(z, tuple(t.bool().unbind(0)), ts_eps=-1.0)
    with pytest.raises(_lib.HotpathError, match="logits must be fp32, got torch.float64"):
        rm_loss.road_map_loss(z.double(), t)
    with pytest.raises(_lib.HotpathError, match="target"):
        rm_loss.road_map_loss(z, t[:, :1024].contiguous())
    with pytest.raises(_lib.HotpathError, match="target"):
        rm_loss.road_map_loss(z, t.double())
    with pytest.raises(_lib.HotpathError, match="masks"):
        rm_loss.road_map_loss(z, tuple(t.bool().unbind(0))[:2])
