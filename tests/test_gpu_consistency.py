"""The mirror consistency loss on the device (csrc/consistency.hip: dd_cons_fwd / dd_cons_fwd_grad; consistency.mirror_consistency)
against the fp64 reference of tests/_consistency_ref.py.

Bounds, the project's kernel bounds: a gradient within 2e-5 of its tensor's peak, the loss and every pair's sum within 2e-5 of
themselves, the disagreement counts exact.  The shapes are ``_consistency_ref.SHAPES``: the smallest at which the kernels can still go
wrong, and the road map's once.  Every test prints the worst fraction of a bound it saw.

Observed on an MI355X: at most 0.030 of a bound over the shapes, the edge logits' gradients at 0.014 of theirs."""
import functools

import pytest
import torch

import _consistency_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import consistency
    consistency.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(shape, dev):
    """(a, m) on the device for one shape; built once, never written to."""
    a, m = ref.inputs(shape, salt=shape[0] + shape[2])
    return a.to(dev), m.to(dev)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """(L, stats, dL/da, dL/dm) in fp64 for one shape, computed once on the CPU."""
    return ref.loss_and_grad(*ref.inputs(shape, salt=shape[0] + shape[2]))


def bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def held(got, want, scale=1.0):
    """(loss, stats, da, dm) of the kernels against the reference's -> the worst fraction of a bound.  ``scale``: the gradients' factor."""
    loss, stats, da, dm = got
    w_loss, w_stats, w_da, w_dm = want
    assert loss.dtype == torch.float32 and stats.dtype == torch.float64 and tuple(stats.shape) == (da.shape[0], 2)
    assert torch.equal(stats[:, 1].cpu(), w_stats[:, 1]), "the disagreement counts are exact"
    e_loss = abs(float(loss) - float(w_loss)) / float(w_loss)
    e_q = float(((stats[:, 0].cpu() - w_stats[:, 0]).abs() / w_stats[:, 0]).max())
    e_da, e_dm = ref.peak_error(da, w_da * scale), ref.peak_error(dm, w_dm * scale)
    assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(dm).all())
    assert e_loss <= ref.LOSS_REL and e_q <= ref.LOSS_REL, (e_loss, e_q)
    assert e_da <= ref.GRAD_OF_PEAK and e_dm <= ref.GRAD_OF_PEAK, (e_da, e_dm)
    return max(e_loss / ref.LOSS_REL, e_q / ref.LOSS_REL, e_da / ref.GRAD_OF_PEAK, e_dm / ref.GRAD_OF_PEAK)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_loss_statistics_and_gradients_against_fp64(dev, shape):
    """Also: ``fwd`` and ``fwd_grad`` give the same bits of loss and stats, and a second run gives the bits of the first."""
    from driving_dirty_amd import consistency
    a, m = case(shape, dev)
    got = consistency.fwd_grad(a, m)
    worst = held(got, reference(shape))
    print(f"{shape}: worst fraction of a bound {worst:.3g}")
    loss, stats = consistency.fwd(a, m)
    assert torch.equal(bits(loss), bits(got[0])) and torch.equal(bits(stats), bits(got[1])), "one kernel template: the same bits with and without the gradient"
    again = consistency.fwd_grad(a, m)
    for x, y in zip(got, again):
        assert torch.equal(bits(x), bits(y)), "no atomics: two runs give the same bits"


def test_misaligned_operands_take_the_other_path_and_agree(dev):
    """A vector-shaped case, (2,4,8), whose inputs and outputs start 4 bytes past a 16-byte boundary: the launcher must take the 4-byte
    path.  Both paths give an element to the same lane in the same order, so the results are the aligned call's bit for bit."""
    from driving_dirty_amd import consistency
    shape = (2, 4, 8)
    a, m = case(shape, dev)
    n = a.numel()

    def shifted(src=None):
        buf = torch.full((n + 4,), float("nan"), device=dev)
        view = buf[1:n + 1].view(shape)
        if src is not None:
            view.copy_(src)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return buf, view

    (_, a4), (_, m4), (bda, da4), (bdm, dm4) = shifted(a), shifted(m), shifted(), shifted()
    assert a.data_ptr() % 16 == 0 and m.data_ptr() % 16 == 0
    want = consistency.fwd_grad(a, m)
    got = consistency.fwd_grad(a4, m4, out=(da4, dm4))
    held(got, reference(shape))
    for x, y in zip(got, want):
        assert torch.equal(bits(x), bits(y))
    for buf in (bda, bdm):      # nothing written in front of the payload or behind it
        assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[n + 1:]).all())
    # one misaligned operand is enough
    mixed = consistency.fwd_grad(a, m4)
    for x, y in zip(mixed, want):
        assert torch.equal(bits(x), bits(y))
    loss4, stats4 = consistency.fwd(a4, m)
    assert torch.equal(bits(loss4), bits(want[0])) and torch.equal(bits(stats4), bits(want[1]))


@pytest.mark.parametrize("w", [16, 14], ids=["w16", "w14"])
def test_extreme_logits_give_finite_gradients_within_the_bound(dev, w):
    """Every pair of +-{0, 1e-3, 1, 17, 40, 88, 104}: the gradient goes through p (1 - p) alone."""
    from driving_dirty_amd import consistency
    a, m = ref.edge_inputs(w)
    loss, stats, da, dm = consistency.fwd_grad(a.to(dev), m.to(dev))
    w_loss, w_stats, w_da, w_dm = ref.loss_and_grad(a, m)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(da).all()) and bool(torch.isfinite(dm).all())
    e_da, e_dm = ref.peak_error(da, w_da), ref.peak_error(dm, w_dm)
    print(f"edge logits, w = {w}: gradients at {e_da / ref.GRAD_OF_PEAK:.3g} and {e_dm / ref.GRAD_OF_PEAK:.3g} of the bound")
    assert e_da <= ref.GRAD_OF_PEAK and e_dm <= ref.GRAD_OF_PEAK
    assert torch.equal(stats[:, 1].cpu(), w_stats[:, 1])
    assert abs(float(loss) - float(w_loss)) <= ref.LOSS_REL * float(w_loss)


@pytest.mark.parametrize("shape", [(2, 3, 8), (3, 5, 6), (2, 1, ref.CHUNK + 4)], ids=str)
def test_a_map_and_its_own_reversal_agree_exactly(dev, shape):
    from driving_dirty_amd import consistency
    a, _ = case(shape, dev)
    loss, stats, da, dm = consistency.fwd_grad(a, torch.flip(a, dims=(1,)).contiguous())
    assert float(loss) == 0.0 and bool((stats == 0).all())
    assert bool((da == 0).all()) and bool((dm == 0).all())


@pytest.mark.parametrize("shape", [(2, 3, 8), (3, 5, 6)], ids=str)
def test_grad_scale(dev, shape):
    from driving_dirty_amd import consistency
    a, m = case(shape, dev)
    one = consistency.fwd_grad(a, m, 1.0)
    quarter = consistency.fwd_grad(a, m, 0.25)
    assert torch.equal(bits(one[0]), bits(quarter[0])) and torch.equal(bits(one[1]), bits(quarter[1])), "the loss does not know about grad_scale"
    held(quarter, reference(shape), scale=0.25)
    for q, o in zip(quarter[2:], one[2:]):
        assert ref.peak_error(q, o.double().cpu() * 0.25) <= ref.GRAD_OF_PEAK


def test_autograd_scales_the_gradient_and_refuses_a_slice(dev):
    from driving_dirty_amd import consistency
    shape = (2, 3, 8)
    a, m = case(shape, dev)
    _, _, w_da, w_dm = reference(shape)
    z = torch.cat([a, m]).requires_grad_(True)
    loss, stats = consistency.mirror_consistency(z, return_stats=True)
    assert loss.dim() == 0 and loss.requires_grad and not stats.requires_grad
    (loss * 3).backward()
    assert ref.peak_error(z.grad, torch.cat([w_da, w_dm]) * 3) <= ref.GRAD_OF_PEAK
    plain = consistency.mirror_consistency(z.detach())
    assert not plain.requires_grad and torch.equal(bits(plain), bits(loss))
    wide = torch.zeros((4, 3, 16), device=dev, requires_grad=True)
    with pytest.raises(consistency.HotpathError, match="contiguous"):
        consistency.MirrorConsistency.apply(wide[:, :, ::2])
    with pytest.raises(consistency.HotpathError, match=r"\[2B,h,w\]"):
        consistency.mirror_consistency(torch.zeros((3, 3, 8), device=dev))
    with pytest.raises(consistency.HotpathError, match="fp32"):
        consistency.mirror_consistency(torch.zeros((2, 3, 8), device=dev, dtype=torch.float64))
