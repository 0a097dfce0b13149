"""The road-map loss without a GPU: the fp64 reference of tests/_rm_loss_ref.py holds together (autograd against the header's closed
form, the plain setting against torch's BCE-with-logits), and THE BOUNDS CAN BE MET -- an fp32 numpy model of the kernels' element
function and of their summation stays inside the derived bounds on every input the GPU test uses.  Nothing here runs a kernel."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _element_ref as E
import _rm_loss_ref as ref

POS_WEIGHTS = [None, 2.5, "auto"]
MIXES = [(1.0, 0.0), (0.0, 1.0), (0.7, 1.3)]
EPSILONS = [1.0, 0.0]
SMALL = [(1, 4), (3, 1028), (5, 260)]


def small_case(shape):
    b, per = shape
    return ref.inputs(b, per, salt=7 + b, empty=(1,) if b >= 3 else (), full=(2,) if b >= 3 else ())


@pytest.mark.parametrize("shape", SMALL)
def test_autograd_and_the_closed_form_agree(shape):
    z, t = small_case(shape)
    for w in POS_WEIGHTS:
        for alpha, beta in MIXES:
            for eps in EPSILONS:
                _, _, _, g = ref.loss_and_grad(z, t, w, alpha, beta, eps)
                c = ref.closed_form_grad(z, t, w, alpha, beta, eps)
                peak = float(g.abs().max())
                assert float((g - c).abs().max()) <= 1e-12 * peak, (shape, w, alpha, beta, eps)
    ze, te = ref.edge_inputs()
    _, _, _, g = ref.loss_and_grad(ze, te, "auto", 0.7, 1.3, 1.0)
    c = ref.closed_form_grad(ze, te, "auto", 0.7, 1.3, 1.0)
    assert bool(torch.isfinite(g).all()) and float((g - c).abs().max()) <= 1e-12 * float(g.abs().max())


@pytest.mark.parametrize("shape", SMALL)
def test_the_plain_setting_is_torchs_bce_with_logits(shape):
    z, t = small_case(shape)
    total, l_bce, _, g = ref.loss_and_grad(z, t, None, 1.0, 0.0)
    zd = z.double().requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(zd, t.double())
    (gw,) = torch.autograd.grad(want, zd)
    want = want.detach()
    assert abs(float(total) - float(want)) <= 1e-14 * float(want) and torch.equal(total, l_bce)
    assert float((g - gw).abs().max()) <= 1e-14 * float(gw.abs().max())
    # ... and a numeric pos_weight is torch's
    _, l_w, _, _ = ref.loss_and_grad(z, t, 2.5, 1.0, 0.0)
    want_w = F.binary_cross_entropy_with_logits(z.double(), t.double(), pos_weight=torch.tensor(2.5, dtype=torch.float64))
    assert abs(float(l_w) - float(want_w)) <= 1e-14 * float(want_w)
    # the statistics are the loss's parts
    st = ref.stats(z, t)
    b, per = shape
    assert abs(float((st[:, 3] + st[:, 4]).sum() / (b * per)) - float(want)) <= 1e-14 * float(want)


def test_the_constants_of_the_split():
    assert ref.CHUNK % 1024 == 0 and ref.ACC == ref.CHUNK // 256 and ref.ACC % 4 == 0
    assert ref.SHAPES == [(1, 4), (3, ref.CHUNK + 4), (65, 260), (2, 640000)]
    z, t = ref.edge_inputs()
    assert z.shape[1] % 4 == 0 and float(z.abs().max()) > 87.0 and torch.equal(t[0], 1 - t[1])
    assert {60.0, -60.0} <= set(z[0].tolist()) and set(E.logit_edges().tolist()) <= set(z[0].tolist())


@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_an_fp32_model_of_the_kernels_stays_inside_the_bounds(shape):
    """Before any GPU run: the header's operation sequence in numpy float32 (correctly rounded primitives) and the kernels' order of
    summation, against the fp64 reference, on the inputs of tests/test_gpu_rm_loss.py."""
    z, t = ref.case(shape)
    want, bound = ref.stats(z, t).numpy(), ref.stat_bounds(z, t)
    got = ref.model_stats(z.numpy(), t.numpy())
    assert np.array_equal(got[:, 0], want[:, 0]), "T is exact"
    frac = E.error_fraction(np.abs(got - want)[:, 1:], bound[:, 1:])
    print(f"rm_loss model {shape}: statistics use at most {frac.max():.3f} of their bounds (S, I, A, C: {frac.max(axis=0)})")
    assert frac.max() <= 1.0, (shape, frac)
    b, per = shape
    T, S, I, A, C = got.T
    worst = 0.0
    for w in POS_WEIGHTS:
        wb = ref.weights(t.double(), w).numpy()[:, 0]
        for alpha, beta in MIXES:
            for eps in EPSILONS:
                if eps == 0.0 and not bool((want[:, 1] + want[:, 0] - want[:, 2] > 0).all()):
                    continue
                a32, b32, e32 = ref.abi(alpha), ref.abi(beta), ref.abi(eps)
                l_bce = (wb * A + C).sum() / (b * per)
                l_ts = ref.soft_ts(I, S, T, e32).sum() / b
                model = [np.float32(a32 * l_bce + b32 * l_ts), np.float32(l_bce), np.float32(l_ts)]
                ref_l = ref.loss_and_grad(z, t, w, alpha, beta, eps)[:3]
                for m, r, bd in zip(model, ref_l, ref.loss_bounds(z, t, w, alpha, beta, eps)):
                    f = float(E.error_fraction(abs(float(m) - float(r)), bd))
                    worst = max(worst, f)
                    assert f <= 1.0, (shape, w, alpha, beta, eps, float(m), float(r), bd)
    print(f"rm_loss model {shape}: losses use at most {worst:.3f} of their bounds")


def test_the_model_on_the_edge_logits_is_finite_and_inside_the_bounds():
    z, t = ref.edge_inputs()
    want, bound = ref.stats(z, t).numpy(), ref.stat_bounds(z, t)
    got = ref.model_stats(z.numpy(), t.numpy())
    assert np.isfinite(got).all() and np.array_equal(got[:, 0], want[:, 0])
    frac = E.error_fraction(np.abs(got - want)[:, 1:], bound[:, 1:])
    print(f"rm_loss model, edge logits: statistics use at most {frac.max():.3f} of their bounds")
    assert frac.max() <= 1.0, frac
    five, sig = ref.model_terms(z.numpy(), t.numpy())
    # the gradient's factors from the probabilities alone: finite at every edge, and p (1 - p) is 0, not NaN, where p rounds to 0 or 1
    q = np.float32(1) - sig
    assert np.isfinite(sig * q).all() and np.isfinite(five).all()


def test_the_gradient_bound_is_the_box_losss():
    import test_gpu_box_loss as box
    assert ref.GRAD_OF_PEAK == box.GRAD_OF_PEAK == 2e-5 and ref.MODEL_GRAD_OF_PEAK == box.MODEL_GRAD_OF_PEAK == 2e-4
