"""The BatchNorm2d family without a GPU: the fp64 reference of tests/_bn2d_ref.py against torch.nn.BatchNorm2d(...).double() and
F.max_pool1d, the proof that the bound of tests/test_gpu_bn2d.py tells the two ways of gathering batch statistics apart, and the
exclusion cap on the inputs that file uses."""
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import _bn2d_ref as ref

C = ref.C


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("kind", ["positive", "signs"])
def test_the_chain_against_torch_in_fp64(training, kind):
    b, h, w = 2, 5, 7
    u = ref.inputs((b, h, w), 8)
    gamma, beta = ref.gamma_beta(kind)
    rm0, rv0 = ref.running_stats()
    g_raw = ref.hu((b, h, w, C), "ref_g")
    want = ref.chain(u, gamma, beta, rm0, rv0, g_raw, training)
    bn = nn.BatchNorm2d(C, eps=ref.EPS, momentum=ref.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    bn.train(training)
    x = ref.nchw(u.double()).requires_grad_(True)
    y = F.relu(bn(x))
    y.backward(ref.nchw(g_raw.double()))
    tol = 1e-12
    assert ref.peak_error(ref.nhwc(y), want["y"]) <= tol and ref.peak_error(ref.nhwc(x.grad), want["du"]) <= tol
    assert ref.peak_error(bn.weight.grad, want["dgamma"]) <= tol and ref.peak_error(bn.bias.grad, want["dbeta"]) <= tol
    assert ref.peak_error(bn.running_mean, want["running_mean"]) <= tol and ref.peak_error(bn.running_var, want["running_var"]) <= tol
    mean, var = (u.double().mean((0, 1, 2)), u.double().var((0, 1, 2), unbiased=False)) if training else (rm0.double(), rv0.double())
    assert ref.peak_error(want["save_mean"], mean) <= tol and ref.peak_error(want["save_invstd"], 1 / (var + ref.EPS).sqrt()) <= tol
    sc = gamma.double() / (var + ref.EPS).sqrt()
    assert ref.peak_error(want["affine"], torch.cat([sc, beta.double() - mean * sc] * 2)) <= tol
    assert torch.equal(want["g"], g_raw.double() * (want["y"] > 0))
    if not training:
        assert torch.equal(want["running_mean"], rm0.double()) and torch.equal(want["running_var"], rv0.double())


def test_two_values_give_the_unbiased_factor_two():
    u = ref.inputs((2,), 1)
    rm0, rv0 = ref.running_stats()
    gamma, beta = ref.gamma_beta("positive")
    want = ref.chain(u, gamma, beta, rm0, rv0, torch.zeros(2, C), True)
    a, b = u[0].double(), u[1].double()
    assert ref.peak_error(want["running_var"], 0.9 * rv0.double() + 0.1 * (a - b) ** 2 / 2) <= 1e-12      # biased (a - b)^2 / 4, times 2
    with pytest.raises(ValueError, match="more than 1 value"):      # count = 1 in training mode: torch refuses it, as dd_bn2d_finalize does
        F.batch_norm(torch.zeros(1, C, 1, 1), rm0.clone(), rv0.clone(), gamma, beta, True)


@pytest.mark.parametrize("shape", [(2, 6, 10), (1, 2, 2), (3, 4, 5)])
def test_the_pool_against_max_pool1d(shape):
    """... with gamma of both signs and exactly zero: on a zero-gamma channel with beta > 0 all four taps tie and the first takes the
    gradient, with beta < 0 the window is 0 and nothing flows."""
    b, h, w = shape
    case = ref.pool_case(shape)
    u, aff, gp = case["u"], case["affine"], case["gp"]
    sc, sh = aff[:C].double(), aff[C:2 * C].double()
    z = ref.nchw(u.double() * sc + sh).requires_grad_(True)
    feat = F.relu(z)
    pooled = F.max_pool1d(feat.reshape(b, 1, -1), 4).squeeze(1)
    pooled.backward(gp.double())
    assert torch.equal(case["pooled"], pooled.detach())
    assert torch.equal(case["dfeat"], ref.nhwc(z.grad))
    gamma, beta = ref.gamma_beta("signs")
    d = case["dfeat"].reshape(b, h * w // 4, 4, C)      # [.., window, tap, channel]
    tied = [c for c in range(C) if gamma[c] == 0 and beta[c] > 0]
    dead = [c for c in range(C) if gamma[c] == 0 and beta[c] < 0]
    assert tied and dead and bool((gamma < 0).any()) and bool((gamma > 0).any())
    want_first = gp.double().reshape(b, C, h * w // 4).permute(0, 2, 1)
    assert torch.equal(d[:, :, 0, tied], want_first[:, :, tied]) and bool((d[:, :, 1:, tied] == 0).all())
    assert bool((d[..., dead] == 0).all())


@pytest.mark.parametrize("npix", [1408, 257 * 257])
def test_the_bound_separates_raw_moments_from_merged_moments(npix):
    """A plain-torch model of the two accumulation schemes (tests/_bn2d_ref.py) against the bound of the GPU test: fp32 sums of v and v^2
    per lane break it at |mean| / sigma = 512 (at 1408 pixels; at 66049 the roundings of two trips and more lanes average further and the
    model only comes close, so nothing is claimed there), moments about a pivot, merged by Chan's formula, hold it at every ratio."""
    for ratio in ref.RATIOS + (4096,):
        case = ref.chain_case(npix, ratio, True)
        want, e_ref = case["want"], case["e_ref"]
        figures = {}
        for name, model in (("raw", ref.model_raw_moments), ("merged", ref.model_merged_moments)):
            mean, invstd = model(case["u"])
            figures[name] = (ref.peak_error(mean, want["save_mean"]), ref.peak_error(invstd, want["save_invstd"]))
        b_mean, b_inv = ref.bound("save_mean", e_ref["save_mean"]), ref.bound("save_invstd", e_ref["save_invstd"])
        print(f"npix {npix} ratio {ratio}: invstd raw {figures['raw'][1]:.2e} merged {figures['merged'][1]:.2e} E_ref {e_ref['save_invstd']:.2e} "
              f"bound {b_inv:.2e}; mean raw {figures['raw'][0]:.2e} merged {figures['merged'][0]:.2e} bound {b_mean:.2e}")
        assert figures["merged"][0] <= b_mean and figures["merged"][1] <= b_inv, (ratio, figures)
        if ratio >= 512 and npix == 1408:
            assert figures["raw"][1] > b_inv, (ratio, figures)


def test_the_inputs_have_their_offsets():
    u = ref.inputs((4096,), 64).double()
    mean, var = ref.batch_stats(u)
    r = mean / var.sqrt()
    assert abs(float(r[ref.ZERO_MEAN_CHANNEL])) < 0.1
    others = [c for c in range(C) if c != ref.ZERO_MEAN_CHANNEL]
    assert all(abs(abs(float(r[c])) - 64) < 3.2 for c in others)      # the sample's own spread is within 5 % of sigma_c
    assert all((float(r[c]) > 0) == (c % 2 == 0) for c in others)
    assert len({round(float(m), 4) for m in mean}) == C, "every channel its own mean"
    assert 257 * 257 > ref.GRID_CAP_PIXELS and (257 * 257) % 2 == 1 and 256 * 258 > ref.GRID_CAP_PIXELS
    b, h, w = ref.POOL_SHAPES[-1]
    assert b * h * w * 2 > 8 * ref.GRID_CAP_PIXELS and (h * w) % 4 == 0      # dd_pool4_bn_*: B * (H W / 4) * 8 items


def test_the_exclusion_cap_on_the_reference_alone():
    """Every tensor whose comparison leaves undecided elements out leaves out at most FLIP_CAP of them."""
    for shape in ref.POOL_SHAPES:
        frac = float(ref.pool_case(shape)["skip"].double().mean())
        print(f"pool {shape}: {frac:.2e} of dfeat left out")
        assert frac <= ref.FLIP_CAP
    for stride in (1, 2):
        frac = float(ref.sign_layer(stride)["skip"].double().mean())
        print(f"dgrad_bn stride {stride}: {frac:.2e} of dx left out")
        assert frac <= ref.FLIP_CAP
    # the stand-alone chain hands the kernels an already-masked gradient: nothing is left out there, and y is compared everywhere
    for npix in ref.CHAIN_PIXELS[2:]:
        for ratio in ref.RATIOS:
            case = ref.chain_case(npix, ratio, True)
            frac = float(ref.undecided(case["u"], case["want"]["affine"][:C], case["want"]["affine"][C:2 * C]).double().mean())
            assert frac <= ref.FLIP_CAP, (npix, ratio, frac)
