"""The BatchNorm2d kernels of the Conv -> BatchNorm2d -> ReLU variant against fp64 (tests/_bn2d_ref.py): csrc/bn2d.hip (dd_bn2d_stats,
_finalize, _apply_relu, _bwd, dd_pool4_bn_fwd / _bwd), the statistics epilogue of dd_conv_fwd_stats, and the mask / input transforms of
dd_conv_dgrad_bn / dd_conv_wgrad_bn -- where the guard-band cases (inputs with mean ~ 0, gamma > 0, at most 1408 pixels) do not look:

  * offsets: channels with |mean| / sigma up to 512, every channel its own mean with alternating sign, one channel at 0;
  * full grids: 257 x 257 pixels, the smallest odd count at which lanes of the grid-stride kernels make a second trip (and a pooling
    shape past ITS cap); the conv epilogue at one compute unit, where a lane gathers over several rows and column segments;
  * gamma of both signs and exactly zero.

The bound, everywhere: error relative to the reference tensor's peak <= max(B, 4 E_ref), B the guard cases' bound for that output, E_ref
the error of torch's own fp32 batch norm on the same inputs (tests/_bn2d_ref.py states why).  Outputs of the conv kernels proper (u, dx,
dw, dbias) and of the pool are held to B = KERNEL_TOL alone.  Every test prints error, E_ref and bound before it asserts (pytest -s).

Observed on an MI355X (error relative to the peak; worst case of each group, E_ref and the bound beside it; 59 tests in 4.3 s):
  chain, ratio 0..8     every output <= 3.0e-6 (du at ratio 1: 3.0e-6, E_ref 3.1e-6, bound 2e-4); y <= 3.0e-7 (E_ref 2.4e-7, bound 2e-5)
  chain, ratio 64       save_invstd 5.2e-8 (E_ref 6.5e-8, 2e-5)   y 2.5e-6 (E_ref 2.5e-6, 2e-5)    dgamma 1.7e-6 (E_ref 1.8e-6, 2e-4)
  chain, ratio 512      save_invstd 5.2e-8 (E_ref 6.5e-8, 2e-5)   y 2.0e-5 (E_ref 1.9e-5, 7.4e-5)  dgamma 2.5e-5 (E_ref 2.5e-5, 2e-4)
                        du 7.8e-7 (E_ref 7.8e-7, 2e-4)            affine 9.8e-8 (E_ref 1.6e-7, 2e-5)   running_var 8.9e-8 (E_ref 8.9e-8, 2e-5)
  conv epilogue         save_invstd 2.9e-7 / 2.9e-7 / 3.2e-7 / 1.2e-7 at ratio 0 / 8 / 64 / 512 (E_ref 6e-8..7e-8, 2e-5); save_mean <= 7.4e-8; u <= 5.1e-7
  gamma signs           chain: y 9.6e-8, du 1.4e-7; pool: pooled 4.1e-8, dfeat exact (3.8e-6 of (1, 258, 256) left out, 4.8e-7 of (1, 513, 512), none
                        of (2, 6, 10)); conv readers: u 4.6e-7, dx 7.1e-7 (nothing left out), dw 1.1e-7, dbias 8.3e-8 (all against 2e-5)
  count 2               running_var 6.9e-8 (2e-5)
With raw fp32 sums of v and v^2 in the statistics table (what the kernels gathered before they kept a pivot) the same run failed 15 of these
tests: ratios 0, 1, 8 within the bound everywhere; ratio 64: save_invstd 5.3e-5 for the chain at 1408 pixels (within the bound at 66049) and
5.8e-5 .. 4.0e-4 for every conv case; ratio 512: 1.9e-3 (1408 pixels) and 3.6e-4 (66049) for the chain, with y, du, dgamma, affine and
running_var past their bounds behind it, and 3.9e-3 .. 2.2e-2 for every conv case, the largest at one compute unit.
"""
import math

import pytest
import torch

from driving_dirty_amd import _lib

import _bn2d_ref as ref
from test_gpu_wave_ranges import cu_budget

pytestmark = pytest.mark.gpu

C = ref.C
f32 = torch.float32
PACK_FWD, PACK_DGRAD_S1, PACK_DGRAD_S2 = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.lib()
    return torch.device("cuda:0")


def stats_table(dev):
    """dd_conv_stats_floats() floats of NaN: every row the finalize kernel reads must have been written by the producer."""
    return torch.full((_lib.size("dd_conv_stats_floats"),), math.nan, device=dev, dtype=f32)


def finalize(dev, stats, count, gamma, beta, rm0, rv0, training):
    """-> (affine, save_mean, save_invstd, running_mean, running_var) on the device."""
    rm, rv = rm0.to(dev).clone(), rv0.to(dev).clone()
    aff, sm, si = (torch.empty(n, device=dev, dtype=f32) for n in (128, C, C))
    _lib.call("dd_bn2d_finalize", stats, count, gamma.to(dev), beta.to(dev), rm, rv, ref.MOMENTUM, ref.EPS, int(training), aff, sm, si)
    return aff, sm, si, rm, rv


def run_chain(dev, case, training):
    """dd_bn2d_stats -> dd_bn2d_finalize -> dd_bn2d_apply_relu -> dd_bn2d_bwd on the inputs of ref.chain_case: its outputs by name, on the CPU."""
    u, g, gamma = case["u"].to(dev), case["g"].to(dev), case["gamma"].to(dev)
    npix = u.shape[0]
    stats = None
    if training:
        stats = stats_table(dev)
        _lib.call("dd_bn2d_stats", u, stats, npix)
    aff, sm, si, rm, rv = finalize(dev, stats, npix, case["gamma"], case["beta"], case["rm0"], case["rv0"], training)
    y = torch.empty_like(u)
    _lib.call("dd_bn2d_apply_relu", u, aff, y, npix)
    du, dg, db = torch.empty_like(u), torch.empty(C, device=dev, dtype=f32), torch.empty(C, device=dev, dtype=f32)
    ws = torch.empty(_lib.size("dd_bn2d_workspace_bytes"), device=dev, dtype=torch.uint8)
    _lib.call("dd_bn2d_bwd", g, u, gamma, sm, si, du, dg, db, npix, int(training), ws)
    torch.cuda.synchronize()
    if training:
        assert bool(torch.isfinite(stats).all()), "dd_bn2d_stats must leave every row of the table defined"
    out = {"save_mean": sm, "save_invstd": si, "affine": aff, "running_mean": rm, "running_var": rv, "y": y, "du": du, "dgamma": dg, "dbeta": db}
    return {k: v.cpu() for k, v in out.items()}


def judge(label, got, want, e_ref, names=None):
    """Print error, E_ref and bound of every output; return the ones past their bound."""
    bad = []
    for name in names or ref.OUTPUT_BOUNDS:
        err, bound = ref.peak_error(got[name], want[name]), ref.bound(name, e_ref[name])
        print(f"{label} {name}: error {err:.2e}  E_ref {e_ref[name]:.2e}  bound {bound:.2e}" + ("" if err <= bound else "  <-- PAST THE BOUND"))
        if not err <= bound:
            bad.append((name, err, bound))
    return bad


# ------------------------------------------------------------------------------------------------ the stand-alone chain
CHAIN_CASES = [(n, 1) for n in ref.CHAIN_PIXELS[:2]] + [(n, r) for n in ref.CHAIN_PIXELS[2:] for r in ref.RATIOS]


@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
@pytest.mark.parametrize("npix,ratio", CHAIN_CASES)
def test_chain_against_fp64(dev, npix, ratio, training):
    case = ref.chain_case(npix, ratio, training)
    got = run_chain(dev, case, training)
    bad = judge(f"chain npix {npix} ratio {ratio} {'training' if training else 'eval'}", got, case["want"], case["e_ref"])
    assert not bad, bad
    if not training:
        assert torch.equal(got["running_mean"], case["rm0"]) and torch.equal(got["running_var"], case["rv0"])


def test_chain_with_gamma_of_both_signs_and_zero(dev):
    """dd_bn2d_apply_relu (and the rest of the chain) at ratio 1 with negative, exactly zero and positive gamma: a kernel that selected on u
    and applied the affine afterwards, or assumed sc > 0, fails on y; on the zero channels y = relu(beta) everywhere and du = 0."""
    case = ref.chain_case(1408, 1, True, "signs")
    got = run_chain(dev, case, True)
    bad = judge("chain gamma signs", got, case["want"], case["e_ref"])
    assert not bad, bad
    zero = case["gamma"] == 0
    assert bool(zero.any()) and bool((case["gamma"] < 0).any())
    assert torch.equal(got["y"][:, zero], torch.relu(case["beta"][zero]).expand(1408, -1)) and bool((got["du"][:, zero] == 0).all())


@pytest.mark.parametrize("npix,ratio", [(1408, 64), (257 * 257, 64)])
def test_two_runs_give_the_same_bits(dev, npix, ratio):
    case = ref.chain_case(npix, ratio, True)
    first, second = run_chain(dev, case, True), run_chain(dev, case, True)
    for name in first:
        assert torch.equal(first[name].view(torch.int32), second[name].view(torch.int32)), name


# ------------------------------------------------------------------------------------------------ count edges
def test_two_values_give_the_unbiased_factor_two(dev):
    case = ref.chain_case(2, 1, True)
    got = run_chain(dev, case, True)
    a, b = case["u"][0].double(), case["u"][1].double()
    want = (1 - ref.MOMENTUM) * case["rv0"].double() + ref.MOMENTUM * (a - b) ** 2 / 2      # the biased variance (a - b)^2 / 4, times 2 / (2 - 1)
    err = ref.peak_error(got["running_var"], want)
    print(f"count 2: running_var error {err:.2e}  bound {ref.KERNEL_TOL:.2e}")
    assert err <= ref.KERNEL_TOL


def test_one_value_is_refused_in_training_mode(dev):
    """... as torch refuses it ("Expected more than 1 value per channel when training", tests/test_bn2d_ref.py); nothing is written."""
    gamma, beta = ref.gamma_beta("positive")
    rm0, rv0 = ref.running_stats()
    stats = torch.zeros(_lib.size("dd_conv_stats_floats"), device=dev, dtype=f32)
    rm, rv = rm0.to(dev), rv0.to(dev)
    aff, sm, si = (torch.full((n,), -7.0, device=dev, dtype=f32) for n in (128, C, C))
    with pytest.raises(_lib.HotpathError, match="more than one value"):
        _lib.call("dd_bn2d_finalize", stats, 1, gamma.to(dev), beta.to(dev), rm, rv, ref.MOMENTUM, ref.EPS, 1, aff, sm, si)
    torch.cuda.synchronize()
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and bool((aff == -7.0).all()) and bool((sm == -7.0).all())


def test_eval_mode_needs_no_statistics_and_keeps_the_running_ones(dev):
    gamma, beta = ref.gamma_beta("signs")
    rm0, rv0 = ref.running_stats()
    for count in (1, 1408):
        aff, sm, si, rm, rv = finalize(dev, None, count, gamma, beta, rm0, rv0, False)
        torch.cuda.synchronize()
        assert torch.equal(rm.cpu().view(torch.int32), rm0.view(torch.int32)) and torch.equal(rv.cpu().view(torch.int32), rv0.view(torch.int32))
        inv = 1 / (rv0.double() + ref.EPS).sqrt()
        assert torch.equal(sm.cpu(), rm0) and ref.peak_error(si.cpu(), inv) <= ref.KERNEL_TOL
        assert ref.peak_error(aff.cpu(), ref.affine_table(rm0.double(), inv, gamma, beta)) <= ref.KERNEL_TOL


# ------------------------------------------------------------------------------------------------ dd_conv_fwd_stats
def desc_of(shape, cin, stride):
    b, h, w = shape
    return _lib.ConvDesc(b, h, w, cin, 4 if cin == 3 else cin, 32, 3, stride, 1, 0)


def packed(dev, weight, desc, kind):
    p = torch.empty(_lib.size("dd_conv_packed_floats", desc, kind), device=dev, dtype=f32)
    _lib.call("dd_conv_pack", weight.to(dev), p, desc, kind)
    return p


def conv_fwd_stats(dev, x, weight, bias, aff, desc):
    """-> (u, the finalize kernel's batch mean, inv-std) on the CPU, gamma = 1, beta = 0."""
    ho, wo = (desc.height - 1) // desc.stride + 1, (desc.width - 1) // desc.stride + 1
    u = torch.empty((desc.batch, ho, wo, C), device=dev, dtype=f32)
    stats = stats_table(dev)
    _lib.call("dd_conv_fwd_stats", x.to(dev), packed(dev, weight, desc, PACK_FWD), bias.to(dev), None if aff is None else aff.to(dev), u, stats, desc)
    _, sm, si, _, _ = finalize(dev, stats, u.numel() // C, torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C), True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(stats).all()), "dd_conv_fwd_stats must leave every row of the statistics table defined"
    return u.cpu(), sm.cpu(), si.cpu()


@pytest.mark.parametrize("ratio", ref.CONV_RATIOS)
@pytest.mark.parametrize("shape", ref.CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ref.CONV_KINDS, ids=lambda k: f"cin{k[0]}s{k[1]}")
def test_conv_epilogue_statistics(dev, kind, shape, ratio):
    """The three layers of the v2 encoder with bias = ratio x (std of the bias-free output), at the whole chip and at one compute unit.
    u against the fp64 conv at KERNEL_TOL; the finalize kernel's mean and inv-std against the fp64 statistics OF THE u THE KERNEL RETURNED,
    which separates the statistics from the rounding of the convolution."""
    cin, stride, _ = kind
    layer = ref.conv_layer(kind, shape)
    bias = ref.conv_bias(layer, ratio)
    u64 = layer["conv0"] + bias.double()
    desc = desc_of(shape, cin, stride)
    ones, zeros = torch.ones(C), torch.zeros(C)
    bad = []
    for budget in (256, 1):
        with cu_budget(budget):
            u, sm, si = conv_fwd_stats(dev, layer["x"], layer["weight"], bias, layer["affine"], desc)
        label = f"conv cin {cin} stride {stride} {shape} ratio {ratio} budget {budget}"
        err = ref.peak_error(u, u64)
        print(f"{label} u: error {err:.2e}  bound {ref.KERNEL_TOL:.2e}")
        if not err <= ref.KERNEL_TOL:
            bad.append(("u", budget, err))
        flat = u.reshape(-1, C)
        want = ref.chain(flat, ones, zeros, zeros, ones, torch.zeros_like(flat), True)
        e_ref = ref.reference_fp32_error(flat, ones, zeros, zeros, ones, torch.zeros_like(flat), True, want)
        bad += [(budget,) + b for b in judge(label, {"save_mean": sm, "save_invstd": si}, want, e_ref, ("save_mean", "save_invstd"))]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ gamma signs through the readers of u
def masked_error(got, want, skip):
    """(peak error over the elements that are not left out, fraction left out)."""
    got, want = got.double(), want.double()
    keep = ~skip
    return float(((got - want).abs() * keep).max()) / float(want.abs().max()), float(skip.double().mean())


@pytest.mark.parametrize("shape", ref.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_with_gamma_of_both_signs_and_zero(dev, shape):
    """dd_pool4_bn_fwd / _bwd.  On a zero-gamma channel with beta > 0 all four taps tie and the gradient must land on the first, as
    max_pool1d routes it; with beta < 0 nothing flows.  (1, 513, 512) is past the grid cap of these two kernels."""
    b, h, w = shape
    case = ref.pool_case(shape)
    u, aff, gp = case["u"].to(dev), case["affine"].to(dev), case["gp"].to(dev)
    pooled, dfeat = torch.empty_like(gp), torch.empty_like(u)
    _lib.call("dd_pool4_bn_fwd", u, aff, pooled, b, h, w)
    _lib.call("dd_pool4_bn_bwd", gp, u, aff, dfeat, b, h, w)
    torch.cuda.synchronize()
    e_fwd = ref.peak_error(pooled.cpu(), case["pooled"])
    e_bwd, left_out = masked_error(dfeat.cpu(), case["dfeat"], case["skip"])
    print(f"pool {shape}: pooled error {e_fwd:.2e}, dfeat error {e_bwd:.2e} ({left_out:.1e} left out)  bound {ref.KERNEL_TOL:.2e}")
    assert left_out <= ref.FLIP_CAP
    assert e_fwd <= ref.KERNEL_TOL and e_bwd <= ref.KERNEL_TOL
    gamma, beta = ref.gamma_beta("signs")
    tied = (gamma == 0) & (beta > 0)
    d = dfeat.cpu().reshape(b, h * w // 4, 4, C)
    assert torch.equal(d[:, :, 0, tied], case["gp"].reshape(b, C, h * w // 4).permute(0, 2, 1)[:, :, tied]) and bool((d[:, :, 1:, tied] == 0).all())


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_readers_with_gamma_of_both_signs_and_zero(dev, stride):
    """in_affine of dd_conv_fwd_stats, the mask of dd_conv_dgrad_bn and the input of dd_conv_wgrad_bn, the table built from gamma < 0, = 0
    and > 0; the mask pair is the input pair rolled by one channel, so the two differ in sign per channel."""
    layer = ref.sign_layer(stride)
    shape = ref.CONV_SHAPES[0]
    desc = desc_of(shape, 32, stride)
    u, _, _ = conv_fwd_stats(dev, layer["pre"], layer["weight"], layer["bias"], layer["affine"], desc)
    x, aff, gy = layer["pre"].to(dev), layer["affine"].to(dev), layer["gy"].to(dev)
    dx = torch.empty_like(x)
    _lib.call("dd_conv_dgrad_bn", gy, packed(dev, layer["weight"], desc, PACK_DGRAD_S1 if stride == 1 else PACK_DGRAD_S2), x, aff, dx, desc)
    nbytes = _lib.size("dd_conv_wgrad_workspace_bytes", desc)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    dw, db = torch.empty((C, C, 3, 3), device=dev, dtype=f32), torch.empty(C, device=dev, dtype=f32)
    _lib.call("dd_conv_wgrad_bn", x, aff, gy, dw, db, ws, nbytes, desc)
    torch.cuda.synchronize()
    e_dx, left_out = masked_error(dx.cpu(), layer["dx"], layer["skip"])
    errs = {"u": ref.peak_error(u, layer["u"]), "dx": e_dx, "dw": ref.peak_error(dw.cpu(), layer["dw"]), "dbias": ref.peak_error(db.cpu(), layer["dbias"])}
    print(f"conv readers stride {stride}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" ({left_out:.1e} of dx left out)  bound {ref.KERNEL_TOL:.2e}")
    assert left_out <= ref.FLIP_CAP
    assert all(v <= ref.KERNEL_TOL for v in errs.values()), errs
