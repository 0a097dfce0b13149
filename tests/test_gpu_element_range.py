"""GPU tests of the two element functions over the whole fp32 range: ``dd_sigmoid_softplus`` (csrc/dd_device.h: dd_sigmoid, the three
dd_bce_logits* entry points, dd_linear_sigmoid_gt) and ``adam_elem2`` / ``adam_elem`` (csrc/dd_adam.h: dd_adam_step, _multi, _rankb and
their _dev forms) against the fp64 references, on the grids and at the bounds of tests/_element_ref.py (derived there from an fp32 model
with correctly rounded primitives, not from these kernels), and against each other bit for bit -- the optimizer and the head pick among
these kernels by size and timing, so whichever one an element meets has to give the same bits.  Every launch is at most 70 k elements.
Each test prints the worst error it saw as a fraction of its bound."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _element_ref as R  # noqa: E402

D = np.float64
BANDS = (0, 2, 4, 8, 12, 16, 24, 40, 80)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _to(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _say(capsys, text):
    with capsys.disabled():
        print("\n[element range] " + text)


def _sigmoid(z):
    """ops.sigmoid for any element count (dd_sigmoid takes multiples of 4: zero padding, cut off again)."""
    from driving_dirty_amd import ops
    pad = (-z.numel()) % 4
    return ops.sigmoid(torch.cat([z, z.new_zeros(pad)]) if pad else z)[:z.numel()]


@pytest.fixture(scope="module")
def grid(dev):
    """The logit grid on the device with dd_sigmoid's probabilities, computed once."""
    z = R.logit_grid()
    zd = _to(z, dev)
    return z, zd, _sigmoid(zd)


# ------------------------------------------------------------------------------------------------ sigmoid family
def test_every_probability_output_is_dd_sigmoids_bits(dev, grid):
    """dd_bce_logits (float target), dd_bce_logits_u8 (bool) and dd_bce_logits_u8_ptrs (a tuple of two bool samples) write the
    probabilities dd_sigmoid writes, on the whole grid: vector body and the 3-element tail."""
    from driving_dirty_amd import ops
    z, zd, sig = grid
    t = _to(np.random.RandomState(1).uniform(size=z.size) < 0.5, dev)
    _, pf = ops.BceWithLogitsProbs.apply(zd, t.float())
    _, pb = ops.BceWithLogitsProbs.apply(zd, t)
    assert _same_bits(pf, sig) and _same_bits(pb, sig)
    n8 = z.size - z.size % 8
    halves = tuple(h.contiguous() for h in t[:n8].reshape(2, -1))
    _, pt = ops.BceWithLogitsProbs.apply(zd[:n8].contiguous().reshape(2, -1), halves)
    assert _same_bits(pt.reshape(-1), sig[:n8])


@pytest.mark.parametrize("tau", [0.5, 1e-6, 1.0 - 2.0 ** -24, 0.0, 1.0])
def test_linear_sigmoid_gt_is_sigmoid_of_linear_on_the_grid(dev, grid, tau):
    """K = 4, x = (1, 0, 0, 0) and the grid in the weight's first column: the contraction hands every grid logit to the epilogue's sigmoid
    unchanged, and the fused compare gives what dd_sigmoid of dd_linear_fwd's logits gives."""
    from driving_dirty_amd import ops
    z, zd, sig = grid
    n = z.size + (-z.size) % 4
    w = torch.zeros(n, 4, device=dev)
    w[:z.size, 0] = zd
    x = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev)
    y = ops.linear(x, w, None)
    assert torch.equal(y.reshape(-1)[:z.size], zd)                # the logits ARE the grid
    want = ops.sigmoid(y.reshape(-1)).reshape(1, n) > tau
    got = ops.linear_sigmoid_gt(x, w, None, tau)
    assert got.dtype == torch.bool and torch.equal(got, want)
    assert torch.equal(want.reshape(-1)[:z.size], sig > tau)
    count = int(got.sum())
    assert (0 < count < n) if tau < 1.0 else count == 0             # the compare separates the grid, except at tau = 1: nothing is above


def test_sigmoid_on_the_grid_against_fp64(dev, grid, capsys):
    """|sig - sigmoid64|: 3 x 2^-24 absolute for z >= 0, (|z| + 11) 2^-24 relative (+ 2^-126: the flush) for z < 0."""
    z, zd, sig = grid
    ref = R.sigmoid64(z)
    frac = np.abs(D(_np(sig)) - ref) / R.sig_bound(z, ref)
    pos = z >= 0
    normal = ~pos & (ref >= 2 * R.TINY)                           # at the flush the error IS the reference: 1.000 of the bound by construction
    i = int(np.argmax(np.where(normal, frac, 0)))
    _say(capsys, f"sigmoid: worst error / bound {frac[pos].max():.3f} (z >= 0), {frac[normal].max():.3f} (z < 0 above the flush, at z = "
                 f"{float(z[i])!r}), {frac[~pos & ~normal].max():.3f} (at and past the flush)")
    assert frac.max() <= 1.0
    s = _np(_sigmoid(torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0], device=dev)))
    assert np.isnan(s[0]) and s[1] == 1.0 and s[2] == 0.0 and s[3] == 0.5


def test_sigmoid_of_a_positive_logit_is_the_correctly_rounded_reciprocal(dev, capsys):
    """For z >= 0 the probability is the Newton-refined reciprocal of u = fl(1 + e): wherever u is determined despite the exponential's
    allowed error, and 1 / u is not on a rounding tie, the refinement lands on the correctly rounded 1 / u -- known to the bit
    (_element_ref.exact_sigmoid) -- from any v_rcp_f32 good to an ulp or two.  This is what the Newton step is there for: the 3 x 2^-24
    bound alone holds without it."""
    z = R.exact_sigmoid_logits()
    known, bits = R.exact_sigmoid(z)
    got = _np(_sigmoid(_to(z, dev)))
    wrong = int(np.sum(got.view(np.uint32)[known] != bits.view(np.uint32)[known]))
    _say(capsys, f"sigmoid, z >= 0: {int(known.sum())} of {z.size} probabilities known to the bit, {wrong} differ")
    assert wrong == 0


# ------------------------------------------------------------------------------------------------ loss value
def _loss(zd, td, want_dz=False, grad_scale=1.0):
    """dd_bce_logits / dd_bce_logits_u8 by the target's type -> (loss, dz); the kernel's gradient factor is grad_scale / n."""
    from driving_dirty_amd import ops
    n = zd.numel()
    loss = torch.empty((), device=zd.device, dtype=torch.float32)
    dz = torch.empty_like(zd) if want_dz else None
    name = "dd_bce_logits_u8" if td.dtype == torch.bool else "dd_bce_logits"
    ops.call(name, zd, td, loss, dz, None, n, float(grad_scale), ops._loss_ws(n, zd.device))
    return loss, dz


@pytest.mark.parametrize("k", BANDS)
def test_band_mean_loss_against_fp64(dev, k, capsys):
    """The mean BCE-with-logits of 65 539 logits with |z| in [k, k + 1].  Targets that agree with the sign (a confident, correct head: every
    term is the softplus term alone): relative error at most the softplus bound at |z| = k + 1.  All targets wrong (terms |z| + softplus):
    4 x 2^-24.  Half and half: the two bounds weighted by their share of the sum (_element_ref.band_mean_bound)."""
    z = R.band_logits(k)
    zd = _to(z, dev)
    right = (z > 0)
    mix = np.where(np.random.RandomState(k).uniform(size=z.size) < 0.5, right, ~right)
    fracs = []
    for t in (right, ~right, mix):
        ref = R.bce_logits_terms64(z, t).mean()
        loss, _ = _loss(zd, _to(t.astype(np.float32), dev))
        loss_b, _ = _loss(zd, _to(t, dev))
        assert _same_bits(loss.reshape(1), loss_b.reshape(1))
        fracs.append(abs(float(loss) - ref) / ref / R.band_mean_bound(k, z, t))
    _say(capsys, f"band {k}: mean loss error / bound: right {fracs[0]:.3f}, wrong {fracs[1]:.3f}, mixed {fracs[2]:.3f}")
    assert np.max(fracs) <= 1.0                                   # np.max: a NaN loss in any of the three is a failure


def test_softplus_per_element_against_fp64(dev, capsys):
    """The loss of ONE logit whose target agrees with its sign is the softplus term itself, bit for bit (one fp32 term, widened and
    narrowed again): single-element launches read the element's second output directly.  Every integer and half-integer |z| up to 104,
    and the |z| at which e = exp(-|z|) is k ulps of 1 for k = 1 .. 64 -- there u = fl(1 + e) is 1 + k 2^-23, the only arguments
    v_log_f32 ever sees next to 1, and log1p(e) = log(u) e / (u - 1) stands or falls with its RELATIVE accuracy at them.  Bound:
    (|z| + 12) 2^-24 relative, per element."""
    from driving_dirty_amd import ops
    z = R.softplus_points()
    zd, td = torch.zeros(z.size, 4, device=dev), torch.zeros(z.size, 4, device=dev)      # one element per 16-byte aligned row
    zd[:, 0], td[:, 0] = _to(z, dev), _to((z > 0).astype(np.float32), dev)
    out = torch.zeros(z.size, device=dev)
    ws = ops._loss_ws(1, dev)
    for i in range(z.size):
        ops.call("dd_bce_logits", zd[i], td[i], out[i:i + 1], None, None, 1, 1.0, ws)
    ref = R.softplus64(z)
    frac = np.abs(D(_np(out)) - ref) / R.softplus_bound(z, ref)
    k_part = frac[209:]
    _say(capsys, f"softplus per element: worst error / bound {frac[:209].max():.3f} on the half-integers (at |z| = "
                 f"{abs(float(z[int(np.argmax(frac[:209]))]))}), {k_part.max():.3f} at u = 1 + k 2^-23, k <= 64")
    assert frac.max() <= 1.0


@pytest.mark.parametrize("unit_scale", [True, False])
def test_logit_gradient_on_the_grid_against_fp64(dev, grid, unit_scale, capsys):
    """dz = (sig - t) gscale per element for the kernel's gscale = 1 and = 1 / n, against (sigmoid64 - t) gscale.  The bound is the
    sigmoid's absolute bound times gscale, plus what the fp32 OUTPUT costs whatever the element does: the subtraction sig - t and the
    multiply round once each (at most 2^-24 of the result each), and a result below 2^-126 may be flushed."""
    z, zd, _ = grid
    n = z.size
    t = (np.random.RandomState(2).uniform(size=n) < 0.5).astype(np.float32)
    gs = np.float32(1.0) if unit_scale else np.float32(1.0) / np.float32(n)      # dd_bce_logits forms grad_scale / (float)n
    _, dz = _loss(zd, _to(t, dev), want_dz=True, grad_scale=float(n) if unit_scale else 1.0)
    s64 = R.sigmoid64(z)
    ref = (s64 - D(t)) * D(gs)
    # two roundings of at most 2^-24 each, relative to the COMPUTED result: (1 + 2^-24)^2 - 1 and the result's own error are second
    # order, which the factor 1 + 2^-20 covers with room
    tol = D(gs) * (R.sig_bound(z, s64) + 2 * R.U24 * (1 + 2.0 ** -20) * np.abs(s64 - D(t))) + R.TINY
    frac = np.abs(D(_np(dz)) - ref) / tol
    _say(capsys, f"dz, gscale {float(gs):.3g}: worst error / bound {frac.max():.3f}")
    assert frac.max() <= 1.0


# ------------------------------------------------------------------------------------------------ Adam family
@pytest.fixture(scope="module")
def adam(dev):
    host = R.adam_grid()
    return host, tuple(_to(t, dev) for t in host)


def _flat(state, cfg, scale=None):
    """One dd_adam_step on clones of (p, g, m, v) -> (p, m, v); ``scale``: a device tensor in place of cfg's grad_scale."""
    from driving_dirty_amd import ops
    p, g, m, v = state
    p, m, v = p.clone(), m.clone(), v.clone()
    lr, b1, b2, eps, step, gs = cfg
    ops.adam_step_flat(p, g, m, v, lr, b1, b2, eps, step, gs if scale is None else scale)
    return p, m, v


def _check_adam(host, out, cfg):
    """([worst m, v, update error / bound over the bounded elements, the update's again where p's final half ulp is under 5 % of the
    bound], mismatches of m and v against the fp32 model's bits, share of bounded elements)."""
    p, g, m, v = host
    pn, mn, vn = (_np(t) for t in out)
    M, V, U, mag = R.adam64(p, g, m, v, *cfg)
    ok = R.adam_bounded(M, V, U)
    em, ev, eu = R.adam_errors(p, pn, mn, vn, M, V, U)
    tm, tv, tu = R.adam_bounds(p, M, V, U, mag)
    _, _, half = R.adam_bounds(p, M, V, U, mag, 0, 0, 0)
    with np.errstate(all="ignore"):
        fr = [float(R.error_fraction(e, t)[ok].max()) for e, t in ((em, tm), (ev, tv), (eu, tu))]      # NaN stays NaN: a failure
        rel = ok & (half <= 0.05 * tu)                             # where the bound is the relative part, not p's final rounding
        fr.append(float(R.error_fraction(eu, tu)[rel].max()) if rel.any() else 0.0)
    _, mm, vm = R.model_adam(p, g, m, v, *cfg)
    bits = int(np.sum((mm.view(np.uint32) != mn.view(np.uint32))[ok]) + np.sum((vm.view(np.uint32) != vn.view(np.uint32))[ok]))
    return fr, bits, float(ok.mean())


@pytest.mark.parametrize("step", R.ADAM_STEPS)
def test_adam_on_the_grid_against_fp64(dev, adam, step, capsys):
    """One dd_adam_step from the grid state (30 decades of g and m, 60 of v) at bias-correction step ``step``, for both beta pairs, eps
    1e-8 and 1e-3, lr 1e-3 and 1, grad_scale 1 and 0.37: m within ADAM_KM x 2^-24 of its terms' magnitude, v within ADAM_KV x 2^-24,
    p_new - p within (ADAM_KM magnitude / |M| + ADAM_KU) 2^-24 |U| + half an ulp of the larger of p and p_new (the number the final
    rounding acts on).  m and v are multiplies and fused multiply-adds
    only -- IEEE on the device -- so they also equal the fp32 model bit for bit."""
    host, state = adam
    worst, wrong_bits = [0.0, 0.0, 0.0, 0.0], 0
    for cfg in R.adam_configs(step):
        fr, bits, kept = _check_adam(host, _flat(state, cfg), cfg)
        assert kept >= 0.99
        assert np.max(fr) <= 1.0, (cfg, fr)                        # np.max keeps a NaN, which fails
        worst = [max(a, b) for a, b in zip(worst, fr)]
        wrong_bits += bits
    _say(capsys, f"adam step {step}: worst error / bound over 16 configurations: m {worst[0]:.3f}, v {worst[1]:.3f}, update {worst[2]:.3f} "
                 f"({worst[3]:.3f} where p's final rounding is under 5 % of the bound); "
                 f"m, v elements off the model's bits: {wrong_bits}")
    assert wrong_bits == 0


BIT_CONFIGS = [(1e-3, 0.9, 0.999, 1e-8, 10, 0.37), (1.0, 0.5, 0.9, 1e-3, 1, 1.0)]


@pytest.mark.parametrize("cfg", BIT_CONFIGS)
def test_adam_body_tail_multi_and_device_scale_give_the_same_bits(dev, adam, cfg):
    """The float4 body of dd_adam_step and its scalar tail (the grid rotated by three elements: what was the tail is body and the other way
    round), dd_adam_step_multi on pieces of 1, 3, 255, 256, 257 and 4099 elements, and the _dev form of each (the scale read from device
    memory) give the bits of the one flat pass."""
    from driving_dirty_amd import ops
    _, state = adam
    base = _flat(state, cfg)
    rolled = _flat(tuple(torch.roll(t, 3) for t in state), cfg)
    for a, b in zip(base, rolled):
        assert _same_bits(torch.roll(a, 3), b)
    scale = torch.tensor([cfg[5]], device=dev, dtype=torch.float32)
    for a, b in zip(base, _flat(state, cfg, scale)):
        assert _same_bits(a, b)
    lr, b1, b2, eps, step, gs = cfg
    for s in (gs, scale):
        quads, off = [], 11
        for size in (1, 3, 255, 256, 257, 4099):
            quads.append(tuple(t[off:off + size].clone() for t in state))
            off += size + 5
        ops.adam_step_multi(quads, lr, b1, b2, eps, step, s)
        off = 11
        for (p, _, m, v), size in zip(quads, (1, 3, 255, 256, 257, 4099)):
            for a, b in zip(base, (p, m, v)):
                assert _same_bits(a[off:off + size], b), size
            off += size + 5


def _log_uniform(rs, n, lo, hi):
    return (np.exp(rs.uniform(np.log(lo), np.log(hi), n)) * rs.choice([-1.0, 1.0], n)).astype(np.float32)


@pytest.mark.parametrize("n,k,blocks", [(52, 132, 1), (640, 64, 1), (16, 4036, 4)])
@pytest.mark.parametrize("cfg", BIT_CONFIGS)
def test_adam_rankb_with_one_batch_row_gives_the_flat_kernels_bits(dev, adam, n, k, blocks, cfg):
    """With one batch row the gradient dy[n] x[k] is a single product -- no summation order -- and the matrix core's fp32 multiply-add onto
    a zero accumulator rounds it once, as the fp32 multiply does: dd_adam_step_rankb must then give dd_adam_step's bits on that product, and
    on dy itself for the bias.  The three kernel forms of csrc/adam_rankb.hip that one row reaches: the LDS form (52 x 132: three k-tiles,
    ragged n- and k-tiles), the short-row form (K <= 64) and, with four workgroups per CU, the 16 x 256 wide form (64 k-tiles: K = 4036, a
    ragged last tile); each with the scale by value and from device memory.  The fourth form, adam_rankb_lds_kernel<2, 1>, is chosen for
    more than 32 batch rows only: its gradient is then a sum of 33 or more products in the matrix core's order, which no flat-kernel
    input reproduces bit for bit, so it stays with tests/test_gpu_round5.py's comparison against fp64 (rows = 64)."""
    from driving_dirty_amd import _lib, ops
    lib = _lib.lib()
    _, (pg, _, mg, vg) = adam
    rs = np.random.RandomState(n + k)
    dy, x = _to(_log_uniform(rs, n, 1e-6, 1e6).reshape(1, n), dev), _to(_log_uniform(rs, k, 1e-6, 1e6).reshape(1, k), dev)
    cut = lambda t, lo, shape: t[lo:lo + int(np.prod(shape))].clone().reshape(shape)
    p0, m0, v0 = (cut(t, 0, (n, k)) for t in (pg, mg, vg))
    b0, bm0, bv0 = (cut(t, 7, (n,)) for t in (pg, mg, vg))
    gw = (dy.t() * x).contiguous()                                  # [n, k], each element one rounded product
    want = _flat((p0.reshape(-1), gw.reshape(-1), m0.reshape(-1), v0.reshape(-1)), cfg)
    want_b = _flat((b0, dy.reshape(-1).contiguous(), bm0, bv0), cfg)
    lr, b1, b2, eps, step, gs = cfg
    assert lib.dd_set_adam_blocks_per_cu(blocks) == 0
    try:
        for s in (gs, torch.tensor([gs], device=dev, dtype=torch.float32)):
            p, m, v, b, bm, bv = (t.clone() for t in (p0, m0, v0, b0, bm0, bv0))
            ops.adam_step_rankb(p, m, v, dy, x, b, bm, bv, lr, b1, b2, eps, step, s)
            for a, c in zip(want + want_b, (p.reshape(-1), m.reshape(-1), v.reshape(-1), b, bm, bv)):
                assert _same_bits(a, c)
            p, m, v = (t.clone() for t in (p0, m0, v0))               # and without a bias: the weight's bits are the same
            ops.adam_step_rankb(p, m, v, dy, x, None, None, None, lr, b1, b2, eps, step, s)
            for a, c in zip(want, (p.reshape(-1), m.reshape(-1), v.reshape(-1))):
                assert _same_bits(a, c)
    finally:
        assert lib.dd_set_adam_blocks_per_cu(1) == 0


def _torch_adam32(p, g, m, v, lr, b1, b2, eps, step):
    pt = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[pt] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    pt.grad = torch.from_numpy(g.copy())
    opt.step()
    return pt.detach().numpy(), opt.state[pt]["exp_avg"].numpy(), opt.state[pt]["exp_avg_sq"].numpy()


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_special_values_follow_torch(dev, step):
    """Zero, negative zero, subnormal, g^2-subnormal, g^2-overflowing, infinite and NaN gradients against zero and subnormal moments: p, m
    and v are zero / finite / +inf / -inf / NaN where fp32 torch.optim.Adam (CPU, foreach=False) has them so; where the fp64 reference is
    finite and normal they are inside the bounds; and the all-zero state leaves p bit-identical.  One exception to torch's pattern: where
    the fp64 value is non-zero but below 2^-126, zero and (subnormal) finite both count -- which of the two fp32 gives there is the order
    of the operations (torch forms (-step_size m) / denom, and 1e-3 x 1e-43 underflows to zero; the kernel forms -step_size (m / denom) and
    keeps the subnormal -1e-38, which is the fp64 value)."""
    host = R.adam_special_grid()
    cfg = (1e-3, 0.9, 0.999, 1e-8, step, 1.0)
    out = _flat(tuple(_to(t, dev) for t in host), cfg)
    pn, mn, vn = (_np(t) for t in out)
    p, g, m, v = host
    M, V, U, _ = R.adam64(p, g, m, v, *cfg)
    for name, got, want, ref in zip("pmv", (pn, mn, vn), _torch_adam32(*host, *cfg[:5]), (D(p) + U, M, V)):
        cg, cw = R.value_class(got), R.value_class(want)
        with np.errstate(invalid="ignore"):
            underflow = (ref != 0) & (np.abs(ref) < R.TINY)
        bad = (cg != cw) & ~(underflow & (cg <= 1) & (cw <= 1))
        assert not bad.any(), (name, np.nonzero(bad)[0].tolist(), got[bad].tolist(), want[bad].tolist())
    fr, _, _ = _check_adam(host, out, cfg)
    assert np.max(fr) <= 1.0, fr
    still = (g == 0) & (m == 0) & (v == 0)
    assert still.sum() >= 4 and np.array_equal(pn.view(np.uint32)[still], p.view(np.uint32)[still])
