"""GPU parity of BasicAE's bf16 mixed-precision mode: the masked-view gather, the decoder's bf16 kernels layer by layer, and the
whole pre-training step against an fp64 statement of the contract.

The contract is oracle/bf16_parts.py's "torch autocast equivalent", extended to the decoder (ops_bf16.DecoderConvStackBf16):
every conv reads bf16-rounded inputs and weights, accumulates in fp32 and rounds its output to bf16 once, after bias and ReLU;
dc4's output y_hat is rounded once; dL/dy_hat and every pre-activation gradient are rounded to bf16 once; weight and bias
gradients are fp32 sums of bf16 products; the gradient handed back to fc2 is the bf16-rounded dL/d(decoder input).  The decoder's
fp64 statement of it lives here (``oracle/`` stays as it is).  bf16 outputs are compared exactly except where fp32 and fp64
accumulation orders land on different sides of a rounding boundary (one ulp, on a small fraction of the elements)."""
from argparse import Namespace

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def hu(shape, name, lo=-1.0, hi=1.0, seed=0):
    return synth.hash_uniform(shape, synth.key_salt(name, seed), lo, hi)


def assert_bf16_close(got, ref, what, max_flip_frac=5e-3, mag=None):
    """got: bf16 tensor from the GPU; ref: fp64 tensor already rounded to bf16 by the oracle.  ``mag`` (optional, ref's shape): the
    sum of the absolute values of the terms behind each element -- where hundreds of terms nearly cancel, the fp32 sum's own error
    (a few 2^-24 of ``mag``) can exceed one bf16 ulp of the small result, and that much more is allowed there."""
    got, ref = got.detach().float().cpu().double(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = (got - ref).abs()
    spacing = torch.pow(2.0, torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)     # bf16 ulp at ref
    spacing = torch.maximum(spacing, torch.full_like(spacing, 2.0 ** -133))
    allowed = 1.001 * spacing + 1e-30
    if mag is not None:
        allowed = allowed + 2.0 ** -18 * mag.detach().double().cpu()
    assert bool((diff <= allowed).all()), (what, "more than one ulp beyond the fp32 sum's error", float((diff / spacing).max()))
    frac = float((diff > 0).double().mean())
    assert frac <= max_flip_frac, (what, "fraction of one-ulp flips", frac)


def assert_sum_close(got, ref, what, tol=1e-4):
    """fp32 sums of bf16 products vs the fp64 sum of the same products: relative to the tensor's peak."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
    assert err < tol, (what, err)


def bf16r(t):
    return t.to(torch.bfloat16).to(t.dtype)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def bits_of(t_nchw):
    """[B,32,H,W] -> int32 [B,H,W] sign words (bit c = channel c > 0)."""
    pos = (t_nchw > 0).to(torch.int64)
    w = (pos << torch.arange(32).view(1, 32, 1, 1)).sum(dim=1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def bits_mask(bits):
    """int32 [B,H,W] -> 0/1 fp64 [B,32,H,W]."""
    w = bits.to(torch.int64) & 0xFFFFFFFF
    return ((w.unsqueeze(1) >> torch.arange(32).view(1, 32, 1, 1)) & 1).double()


# ------------------------------------------------------------------------------------------------ fp64 decoder contract
class _DeconvBf16(torch.autograd.Function):
    """One ConvTranspose2d of the decoder in the contract: bf16 operands, fp64 arithmetic, output rounded once after bias (+ReLU);
    backward: the pre-activation gradient rounded once, dx optionally rounded (dc1: the gradient handed back to fc2)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, relu, round_dx):
        xr, wr = bf16r(x.float()).double(), bf16r(w.float()).double()
        z = F.conv_transpose2d(xr, wr, b.double(), stride=stride, padding=pad)
        y = bf16r((F.relu(z) if relu else z).float()).double()
        ctx.save_for_backward(xr, wr, y)
        ctx.cfg = (stride, pad, relu, round_dx)
        return y

    @staticmethod
    def backward(ctx, gy):
        xr, wr, y = ctx.saved_tensors
        stride, pad, relu, round_dx = ctx.cfg
        gz = bf16r((gy * (y > 0) if relu else gy).float()).double()
        with torch.enable_grad():
            xx, ww = xr.detach().requires_grad_(), wr.detach().requires_grad_()
            out = F.conv_transpose2d(xx, ww, None, stride=stride, padding=pad)
            dx, dw = torch.autograd.grad(out, (xx, ww), gz)
        if round_dx:
            dx = bf16r(dx.float()).double()
        return dx, dw, gz.sum(dim=(0, 2, 3)), None, None, None, None


def decoder_conv_stack_ref(h, dec):
    """fp64 [B, 64*dh*dw] -> y_hat [B,3,2dh,2dw] through ``dec``'s dc1..dc4 (an oracle.ae_parts.DecoderNet, any container dtype)."""
    x = h.reshape(h.shape[0], 64, dec.deconv_dim_h, dec.deconv_dim_w)
    a1 = _DeconvBf16.apply(x, dec.dc1.weight, dec.dc1.bias, 1, 1, True, True)
    a2 = _DeconvBf16.apply(a1, dec.dc2.weight, dec.dc2.bias, 1, 1, True, False)
    a3 = _DeconvBf16.apply(a2, dec.dc3.weight, dec.dc3.bias, 2, 0, True, False)
    return _DeconvBf16.apply(a3, dec.dc4.weight, dec.dc4.bias, 1, 0, False, False)


def ae_loss_ref(enc, dec, views, rng_state):
    """The bf16 BasicAE step in fp64: masked view (same numpy draw), encoder per oracle.bf16_parts, decoder per the contract above,
    MSE against the fp32 target view."""
    from oracle import bf16_parts, steps
    np.random.set_state(rng_state)
    x, y, _ = steps.six_to_one_task(views)
    z = bf16_parts.encoder_latent(enc, bf16r(x.float()).double())
    h = dec.fc2(dec.fc1(z))
    y_hat = decoder_conv_stack_ref(h, dec)
    return ((y_hat - y.double()) ** 2).mean()


# ------------------------------------------------------------------------------------------------ 1. masked gather
@pytest.mark.parametrize("form", ["stack", "tuple", "u8"])
def test_masked_gather_bf16_against_fp32_gather(dev, form):
    from driving_dirty_amd import ops
    b, h, w = 3, 6, 11
    views = synth.camera_batch(b, h, w, seed=5).to(dev)
    if form == "stack":
        sample = views
    elif form == "tuple":
        sample = tuple(views[i] for i in range(b))
    else:
        frames = (hu((b, 6, h, w, 3), "frames", 0.0, 255.99).floor().to(torch.uint8)).to(dev)
        sample = tuple(frames[i] for i in range(b))
    for slot in range(5):
        w32, t32 = ops.wide_image(sample, "fp32", mask_slot=slot, want_target=True)
        w16, t16 = ops.wide_image(sample, "bf16", mask_slot=slot, want_target=True)
        assert w16.dtype == torch.bfloat16 and tuple(w16.shape) == (b, h, 6 * w, 4)
        assert torch.equal(w16.view(torch.int16), w32.to(torch.bfloat16).view(torch.int16)), (form, slot)
        assert t16.dtype == torch.float32 and torch.equal(t16.view(torch.int32), t32.view(torch.int32)), (form, slot)
        assert bool((w16[:, :, slot * w:(slot + 1) * w] == 0).all())
    # no target asked for: the blanked image alone
    only = ops.wide_image(sample, "bf16", mask_slot=2, want_target=False)
    assert torch.equal(only.view(torch.int16), ops.wide_image(sample, "bf16", mask_slot=2, want_target=True)[0].view(torch.int16))


# ------------------------------------------------------------------------------------------------ 2. kernels
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 8, 11), (2, 13, 37)]
FULL = (2, 128, 153)


@pytest.mark.parametrize("shape", SHAPES + [FULL])
def test_dc1_against_oracle(dev, shape):
    from driving_dirty_amd import ops_bf16
    b, dh, dw = shape
    h = hu((b, 64 * dh * dw), "h", seed=dh)
    w1 = hu((64, 32, 3, 3), "w1", -0.1, 0.1, seed=dw)
    b1 = hu((32,), "b1", -0.1, 0.1)
    x_lo, x_hi = ops_bf16.dec_split64(h.to(dev), dh, dw)
    x = h.double().view(b, 64, dh, dw)
    xr = bf16r(x.float()).double()
    assert torch.equal(torch.cat((x_lo, x_hi), dim=3).float().cpu().double(), nhwc(xr))      # the one rounding of fc2's output
    a1, bits = ops_bf16.dec_dc1_fwd(x_lo, x_hi, w1.to(dev), b1.to(dev))
    z = F.conv_transpose2d(xr, bf16r(w1).double(), b1.double(), padding=1)
    ref = bf16r(F.relu(z).float()).double()
    mag = F.conv_transpose2d(xr.abs(), bf16r(w1).double().abs(), b1.double().abs(), padding=1)
    assert_bf16_close(a1, nhwc(ref), "dc1 fwd", mag=nhwc(mag))
    a1_got = nchw(a1.float().cpu())
    assert torch.equal(bits.cpu(), bits_of(a1_got))
    # data and weight gradients from a bf16 pre-activation gradient
    g1 = bf16r(hu((b, 32, dh, dw), "g1", seed=b)).double()
    xx = xr.clone().requires_grad_()
    ww = bf16r(w1).double().requires_grad_()
    dx, dwt = torch.autograd.grad(F.conv_transpose2d(xx, ww, None, padding=1), (xx, ww), g1)
    g1_dev = nhwc(g1.float()).to(torch.bfloat16).to(dev)
    gh, gw, gb = ops_bf16.dec_dc1_bwd(x_lo, x_hi, g1_dev, w1.to(dev))
    assert gh.dtype == torch.float32 and tuple(gh.shape) == (b, 64 * dh * dw)
    mag = torch.autograd.grad(F.conv_transpose2d(xx, ww.detach().abs(), None, padding=1), xx, g1.abs())[0]
    assert_bf16_close(gh.view(b, 64, dh, dw).to(torch.bfloat16), bf16r(dx.float()).double(), "dc1 dgrad", mag=mag)
    assert torch.equal(gh.cpu(), gh.cpu().to(torch.bfloat16).float())                        # bf16 values in fp32 storage
    assert_sum_close(gw, dwt, "dc1 wgrad")
    assert_sum_close(gb, g1.sum(dim=(0, 2, 3)), "dc1 bias grad")


@pytest.mark.parametrize("shape", SHAPES + [FULL])
def test_dc3_dc4_against_oracle(dev, shape):
    from driving_dirty_amd import ops_bf16
    b, dh, dw = shape
    a2 = bf16r(hu((b, 32, dh, dw), "a2", 0.0, 1.0, seed=dh).clamp_min(0.2) - 0.2).double()      # ReLU output: a fifth zeros
    w3 = hu((32, 32, 2, 2), "w3", -0.2, 0.2, seed=dw)
    b3 = hu((32,), "b3", -0.1, 0.1)
    w4 = hu((32, 3, 1, 1), "w4", -0.3, 0.3)
    b4 = hu((3,), "b4", -0.1, 0.1)
    a2_dev = nhwc(a2.float()).to(torch.bfloat16).to(dev)
    a3, y = ops_bf16.dec_dc34_fwd(a2_dev, w3.to(dev), b3.to(dev), w4.to(dev), b4.to(dev))
    z3 = F.conv_transpose2d(a2, bf16r(w3).double(), b3.double(), stride=2)
    mag = F.conv_transpose2d(a2.abs(), bf16r(w3).double().abs(), b3.double().abs(), stride=2)
    assert_bf16_close(a3, nhwc(bf16r(F.relu(z3).float()).double()), "dc3 fwd", mag=nhwc(mag))
    a3_got = nchw(a3.float().cpu()).double()                    # dc4 from the bf16 activation as stored
    y_ref = bf16r(F.conv_transpose2d(a3_got, bf16r(w4).double(), b4.double()).float()).double()
    assert y.dtype == torch.float32
    mag = F.conv_transpose2d(a3_got.abs(), bf16r(w4).double().abs(), b4.double().abs())
    assert_bf16_close(y.to(torch.bfloat16), y_ref, "dc4 fwd", mag=mag)

    # dc4 backward: g3 with dc3's ReLU mask, dc4's weight / bias gradients
    gy = hu((b, 3, 2 * dh, 2 * dw), "gy", -1e-2, 1e-2, seed=b)
    g3, dw4, db4 = ops_bf16.dec_dc4_bwd(gy.to(dev), a3, w4.to(dev))
    gyr = bf16r(gy).double()
    g3_ref = bf16r((torch.einsum("bkhw,ck->bchw", gyr, bf16r(w4).double().view(32, 3)) * (a3_got > 0)).float()).double()
    mag = torch.einsum("bkhw,ck->bchw", gyr.abs(), bf16r(w4).double().view(32, 3).abs())
    assert_bf16_close(g3, nhwc(g3_ref), "dc4 dgrad", mag=nhwc(mag))
    assert_sum_close(dw4, torch.einsum("bchw,bkhw->ck", a3_got, gyr).view(32, 3, 1, 1), "dc4 wgrad")
    assert_sum_close(db4, gyr.sum(dim=(0, 2, 3)), "dc4 bias grad")

    # dc3 backward from the GPU's g3: data gradient with dc2's ReLU mask, weight gradient
    g3_got = nchw(g3.float().cpu()).double()
    bits2 = bits_of(a2)
    xx, ww = a2.clone().requires_grad_(), bf16r(w3).double().requires_grad_()
    dx, dwt = torch.autograd.grad(F.conv_transpose2d(xx, ww, None, stride=2), (xx, ww), g3_got)
    g2 = ops_bf16.dec_dc3_dgrad(g3, w3.to(dev), bits2.to(dev))
    mag = torch.autograd.grad(F.conv_transpose2d(xx, ww.detach().abs(), None, stride=2), xx, g3_got.abs())[0]
    assert_bf16_close(g2, nhwc(bf16r((dx * bits_mask(bits2)).float()).double()), "dc3 dgrad", mag=nhwc(mag))
    gw, gb = ops_bf16.dec_dc3_wgrad(a2_dev, g3)
    assert_sum_close(gw, dwt, "dc3 wgrad")
    assert_sum_close(gb, g3_got.sum(dim=(0, 2, 3)), "dc3 bias grad")


def test_decoder_kernels_are_deterministic(dev):
    """Every weight gradient of the decoder goes through a fixed-order reduction: repeated calls give the same bits."""
    from driving_dirty_amd import ops_bf16
    b, dh, dw = 2, 21, 30
    x_lo, x_hi = ops_bf16.dec_split64(hu((b, 64 * dh * dw), "h").to(dev), dh, dw)
    g1 = hu((b, dh, dw, 32), "g1").to(torch.bfloat16).to(dev)
    a2 = hu((b, dh, dw, 32), "a2").to(torch.bfloat16).to(dev)
    g3 = hu((b, 2 * dh, 2 * dw, 32), "g3").to(torch.bfloat16).to(dev)
    a3 = hu((b, 2 * dh, 2 * dw, 32), "a3").to(torch.bfloat16).to(dev)
    gy = hu((b, 3, 2 * dh, 2 * dw), "gy").to(dev)
    w1, w4 = hu((64, 32, 3, 3), "w1").to(dev), hu((32, 3, 1, 1), "w4").to(dev)
    for call in (lambda: ops_bf16.dec_dc1_bwd(x_lo, x_hi, g1, w1), lambda: ops_bf16.dec_dc3_wgrad(a2, g3),
                 lambda: ops_bf16.dec_dc4_bwd(gy, a3, w4)):
        first, second = call(), call()
        assert all(torch.equal(p, q) for p, q in zip(first, second))


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals(dev):
    from driving_dirty_amd import _lib, ops, ops_bf16
    lib = _lib.lib()
    a2 = torch.zeros((1, 4, 5, 32), device=dev, dtype=torch.bfloat16)
    w3, b3 = torch.zeros((32, 32, 2, 2), device=dev), torch.zeros(32, device=dev)
    w4, b4 = torch.zeros((32, 3, 1, 1), device=dev), torch.zeros(3, device=dev)
    with pytest.raises(_lib.HotpathError):                      # fp32 activation where bf16 is expected
        ops_bf16.dec_dc34_fwd(a2.float(), w3, b3, w4, b4)
    with pytest.raises(_lib.HotpathError):                      # wrong weight shape
        ops_bf16.dec_dc34_fwd(a2, w3[:16], b3, w4, b4)
    with pytest.raises(_lib.HotpathError):                      # fc2 output of the wrong length
        ops_bf16.dec_split64(torch.zeros((1, 64 * 4 * 5 + 1), device=dev), 4, 5)
    with pytest.raises(_lib.HotpathError):                      # halves of different shapes
        ops_bf16.dec_dc1_fwd(a2, a2[:, :3].contiguous(), torch.zeros((64, 32, 3, 3), device=dev), b3)
    with pytest.raises(_lib.HotpathError):                      # sign words of the wrong dtype
        ops_bf16.dec_dc3_dgrad(torch.zeros((1, 8, 10, 32), device=dev, dtype=torch.bfloat16), w3,
                               torch.zeros((1, 4, 5), device=dev, dtype=torch.int64))
    with pytest.raises(_lib.HotpathError):                      # an odd grid is not dc3's output
        ops_bf16.dec_dc4_bwd(torch.zeros((1, 3, 7, 10), device=dev), torch.zeros((1, 7, 10, 32), device=dev, dtype=torch.bfloat16), w4)
    with pytest.raises(_lib.HotpathError):                      # mask slot out of range
        ops.wide_image(torch.zeros((1, 6, 3, 4, 4), device=dev), "bf16", mask_slot=6, want_target=True)
    # the C ABI itself: bad descriptors return non-zero with a message, before any launch
    assert lib.dd_dec_bf16_wgrad_workspace_bytes(2, 1, 4, 4) < 0
    assert lib.dd_dec_bf16_wgrad_workspace_bytes(1, 1, 4, 4) < 0      # dc1 has no workspace of its own
    assert lib.dd_dec_bf16_wgrad_workspace_bytes(3, 0, 4, 4) < 0
    assert lib.dd_dec_bf16_dc1_fwd(None, None, None, None, None, None, 1, 4, 4, None) != 0
    assert lib.dd_dec_bf16_split64(None, None, None, 1, 4, 4, None) != 0
    assert lib.dd_dec_bf16_dc34_fwd(a2.data_ptr(), w3.data_ptr(), b3.data_ptr(), w4.data_ptr(), b4.data_ptr(), a2.data_ptr(),
                                    w3.data_ptr(), 1, 0, 5, None) != 0
    assert b"non-positive" in lib.dd_last_error()
    ws = torch.empty(16, device=dev, dtype=torch.uint8)
    assert lib.dd_dec_bf16_dc3_wgrad(a2.data_ptr(), a2.data_ptr(), w3.data_ptr(), b3.data_ptr(), 1, 4, 5, ws.data_ptr(), 16, None) != 0
    assert b"workspace" in lib.dd_last_error()
    assert lib.dd_stitch6_bf16_masked(a2.data_ptr(), a2.data_ptr(), None, 1, 1, 1, 7, None) != 0


# ------------------------------------------------------------------------------------------------ 4. the model against the oracle
HP = dict(hidden_dim=16, latent_dim=8, input_height=16, input_width=132, output_height=16, output_width=22)


def _small_ae(seed, precision):
    from driving_dirty_amd.autoencoder import BasicAE
    ae = BasicAE(Namespace(precision=precision, learning_rate=1e-3, output_img_freq=10 ** 9, **HP))
    synth.fill_module(ae, seed=seed)
    for blk in (ae.encoder.fc1, ae.encoder.fc2, ae.decoder.fc1, ae.decoder.fc2):
        blk.drop_p = 0.0
    return ae


def _ref_nets(ae):
    from oracle import ae_parts
    enc = ae_parts.EncoderNet(HP["hidden_dim"], HP["latent_dim"], 3, HP["input_height"], HP["input_width"]).double()
    dec = ae_parts.DecoderNet(HP["hidden_dim"], HP["latent_dim"], 3, HP["output_height"], HP["output_width"]).double()
    enc.load_state_dict(ae.encoder.state_dict())
    dec.load_state_dict(ae.decoder.state_dict())
    for blk in (enc.fc1, enc.fc2, dec.fc1, dec.fc2):
        blk.drop_p = 0.0
    return enc, dec


def _assert_grads(named, refs, what):
    for k, p in named:
        r = refs[k].grad.double()
        floor = 1e-30
        if k.endswith(("fc1.bias", "fc_z_out.bias")):      # a Linear bias in front of BatchNorm (z feeds the decoder's): zero by construction
            floor = float(refs[k[:-4] + "weight"].grad.abs().max())
        assert bool(torch.isfinite(p.grad).all()), (what, k)
        err = float((p.grad.cpu().double() - r).abs().max() / max(float(r.abs().max()), floor))
        assert err < 1e-2, (what, k, err)


def test_basic_ae_step_in_bf16_against_oracle(dev):
    """BasicAE(precision='bf16').training_step + backward vs the fp64 contract.

    The loss is compared end to end.  The gradients are compared stage by stage on identical inputs: the oracle decoder runs on the
    GPU's latent z, the oracle encoder tail on the GPU's pooled conv features driven by the GPU's dL/dz, the oracle conv stack driven
    by the GPU's dL/d(pooled).  End to end they are not comparable at this size:
    the decoder's DenseBlocks normalise over a batch of 3, which multiplies a difference in z by 70-300x in h (measured, in the
    fp32 path as much as in bf16 -- fp32 vs fp64 alone puts decoder.fc2.fc_bn's gradient 4e-2 of peak apart), so the
    encoder's contract-conforming one-ulp flips would dominate every comparison behind it."""
    from oracle import bf16_parts, steps
    ae = _small_ae(31, "bf16")
    enc, dec = _ref_nets(ae)
    ae = ae.to(dev)
    assert ae.encoder.precision == "bf16" and ae.decoder.precision == "bf16"
    seen = {}

    def keep_z(module, inputs, output):
        inputs[0].retain_grad()
        seen["z"] = inputs[0]
    hook = ae.decoder.register_forward_hook(keep_z)
    views = synth.camera_batch(3, 16, 22, seed=31)
    np.random.seed(7)
    state = np.random.get_state()
    out = ae.training_step(views.to(dev), 0)
    out["loss"].backward()
    hook.remove()
    z, gz = seen["z"].detach().cpu().double(), seen["z"].grad.detach().cpu().double()

    ref = ae_loss_ref(enc, dec, views, state)
    assert abs(float(out["loss"].detach()) - float(ref.detach())) / float(ref.detach()) < 1e-4

    # decoder half: the oracle decoder on the GPU's z
    enc.zero_grad()
    dec.zero_grad()
    np.random.set_state(state)
    x, y, _ = steps.six_to_one_task(views)
    zr = z.clone().requires_grad_()
    y_hat = decoder_conv_stack_ref(dec.fc2(dec.fc1(zr)), dec)
    ((y_hat - y.double()) ** 2).mean().backward()
    _assert_grads([(k, p) for k, p in ae.decoder.named_parameters()], dict(dec.named_parameters()), "decoder")
    err = float((gz - zr.grad).abs().max() / zr.grad.abs().max())
    assert err < 1e-2, ("dL/dz", err)

    # encoder half, the same way one level down (its FC tail normalises over the batch of 3 as well): the oracle tail on the GPU's
    # pooled conv features, driven by the GPU's dL/dz; the oracle conv stack driven by the GPU's dL/d(pooled)
    from driving_dirty_amd import ops, ops_bf16
    step_grads = {k: p.grad.detach().clone() for k, p in ae.encoder.named_parameters()}
    np.random.set_state(state)
    slot = int(np.random.randint(0, 5))
    wide4 = ops.wide_image(views.to(dev), "bf16", mask_slot=slot, want_target=True)[0]
    e = ae.encoder
    pooled = ops_bf16.encoder_conv_stack(wide4, e.c1, e.c2, e.c3).detach().requires_grad_()
    e._tail(pooled, (None, None)).backward(seen["z"].grad)                 # the kernels are deterministic: the step's dL/d(pooled)
    gp = pooled.grad.detach().cpu().double()
    for k, p in e.named_parameters():
        p.grad = step_grads[k]
    pr = pooled.detach().cpu().double().requires_grad_()
    enc.fc_z_out(enc.fc2(enc.fc1(pr))).backward(gz)
    err = float((gp - pr.grad).abs().max() / pr.grad.abs().max())
    assert err < 1e-2, ("dL/d(pooled)", err)
    pooled_ref, _ = bf16_parts.conv_stack_pooled(bf16r(x.float()).double(), enc.c1, enc.c2, enc.c3)
    pooled_ref.backward(gp)
    _assert_grads([(k, p) for k, p in e.named_parameters()], dict(enc.named_parameters()), "encoder")

    # the same module in fp32: bf16 moves the loss by no more than bf16 resolution
    ae.zero_grad()
    ae.precision = "fp32"
    assert ae.encoder.precision == "fp32" and ae.decoder.precision == "fp32"
    np.random.set_state(state)
    l32 = ae.training_step(views.to(dev), 0)["loss"]
    assert abs(float(l32.detach()) - float(out["loss"].detach())) / float(l32.detach()) < 1e-2


def test_basic_ae_bf16_takes_uint8_frames_and_sample_tuples(dev):
    """The three input forms give the same bf16 step (the uint8 frames through /255 in the gather)."""
    ae = _small_ae(37, "bf16").to(dev)
    views = synth.camera_batch(2, 16, 22, seed=37)
    frames = (views * 255).round().to(torch.uint8)
    as_float = frames.float() / 255
    losses = []
    for sample in (as_float.to(dev), tuple(as_float.to(dev)), tuple(frames.permute(0, 1, 3, 4, 2).contiguous().to(dev))):
        np.random.seed(3)
        losses.append(float(ae.training_step(sample, 0)["loss"].detach()))
    assert losses[0] == losses[1] == losses[2], losses


def test_roadmap_inherits_bf16_from_the_pretrained_ae(dev):
    from driving_dirty_amd.roadmap import RoadMapBCE
    ae = _small_ae(41, "bf16")
    model = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=10 ** 9)).to(dev)
    assert model.ae.encoder.precision == "bf16"
    views = synth.camera_batch(2, 16, 22, seed=41)
    road = synth.road_maps(2, seed=41)
    out = model.training_step((tuple(views.to(dev)), None, tuple(road.to(dev))), 0)
    out["loss"].backward()
    assert torch.isfinite(out["loss"]) and torch.isfinite(model.fc1.weight.grad).all()


# ------------------------------------------------------------------------------------------------ 5. full size (config 1 shapes)
FULL_HP = dict(hidden_dim=128, latent_dim=64, input_height=256, input_width=1836, output_height=256, output_width=306)


def _full_ae(precision):
    from driving_dirty_amd.autoencoder import BasicAE
    torch.manual_seed(0)
    ae = BasicAE(Namespace(precision=precision, learning_rate=1e-3, output_img_freq=10 ** 9, **FULL_HP))
    synth.fill_module(ae, seed=53)
    for blk in (ae.encoder.fc1, ae.encoder.fc2, ae.decoder.fc1, ae.decoder.fc2):
        blk.drop_p = 0.0
    return ae


def test_full_size_bf16_step(dev):
    from driving_dirty_amd.train import TrainStep
    views = synth.camera_batch(4, 256, 306, seed=53).to(dev)
    ae = _full_ae("bf16").to(dev)
    np.random.seed(11)
    out = ae.training_step(views, 0)
    out["loss"].backward()
    l16 = float(out["loss"].detach())
    for k, p in ae.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    ae.zero_grad()
    ae.precision = "fp32"
    np.random.seed(11)
    l32 = float(ae.training_step(views, 0)["loss"].detach())
    assert abs(l16 - l32) / l32 < 1e-2, (l16, l32)
    ae.precision = "bf16"
    ae.zero_grad(set_to_none=True)

    # one TrainStep (rank-B pass for the big Linear layers, optimizer after the backward) == training_step + backward + torch Adam
    twin = _full_ae("bf16").to(dev)
    ts = TrainStep(ae, lr=1e-3, scheduler=False)
    assert not ts.overlap, "a bf16 BasicAE has no MFMA-bound stretch to hide the optimizer under"
    assert ts.fused, "the decoder's fc2 / the encoder's fc1 should take the rank-B pass"
    np.random.seed(12)
    ts(views, 0)
    torch.cuda.synchronize()
    assert ae.decoder.fc2.fc1.weight.grad is None, "the decoder fc2 weight gradient should be formed inside its Adam pass"
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    np.random.seed(12)
    twin.training_step(views, 0)["loss"].backward()
    opt.step()
    for (k, p), (_, q) in zip(ae.named_parameters(), twin.named_parameters()):
        d = (p.detach() - q.detach()).abs()
        # one Adam step moves a weight by at most lr; the two paths sum the big weight gradients in different orders, which can flip
        # the sign of a gradient that is zero to within that order
        assert float(d.max()) <= 2.05e-3, (k, float(d.max()))
        assert float(d.mean()) < 1e-5, (k, float(d.mean()))
    ts.close()
