"""GPU parity tests: the HIP hot path (through the C ABI) against the CPU oracle and the golden fixtures.

Tolerance: north_star asks for 1e-3 relative fp32.  The fp32 MFMA path is an exact-fp32 fma chain, so the
kernels are held to 2e-5 of the tensor's peak magnitude here and whole-model chains to 1e-3.
Run with ``pytest -m gpu`` on an MI355X.
"""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

KERNEL_TOL = 2e-5
CHAIN_TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()          # raises if the HIP library is missing: no silent fallback
    return torch.device("cuda:0")


def rel_err(got, ref, floor=1e-30):
    """max |got-ref| relative to the reference tensor's peak magnitude (at least ``floor``).

    ``floor`` matters for gradients that are mathematically zero (a Linear bias in front of a
    train-mode BatchNorm): the fp64 reference holds ~1e-15 there, any fp32 path holds ~1e-6.
    """
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(floor))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def hu(shape, name, lo=-1.0, hi=1.0):
    return synth.hash_uniform(shape, synth.key_salt(name), lo, hi)


CONV_SHAPES = [(2, 7, 45), (1, 16, 22), (2, 33, 70), (1, 5, 131)]


@pytest.mark.parametrize("b,h,w", CONV_SHAPES)
@pytest.mark.parametrize("cin,stride", [(3, 1), (32, 1), (32, 2)])
@pytest.mark.parametrize("rows", [0, 5])
def test_conv_fwd_dgrad_wgrad(dev, b, h, w, cin, stride, rows):
    """One conv layer: forward (bias+ReLU), data gradient (with fused ReLU mask) and weight/bias gradient."""
    from driving_dirty_amd import ops
    x = hu((b, cin, h, w), f"x{b}{h}{w}{cin}", 0.0, 1.0).double().requires_grad_(True)
    wt = hu((32, cin, 3, 3), f"w{cin}{stride}", -0.3, 0.3).double().requires_grad_(True)
    bias = hu((32,), f"b{cin}{stride}", -0.2, 0.2).double().requires_grad_(True)
    y_ref = F.relu(F.conv2d(x, wt, bias, stride=stride, padding=1))
    gy = hu(tuple(y_ref.shape), f"gy{b}{h}{w}{stride}").double()
    gy_m = gy * (y_ref > 0)                       # gradient after this layer's ReLU
    y_ref.backward(gy)

    desc = ops.conv_desc(b, h, w, cin, stride, rows)
    xd = x.detach().float()
    x_nhwc = ops.nchw_to_nhwc(xd.to(dev), 4 if cin == 3 else 32)
    wd, bd = wt.detach().float().to(dev), bias.detach().float().to(dev)
    y = ops.conv_fwd(x_nhwc, ops.conv_pack(wd, desc, ops.PACK_FWD), bd, desc)
    assert rel_err(y.permute(0, 3, 1, 2), y_ref) < KERNEL_TOL

    g = nhwc(gy_m.float()).to(dev)
    dw, db = ops.conv_wgrad(x_nhwc, g, desc)
    assert rel_err(dw, wt.grad) < KERNEL_TOL
    assert rel_err(db, bias.grad) < KERNEL_TOL

    if cin == 32:
        kind = ops.PACK_DGRAD_S1 if stride == 1 else ops.PACK_DGRAD_S2
        dx = ops.conv_dgrad(g, ops.conv_pack(wd, desc, kind), None, desc)
        assert rel_err(dx.permute(0, 3, 1, 2), x.grad) < KERNEL_TOL
        # fused ReLU mask of the previous layer: x plays the role of that layer's output
        xm = (x.detach() - 0.5).float()
        dxm = ops.conv_dgrad(g, ops.conv_pack(wd, desc, kind), nhwc(xm).to(dev), desc)
        assert rel_err(dxm.permute(0, 3, 1, 2), x.grad * (xm > 0)) < KERNEL_TOL
        # the same mask as a bit plane (one uint32 per pixel), as the forward's *_relu_bits variant writes it
        bits = ((xm > 0).long() << torch.arange(32).view(1, 32, 1, 1)).sum(1)
        bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).to(dev)
        dxb = ops.conv_dgrad_bits(g, ops.conv_pack(wd, desc, kind), bits, desc)
        assert torch.equal(dxb, dxm)
    yb, sb = ops.conv_fwd_bits(x_nhwc, ops.conv_pack(wd, desc, ops.PACK_FWD), bd, desc)
    assert torch.equal(yb, y)
    want = ((y > 0).long() << torch.arange(32, device=dev)).sum(-1)
    assert torch.equal(sb.long() & 0xFFFFFFFF, want)


@pytest.mark.parametrize("b,h,w", CONV_SHAPES + [(1, 1, 1), (1, 3, 64), (2, 4, 33)])
@pytest.mark.parametrize("rows", [0, 3])
def test_conv_winograd_fwd_dgrad_wgrad(dev, b, h, w, rows):
    """The Winograd F(2,3) kernels of the 32 -> 32 stride-1 layer: forward (bias + ReLU + sign bits) and data gradient
    (sign-bit mask) against the fp64 oracle, and against the direct kernels' sign bits."""
    from driving_dirty_amd import _lib, ops
    x = hu((b, 32, h, w), f"wx{b}{h}{w}", 0.0, 1.0).double().requires_grad_(True)
    wt = hu((32, 32, 3, 3), "ww", -0.3, 0.3).double()
    bias = hu((32,), "wb", -0.2, 0.2).double()
    y_ref = F.relu(F.conv2d(x, wt, bias, padding=1))
    gy = hu(tuple(y_ref.shape), f"wgy{b}{h}{w}").double() * (y_ref > 0)
    y_ref.backward(gy)
    desc = ops.conv_desc(b, h, w, 32, 1, rows)
    x_nhwc = ops.nchw_to_nhwc(x.detach().float().to(dev), 32)
    wd, bd = wt.float().to(dev), bias.float().to(dev)
    y, bits = ops.conv_wino_fwd_bits(x_nhwc, ops.conv_wino_pack(wd, desc, 0), bd, desc)
    assert rel_err(y.permute(0, 3, 1, 2), y_ref) < KERNEL_TOL
    want = ((y > 0).long() << torch.arange(32, device=dev)).sum(-1)
    assert torch.equal(bits.long() & 0xFFFFFFFF, want)
    xm = x.detach().float() - 0.5
    mbits = ((xm > 0).long() << torch.arange(32).view(1, 32, 1, 1)).sum(1)
    mbits = torch.where(mbits >= 2 ** 31, mbits - 2 ** 32, mbits).to(torch.int32).to(dev)
    dx = ops.conv_wino_dgrad_bits(nhwc(gy.float()).to(dev), ops.conv_wino_pack(wd, desc, 1), mbits, desc)
    assert rel_err(dx.permute(0, 3, 1, 2), x.grad * (xm > 0)) < KERNEL_TOL
    # the 2-D form F(2x2,3x3): same contract
    y2, bits2 = ops.conv_wino2_fwd_bits(x_nhwc, ops.conv_wino2_pack(wd, desc, 0), bd, desc)
    assert rel_err(y2.permute(0, 3, 1, 2), y_ref) < KERNEL_TOL
    assert torch.equal(bits2.long() & 0xFFFFFFFF, ((y2 > 0).long() << torch.arange(32, device=dev)).sum(-1))
    dx2 = ops.conv_wino2_dgrad_bits(nhwc(gy.float()).to(dev), ops.conv_wino2_pack(wd, desc, 1), mbits, desc)
    assert rel_err(dx2.permute(0, 3, 1, 2), x.grad * (xm > 0)) < KERNEL_TOL
    wt64 = wt.clone().requires_grad_(True)
    bias64 = bias.clone().requires_grad_(True)
    F.conv2d(x.detach(), wt64, bias64, padding=1).backward(gy)
    dw, db = ops.conv_wino_wgrad(x_nhwc, nhwc(gy.float()).to(dev), desc)
    assert rel_err(dw, wt64.grad) < KERNEL_TOL
    assert rel_err(db, bias64.grad) < KERNEL_TOL
    dw2, db2 = ops.conv_wino2_wgrad(x_nhwc, nhwc(gy.float()).to(dev), desc)
    assert rel_err(dw2, wt64.grad) < KERNEL_TOL
    assert rel_err(db2, bias64.grad) < KERNEL_TOL
    # the same data gradient consumed in place by the 3 -> 32 layer's weight gradient (g1 never written):
    # dW1 / db1 of conv2d(img, w1) for the upstream gradient g1 = dx2, against fp64 and against the two-kernel path
    img = hu((b, 3, h, w), f"wimg{b}{h}{w}", 0.0, 1.0).double()
    w1 = torch.zeros(32, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    b1 = torch.zeros(32, dtype=torch.float64, requires_grad=True)
    F.conv2d(img, w1, b1, padding=1).backward(x.grad * (xm > 0))
    img4 = torch.zeros(b, h, w, 4)
    img4[..., :3] = img.float().permute(0, 2, 3, 1)
    img4 = img4.to(dev)
    dw1, db1 = ops.conv_wino2_dgrad_w1(nhwc(gy.float()).to(dev), ops.conv_wino2_pack(wd, desc, 1), mbits, img4, desc)
    assert rel_err(dw1, w1.grad) < KERNEL_TOL
    assert rel_err(db1, b1.grad) < KERNEL_TOL
    dw1b, db1b = ops.conv_wgrad(img4, dx2, ops.conv_desc(b, h, w, 3, 1, rows))
    assert rel_err(dw1, dw1b) < KERNEL_TOL and rel_err(db1, db1b) < KERNEL_TOL
    with pytest.raises(_lib.HotpathError):
        ops.conv_wino_pack(wd, ops.conv_desc(b, h, w, 32, 2), 0)           # stride 2 has no Winograd path


@pytest.mark.parametrize("b,h,w", [(1, 4, 4), (2, 8, 40)])
def test_conv_wino2_wgrad_in_two_calls(dev, b, h, w):
    """dd_conv_wino2_wgrad_partials + dd_conv_wino2_wgrad_finish find the partials where dd_conv_wino2_wgrad's two halves do (one
    workspace layout, csrc/conv_wino2.inc Wino2WgradWs): the same bits from both, and fp64's values -- what holds the layout: a
    wrong offset of the bias rows or of the chunk sums gives wrong sums.  The smallest shape ops.wino2_desc accepts (one
    workgroup: the offsets are one partial long), and 16 row tiles = four workgroups."""
    from driving_dirty_amd import ops
    desc = ops.wino2_desc(b, h, w)
    assert desc is not None
    x = hu((b, 32, h, w), f"w2x{b}{h}{w}", 0.0, 1.0).double()
    gy = hu((b, 32, h, w), f"w2gy{b}{h}{w}").double()
    wt = torch.zeros(32, 32, 3, 3, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(32, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wt, bias, padding=1).backward(gy)
    xd, gd = nhwc(x.float()).to(dev), nhwc(gy.float()).to(dev)
    dw, db = ops.conv_wino2_wgrad(xd, gd, desc)
    dw2, db2, done = ops.conv_wino2_wgrad(xd, gd, desc, finish_stream=torch.cuda.Stream())
    torch.cuda.current_stream().wait_event(done)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    assert rel_err(dw, wt.grad) < KERNEL_TOL and rel_err(db, bias.grad) < KERNEL_TOL


def test_conv_refuses_unsupported(dev):
    from driving_dirty_amd import _lib, ops
    d = _lib.ConvDesc(1, 8, 8, 32, 32, 32, 5, 1, 2, 0)
    with pytest.raises(_lib.HotpathError):
        ops.conv_pack(torch.zeros(32, 32, 3, 3, device=dev), d, 0)


@pytest.mark.parametrize("b,h,w,slot", [(2, 5, 7, -1), (3, 16, 22, 2), (1, 9, 306, 4)])
def test_stitch6(dev, b, h, w, slot):
    from driving_dirty_amd import ops
    from oracle import steps
    v = hu((b, 6, 3, h, w), "views", 0.0, 1.0)
    wide4, wide, tgt = ops.stitch6(v.to(dev), mask_slot=slot, want_nchw=True, want_target=slot >= 0)
    ref = steps.wide_stitch(v).clone()
    if slot >= 0:
        y_ref = ref[..., slot * w:(slot + 1) * w].clone()
        ref[..., slot * w:(slot + 1) * w] = 0
        assert torch.equal(tgt.cpu(), y_ref)
    assert torch.equal(wide.cpu(), ref)
    assert torch.equal(wide4[..., :3].permute(0, 3, 1, 2).cpu(), ref)
    assert float(wide4[..., 3].abs().max()) == 0.0
    if slot < 0:      # the collate's tuple of per-sample tensors, gathered without the stack copy
        samples = [v[i].clone().to(dev) for i in range(b)]
        assert torch.equal(ops.stitch6_samples(samples), wide4)


@pytest.mark.parametrize("b,c,h,w", [(2, 32, 8, 11), (2, 32, 16, 15), (3, 32, 5, 7), (1, 32, 3, 3)])
def test_pool4_nchw_order(dev, b, c, h, w):
    """max_pool1d(4) over the NCHW-flattened feature computed from an NHWC buffer, windows straddling rows."""
    from driving_dirty_amd import ops
    feat = torch.relu(hu((b, c, h, w), f"feat{h}{w}")).requires_grad_(True)
    flat = feat.reshape(b, 1, -1)
    ref = F.max_pool1d(flat, 4).squeeze(1)
    gp = hu(tuple(ref.shape), f"gp{h}{w}")
    ref.backward(gp)
    f_nhwc = nhwc(feat.detach()).to(dev)
    out = ops.pool4_fwd(f_nhwc)
    assert torch.equal(out.cpu(), ref.detach())
    dfeat = ops.pool4_relu_bwd(gp.to(dev), f_nhwc)
    assert torch.equal(dfeat.permute(0, 3, 1, 2).cpu(), feat.grad * (feat.detach() > 0))


@pytest.mark.parametrize("b,c,h,w", [(2, 32, 8, 11), (2, 32, 16, 22), (3, 32, 16, 34), (1, 8, 2, 2)])
def test_pool4_routing_codes(dev, b, c, h, w):
    """dd_pool4_fwd_idx / dd_pool4_idx_relu_bwd: routing decided in the forward (ties -> first index, all-zero windows
    -> no gradient), bit-identical to max_pool1d + its backward + the ReLU mask; shapes whose windows leave the channel
    plane are refused."""
    from driving_dirty_amd import _lib, ops
    feat = torch.relu(hu((b, c, h, w), f"cfeat{h}{w}", -1.0, 1.0))
    feat = (feat * 4).round() / 4                       # many ties and many all-zero windows
    feat.requires_grad_(True)
    ref = F.max_pool1d(feat.reshape(b, 1, -1), 4).squeeze(1)
    gp = hu(tuple(ref.shape), f"cgp{h}{w}")
    ref.backward(gp)
    f_nhwc = nhwc(feat.detach()).to(dev)
    out, codes = ops.pool4_fwd_idx(f_nhwc)
    assert torch.equal(out.cpu(), ref.detach())
    dfeat = ops.pool4_idx_relu_bwd(gp.to(dev), codes, tuple(f_nhwc.shape))
    assert torch.equal(dfeat.permute(0, 3, 1, 2).cpu(), feat.grad * (feat.detach() > 0))
    assert torch.equal(dfeat, ops.pool4_relu_bwd(gp.to(dev), f_nhwc))
    assert not ops.pool4_has_idx(5, 7, 32)
    with pytest.raises(_lib.HotpathError):
        ops.pool4_fwd_idx(torch.zeros(1, 5, 7, 32, device=dev))


@pytest.mark.parametrize("m,h1,h2,l,training", [(32, 128, 128, 64, True), (3, 16, 16, 8, True), (5, 24, 16, 8, False)])
def test_fused_encoder_tail_matches_the_separate_kernels(dev, m, h1, h2, l, training):
    """ops.EncoderTail (one launch each way) against DenseBlock -> DenseBlock -> Linear run kernel by kernel, and against
    the fp64 oracle blocks: outputs, every gradient, running statistics, num_batches_tracked."""
    from driving_dirty_amd import ops
    from driving_dirty_amd.components import DenseBlock
    from oracle.ae_parts import FcBlock

    def build():
        b1 = synth.fill_module(DenseBlock(8, h1, drop_p=0.2), seed=31)
        b2 = synth.fill_module(DenseBlock(h1, h2, drop_p=0.2), seed=32)
        fz = synth.fill_module(torch.nn.Linear(h2, l), seed=33)
        return b1, b2, fz
    lin1 = hu((m, h1), "tail_lin1")
    k1 = (hu((m, h1), "tail_k1", 0.0, 1.0) < 0.8).float()
    k2 = (hu((m, h2), "tail_k2", 0.0, 1.0) < 0.8).float()
    gz = hu((m, l), "tail_gz")
    res = []
    for fused in (True, False):
        b1, b2, fz = (t.to(dev).train(training) for t in build())
        x = lin1.clone().to(dev).requires_grad_(True)
        if fused:
            assert ops.mlp_tail_supported(m, h1, h2, l)
            z = ops.EncoderTail.apply(x, b1.fc_bn.weight, b1.fc_bn.bias, b2.fc1.weight, b2.fc1.bias, b2.fc_bn.weight, b2.fc_bn.bias,
                                      fz.weight, fz.bias, k1.to(dev), k2.to(dev), b1.fc_bn, b2.fc_bn, 1.25, 1.25)
        else:
            bn = b1.fc_bn
            y1 = ops.BnReluDrop.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, k1.to(dev), training, bn.eps, 0.1, 1.25,
                                      bn.num_batches_tracked if training else None)
            z = ops.linear(b2(y1, k2.to(dev)), fz.weight, fz.bias)
        z.backward(gz.to(dev))
        res.append({"z": z.detach(), "dx": x.grad, "bn1.g": b1.fc_bn.weight.grad, "bn1.b": b1.fc_bn.bias.grad,
                    "w2": b2.fc1.weight.grad, "b2": b2.fc1.bias.grad, "bn2.g": b2.fc_bn.weight.grad, "bn2.b": b2.fc_bn.bias.grad,
                    "wz": fz.weight.grad, "bz": fz.bias.grad, "rm1": b1.fc_bn.running_mean, "rv1": b1.fc_bn.running_var,
                    "rm2": b2.fc_bn.running_mean, "rv2": b2.fc_bn.running_var})
        assert int(b1.fc_bn.num_batches_tracked) == int(training) and int(b2.fc_bn.num_batches_tracked) == int(training)
    for k in res[0]:      # a Linear bias in front of a train-mode BatchNorm has a zero gradient: rounding noise of the weight gradient's scale
        floor = float(res[1]["w2"].abs().max()) if (k == "b2" and training) else 1e-6
        assert rel_err(res[0][k], res[1][k], floor=floor) < 1e-5, k
    # fp64 oracle of the same chain
    b1, b2, fz = build()
    o2 = FcBlock(h1, h2, drop_p=0.2).double()
    o2.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in b2.state_dict().items()})
    bn1 = torch.nn.BatchNorm1d(h1).double()
    bn1.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in b1.fc_bn.state_dict().items()})
    bn1.train(training); o2.train(training)
    x64 = lin1.double().requires_grad_(True)
    y1 = F.relu(bn1(x64)) * k1.double() * 1.25
    lin2 = F.linear(y1, o2.fc1.weight, o2.fc1.bias)
    y2 = F.relu(o2.fc_bn(lin2)) * k2.double() * 1.25
    z64 = F.linear(y2, fz.weight.double(), fz.bias.double())
    z64.backward(gz.double())
    assert rel_err(res[0]["z"], z64) < 1e-4
    assert rel_err(res[0]["dx"], x64.grad, floor=1e-6) < 1e-3
    assert not ops.mlp_tail_supported(33, 128, 128, 64) and not ops.mlp_tail_supported(32, 256, 256, 128)


def test_dense_block_counts_batches(dev):
    """BatchNorm1d.num_batches_tracked is advanced by the fused kernel (training mode only), as the module's forward does."""
    from driving_dirty_amd.components import DenseBlock
    blk = synth.fill_module(DenseBlock(8, 16, drop_p=0.2), seed=5).to(dev)
    x = hu((4, 8), "nbtx").to(dev)
    blk.train()
    blk(x)
    blk(x)
    assert int(blk.fc_bn.num_batches_tracked) == 2
    blk.eval()
    blk(x)
    assert int(blk.fc_bn.num_batches_tracked) == 2
    ref = torch.nn.BatchNorm1d(16).train()
    ref(torch.randn(4, 16)); ref(torch.randn(4, 16))
    assert int(ref.num_batches_tracked) == 2


@pytest.mark.parametrize("rows,feat,training,drop", [(3, 16, True, 0.0), (32, 128, True, 0.2), (5, 300, False, 0.2),
                                                     # wide layers (>= 65536 features): four / two features per thread (the decoder's DenseBlock)
                                                     (32, 65540, True, 0.2), (7, 65536, False, 0.2), (32, 70002, True, 0.0),
                                                     # 33-64 rows: bn_relu_drop_{fwd,bwd}_kernel<64>; 65 and up: the generic <0>; train and eval, with
                                                     # and without dropout; a wide layer on each (no multi-feature form past 32 rows)
                                                     (33, 128, True, 0.2), (33, 300, False, 0.0), (48, 300, True, 0.0), (48, 16, False, 0.2),
                                                     (64, 128, True, 0.2), (64, 300, False, 0.2), (65, 128, True, 0.2), (65, 300, False, 0.0),
                                                     (100, 16, True, 0.2), (100, 300, False, 0.2), (130, 128, True, 0.0), (130, 300, True, 0.2),
                                                     (130, 20, False, 0.2), (64, 65540, True, 0.2), (65, 65540, True, 0.2),
                                                     (64, 65536, False, 0.2), (65, 65536, False, 0.0)])
def test_bn_relu_dropout(dev, rows, feat, training, drop):
    from driving_dirty_amd import ops
    from oracle.ae_parts import FcBlock
    blk = synth.fill_module(FcBlock(8, feat, drop_p=drop), seed=9).double()
    blk.train(training)
    x = hu((rows, 8), "bnx").double()
    keep = (hu((rows, feat), "keep", 0.0, 1.0) < 0.8).double() if drop > 0 else None
    lin = F.linear(x, blk.fc1.weight, blk.fc1.bias).detach().requires_grad_(True)
    rm0, rv0 = blk.fc_bn.running_mean.clone(), blk.fc_bn.running_var.clone()
    h = F.relu(blk.fc_bn(lin))
    y_ref = h * keep / (1 - drop) if keep is not None else h
    gy = hu((rows, feat), "bngy").double()
    y_ref.backward(gy)

    lin_d = lin.detach().float().to(dev).requires_grad_(True)
    gamma = blk.fc_bn.weight.detach().float().to(dev).requires_grad_(True)
    beta = blk.fc_bn.bias.detach().float().to(dev).requires_grad_(True)
    rm, rv = rm0.float().to(dev), rv0.float().to(dev)
    y = ops.BnReluDrop.apply(lin_d, gamma, beta, rm, rv, None if keep is None else keep.float().to(dev), training,
                             blk.fc_bn.eps, 0.1, 1.0 / (1.0 - drop))
    y.backward(gy.float().to(dev))
    assert rel_err(y, y_ref) < KERNEL_TOL
    assert rel_err(lin_d.grad, lin.grad) < 10 * KERNEL_TOL
    assert rel_err(gamma.grad, blk.fc_bn.weight.grad) < 10 * KERNEL_TOL
    assert rel_err(beta.grad, blk.fc_bn.bias.grad) < 10 * KERNEL_TOL
    assert rel_err(rm, blk.fc_bn.running_mean) < KERNEL_TOL
    assert rel_err(rv, blk.fc_bn.running_var) < KERNEL_TOL


@pytest.mark.parametrize("m,n,k", [(3, 16, 704), (3, 8, 16), (32, 128, 128), (32, 64, 128), (5, 20, 8), (2, 1000, 64),
                                   (32, 128, 18816), (33, 260, 72), (64, 36, 132), (4, 640000, 8),
                                   # both sides of 64 rows: the forward and the data gradient run 64 rows per launch
                                   (63, 128, 18816), (64, 128, 18816), (65, 128, 18816), (130, 128, 18816),
                                   (63, 260, 72), (64, 260, 72), (65, 260, 72), (130, 260, 72), (65, 640000, 8)])
def test_linear_fwd_dgrad_wgrad(dev, m, n, k):
    """Skinny GEMMs (split-K forward, split-N dgrad, register wgrad) vs fp64 torch."""
    from driving_dirty_amd import ops
    x = hu((m, k), f"lx{m}{k}").double().requires_grad_(True)
    w = hu((n, k), f"lw{n}{k}", -0.2, 0.2).double().requires_grad_(True)
    b = hu((n,), f"lb{n}").double().requires_grad_(True)
    y_ref = F.linear(x, w, b)
    gy = hu((m, n), f"lg{m}{n}").double()
    y_ref.backward(gy)
    xd = x.detach().float().to(dev).requires_grad_(True)
    wd = w.detach().float().to(dev).requires_grad_(True)
    bd = b.detach().float().to(dev).requires_grad_(True)
    y = ops.linear(xd, wd, bd)
    y.backward(gy.float().to(dev))
    assert rel_err(y, y_ref) < KERNEL_TOL
    assert rel_err(xd.grad, x.grad) < KERNEL_TOL
    assert rel_err(wd.grad, w.grad) < KERNEL_TOL
    assert rel_err(bd.grad, b.grad) < KERNEL_TOL
    y2 = ops.linear(xd.detach(), wd.detach(), None)
    assert rel_err(y2, y_ref - b.detach()) < KERNEL_TOL


def test_linear_refuses_unsupported(dev):
    from driving_dirty_amd import _lib, ops
    with pytest.raises(_lib.HotpathError):
        ops.linear(torch.zeros(3, 6, device=dev), torch.zeros(8, 6, device=dev), None)      # K % 4 != 0
    with pytest.raises(_lib.HotpathError):
        ops.linear(torch.zeros(3, 8, device=dev), torch.zeros(6, 8, device=dev), None)      # N % 4 != 0
    # more than 64 rows are no longer refused: they run 64 per launch (test_linear_fwd_dgrad_wgrad at 65 and 130 rows)
    assert tuple(ops.linear(torch.zeros(65, 8, device=dev), torch.zeros(8, 8, device=dev), None).shape) == (65, 8)


@pytest.mark.parametrize("n", [7, 4096, 2 * 640000 + 3])
def test_losses(dev, n):
    from driving_dirty_amd import ops
    z = hu((n,), "z", -6.0, 6.0).double().requires_grad_(True)
    t = (hu((n,), "t", 0.0, 1.0) < 0.3).double()
    ref = F.binary_cross_entropy_with_logits(z, t)
    ref.backward()
    zd = z.detach().float().to(dev).requires_grad_(True)
    loss = ops.BceWithLogits.apply(zd, t.float().to(dev))
    (loss * 2.0).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) / float(ref.detach()) < 1e-6
    assert rel_err(zd.grad, 2.0 * z.grad) < KERNEL_TOL
    # plain loss.backward(): the upstream gradient is 1 and the device-side scaling is skipped -- same numbers, unscaled
    zu = z.detach().float().to(dev).requires_grad_(True)
    ops.BceWithLogits.apply(zu, t.float().to(dev)).backward()
    assert torch.equal(zu.grad * 2.0, zd.grad)
    l2, probs = ops.sigmoid_and_loss(zd.detach(), t.float().to(dev))
    assert rel_err(probs, torch.sigmoid(z)) < KERNEL_TOL
    # bool masks read as bytes: the same arithmetic, so the same bits
    zb = z.detach().float().to(dev).requires_grad_(True)
    lb = ops.BceWithLogits.apply(zb, t.bool().to(dev))
    (lb * 2.0).backward()
    assert torch.equal(lb.detach(), loss.detach()) and torch.equal(zb.grad, zd.grad)
    if n % 4 == 0:
        assert torch.equal(ops.sigmoid(zd.detach()), probs)
    # loss and probabilities from one pass (what the roadmap step uses): the same bits as the two separate kernels
    zp = z.detach().float().to(dev).requires_grad_(True)
    lp, pp = ops.BceWithLogitsProbs.apply(zp, t.bool().to(dev))
    (lp * 2.0).backward()
    assert torch.equal(lp.detach(), loss.detach()) and torch.equal(zp.grad, zd.grad) and torch.equal(pp, probs)
    assert not pp.requires_grad
    if n % 8 == 0:      # the masks as the collate's tuple of per-sample tensors (no stack copy): the same bits again
        zq = z.detach().float().to(dev).requires_grad_(True)
        halves = tuple(h.contiguous() for h in t.bool().to(dev).reshape(2, -1))
        lq, pq = ops.BceWithLogitsProbs.apply(zq.reshape(2, -1), halves)
        (lq * 2.0).backward()
        assert torch.equal(lq.detach(), loss.detach()) and torch.equal(zq.grad, zd.grad) and torch.equal(pq.reshape(-1), probs)
    a = hu((n,), "a").double().requires_grad_(True)
    refm = F.mse_loss(t, a)
    refm.backward()
    ad = a.detach().float().to(dev).requires_grad_(True)
    lm = ops.MseLoss.apply(ad, t.float().to(dev))
    lm.backward()
    assert abs(float(lm.detach()) - float(refm.detach())) / float(refm.detach()) < 1e-6
    assert rel_err(ad.grad, a.grad) < KERNEL_TOL


def test_adam_matches_torch(dev):
    from driving_dirty_amd import ops
    n = 10007
    p0, g = hu((n,), "p"), hu((n,), "g", -0.1, 0.1)
    p_ref = p0.clone().double().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=1e-3)
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for step in range(1, 4):
        gs = g * step
        p_ref.grad = gs.double()
        opt.step()
        ops.adam_step_flat(p, gs.to(dev), m, v, 1e-3, 0.9, 0.999, 1e-8, step)
    assert rel_err(p, p_ref) < 1e-6


def test_adam_multi_tensor_matches_torch(dev):
    """dd_adam_step_multi: the model's small tensors in one launch (ragged sizes, more tensors than one table holds)."""
    from driving_dirty_amd import ops
    sizes = [1, 3, 32, 255, 256, 257, 864, 4097] + [7 + i for i in range(50)]
    ps = [hu((n,), f"p{i}") for i, n in enumerate(sizes)]
    gs = [hu((n,), f"g{i}", -0.1, 0.1) for i, n in enumerate(sizes)]
    refs = [p.clone().double().requires_grad_(True) for p in ps]
    opt = torch.optim.Adam(refs, lr=1e-3)
    quads = [(p.clone().to(dev), torch.empty(p.shape, device=dev), torch.zeros(p.shape, device=dev), torch.zeros(p.shape, device=dev))
             for p in ps]
    for step in range(1, 4):
        for r, q, g in zip(refs, quads, gs):
            r.grad = (g * step).double() * 0.5
            q[1].copy_(g * step)
        opt.step()
        ops.adam_step_multi(quads, 1e-3, 0.9, 0.999, 1e-8, step, grad_scale=0.5)
    for r, q in zip(refs, quads):
        assert rel_err(q[0], r) < 1e-6


@pytest.mark.parametrize("scale_on_device", (False, True))
def test_adam_multi_checks_the_whole_table_before_the_first_launch(dev, scale_on_device):
    """49 tensors, one more than a table holds, the last one empty: refused on the host, and the 48 tensors of the first table keep
    their bits -- parameters, moments and gradients.  (Checked table by table, the first 48 were updated before the refusal.)"""
    from driving_dirty_amd import ops
    from driving_dirty_amd._lib import HotpathError
    host = [tuple(hu((4,), f"{k}{i}", lo, hi) for k, lo, hi in (("p", -1.0, 1.0), ("g", -0.1, 0.1), ("m", -0.05, 0.05), ("v", 1e-4, 1e-2)))
            for i in range(48)]
    quads = [tuple(t.to(dev) for t in quad) for quad in host] + [tuple(torch.empty(0, device=dev) for _ in "pgmv")]
    scale = torch.tensor([0.5], device=dev) if scale_on_device else 0.5
    with pytest.raises(HotpathError, match="adam_multi: tensor 48: NULL pointer or bad size"):
        ops.adam_step_multi(quads, 1e-3, 0.9, 0.999, 1e-8, 1, grad_scale=scale)
    torch.cuda.synchronize()
    for before, after in zip(host, quads):
        for b, a in zip(before, after):
            assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))


def _grad_floor(g, key):
    """A Linear bias in front of a train-mode BatchNorm has an exactly-zero gradient; in fp32 (the reference's
    own fp32 run included: 3.6e-5 in the fixture) it is rounding noise of the layer's gradient scale, so it is
    judged against the peak of that layer's WEIGHT gradient rather than against ~1e-15."""
    if key.endswith(".fc1.bias"):
        wk = key[:-len("bias")] + "weight"
        for cand in (f"grad.{wk}_f64", f"gradsamp.{wk}_f64"):
            if cand in g.files:
                return float(np.abs(g[cand]).max())
    return 1e-30


def _budget(g, key):
    """Tolerance for one tensor of the B = 2 EDGE-CASE fixture: 1e-3 of its peak (north_star), or twice the deviation the
    REFERENCE's own fp32 run shows from its fp64 run, whichever is larger.  Through a train-mode BatchNorm1d over TWO rows the
    normalised values are +-1 whatever the inputs: the gradient that reaches everything upstream of it is an eps = 1e-5 effect,
    a difference of nearly equal numbers (the reference's fp32 gradients are up to 2e-2 of peak off their fp64 values there).
    The well-conditioned checks of this path are at the headline batch: tests/test_gpu_round2.py (B = 32 fixture; the fp64
    oracle on the product's own ReLU / max-pool branch within 2e-4, no budget)."""
    a, b = g[key + "_f64"], g[key + "_f32"]
    ref_dev = float(np.abs(a - b).max() / max(np.abs(a).max(), 1e-30))
    return max(CHAIN_TOL, 2.0 * ref_dev) if ref_dev < 1.0 else CHAIN_TOL


def _tiny_encoder(dev):
    from driving_dirty_amd.components import Encoder
    enc = synth.fill_module(Encoder(16, 8, 3, 16, 22), seed=1).to(dev)
    enc.fc1.drop_p = enc.fc2.drop_p = 0.0
    return enc


def test_tiny_encoder_against_reference_golden(dev, golden):
    """Encoder(16,8,3,16,22) end to end vs the fixture captured from the reference's own module (fp64 truth)."""
    g = golden("tiny_encoder")
    enc = _tiny_encoder(dev)
    x = synth.hash_uniform((3, 3, 16, 22), synth.key_salt("tiny_x"), 0.0, 1.0).to(dev)
    wz = synth.hash_uniform((3, 8), synth.key_salt("tiny_wz")).to(dev)
    enc.train()
    z = enc(x)
    (z * wz).sum().backward()
    assert rel_err(z, torch.from_numpy(g["z_f64"])) < CHAIN_TOL
    for k, p in enc.named_parameters():
        assert rel_err(p.grad, torch.from_numpy(g[f"grad.{k}_f64"]), floor=_grad_floor(g, k)) < CHAIN_TOL, k
    for k, b in enc.named_buffers():
        assert rel_err(b.float(), torch.from_numpy(g[f"buf.{k}_f64"])) < CHAIN_TOL, k
    enc.zero_grad()
    enc.c3_only = True
    feat = enc(x)
    assert feat.shape == (3, 32, 8, 11)
    wf = synth.hash_uniform(tuple(feat.shape), synth.key_salt("tiny_wf")).to(dev)
    (feat * wf).sum().backward()
    assert rel_err(feat, torch.from_numpy(g["feat_f64"])) < KERNEL_TOL
    for k in ("c1.weight", "c1.bias", "c2.weight", "c2.bias", "c3.weight", "c3.bias"):
        assert rel_err(dict(enc.named_parameters())[k].grad, torch.from_numpy(g[f"featgrad.{k}_f64"])) < CHAIN_TOL, k
    enc.c3_only = False
    enc.eval()
    assert rel_err(enc(x), torch.from_numpy(g["z_eval_f64"])) < CHAIN_TOL


def _samp(t, idx):
    return t.detach().reshape(-1)[torch.from_numpy(idx).to(t.device)]


def test_full_size_roadmap_against_reference_golden(dev, golden):
    """Config-2 shapes (6x3x256x306 -> 800x800) at B = 2, the ill-conditioned edge case (see _budget): loss, z, logits and
    every gradient vs the fixture.  The headline batch is checked in tests/test_gpu_round2.py."""
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    g = golden("full_roadmap")
    ae = BasicAE(Namespace(hidden_dim=128, latent_dim=64))
    synth.fill_module(ae.encoder, seed=3)
    hp = Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500)
    model = RoadMapBCE(hp)
    synth.fill_module(model.fc1, seed=4)
    model = model.to(dev)
    model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0
    views = synth.camera_batch(2, seed=3).to(dev)
    road = synth.road_maps(2, seed=3).to(dev)
    batch = (tuple(views), (None, None), tuple(road))
    out = model.training_step(batch, 0)
    out["loss"].backward()
    assert abs(float(out["loss"]) - float(g["loss_f64"])) / float(g["loss_f64"]) < 1e-5
    logits, probs = model(batch[0])
    assert rel_err(_samp(logits, g["logits_idx"]), torch.from_numpy(g["logits_samp_f64"])) < _budget(g, "logits_samp")
    assert abs(float(logits.double().sum()) - float(g["logits_sum_f64"])) / abs(float(g["logits_sum_f64"])) < CHAIN_TOL
    named = {("head." + k): p for k, p in model.fc1.named_parameters()}
    named.update(dict(model.ae.encoder.named_parameters()))
    for k, p in named.items():
        key = f"grad.{k}" if f"grad.{k}_f64" in g.files else f"gradsamp.{k}"
        budget = _budget(g, key)
        if key.startswith("grad."):
            assert rel_err(p.grad, torch.from_numpy(g[key + "_f64"]), floor=_grad_floor(g, k)) < budget, k
        else:
            assert rel_err(_samp(p.grad, g[f"gradidx.{k}"]), torch.from_numpy(g[key + "_f64"])) < budget, k
        s = g[f"gradsum.{k}_f64"]
        if s[1] > 1e-6:     # checksum over the WHOLE tensor (the 481 MB fc1 gradient is only sampled above)
            assert abs(float(p.grad.double().abs().sum()) - s[1]) / s[1] < budget, k
    model.ae.encoder.c3_only = True
    with torch.no_grad():
        feat = model.ae.encoder.forward_nhwc4(__import__("driving_dirty_amd.ops", fromlist=["ops"]).stitch6(views)[0])
    assert rel_err(_samp(feat.contiguous(), g["feat_idx"]), torch.from_numpy(g["feat_samp_f64"])) < KERNEL_TOL
    s = g["feat_sum_f64"]
    assert abs(float(feat.double().abs().sum()) - s[1]) / s[1] < 1e-5


def test_adam_overlapped_with_backward_is_identical(dev):
    """HipAdam.overlap_with_backward (optimizer pass of the big tensors on a side stream, from autograd hooks)
    must leave exactly the same parameters as the plain post-backward step."""
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.optim import HipAdam
    from driving_dirty_amd.roadmap import RoadMapBCE

    class Pieces:
        """Stands in for ddp.GradSync on one process: every big gradient 'arrives' in pieces of 1000 elements."""
        class Work:
            def wait(self):
                pass

        def pieces(self, p):
            n = p.numel()
            return [(self.Work(), o, min(1000, n - o)) for o in range(0, n, 1000)] if n >= 1000 else None

        def shards(self, p):      # all-reduce mode: nothing travels as shards
            return None

        def wait_param(self, p):
            pass

    def run(overlap):
        ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132, output_height=16, output_width=22))
        m = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500))
        synth.fill_module(m, seed=23)
        m = m.to(dev)
        m.ae.encoder.fc1.drop_p = m.ae.encoder.fc2.drop_p = 0.0
        opt = HipAdam(m.parameters(), lr=1e-2)
        if overlap:      # 2: the per-piece path the data-parallel run takes (update of piece k while piece k+1 is on the links)
            opt.overlap_with_backward(big_numel=1000, grad_sync=Pieces() if overlap == 2 else None)
        views = synth.camera_batch(3, 16, 22, seed=23).to(dev)
        road = synth.road_maps(3, seed=23).to(dev)
        for i in range(3):
            m.zero_grad(set_to_none=True)
            m.training_step((tuple(views), None, tuple(road)), i)["loss"].backward()
            opt.step()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.state_dict().items()}

    a, b, c = run(0), run(1), run(2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], c[k]), k


def test_threat_score_and_validation_step(dev):
    """compute_ts_road_map (helper.py:74-77) fused on the device, and RoadMapBCE.validation_step's outputs."""
    from driving_dirty_amd import ops
    from oracle import steps
    t = (hu((3, 800, 800), "tst", 0.0, 1.0) < 0.3).float()
    p = hu((3, 800, 800), "tsp", 0.0, 1.0)
    assert abs(float(ops.threat_score(t.to(dev), p.to(dev))) - float(steps.threat_score(t.double(), p.double()))) < 1e-6
    assert abs(float(ops.threat_score(t.to(dev), p.to(dev), round_b=True)) - float(steps.threat_score(t.double(), p.double().round()))) < 1e-6
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132, output_height=16, output_width=22))
    m = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500)).to(dev)
    views = synth.camera_batch(3, 16, 22, seed=31).to(dev)
    road = synth.road_maps(3, seed=31).to(dev)
    out = m.validation_step((tuple(views), None, tuple(road)), 0)
    agg = m.validation_epoch_end([out, out])
    assert set(out) == {"val_loss", "val_ts_rounded", "val_ts"} and set(agg) == {"val_loss", "log"}
    assert 0.0 <= float(out["val_ts"]) <= 1.0


def test_stitch6_uint8_pipeline(dev):
    """uint8 HWC frames -> wide NHWC4 float: equals ToTensor (/255) followed by the reference stitch."""
    from driving_dirty_amd import ops
    from oracle import steps
    frames = (hu((2, 6, 9, 13, 3), "u8", 0.0, 256.0)).clamp(0, 255).to(torch.uint8)
    ref = steps.wide_stitch(frames.permute(0, 1, 4, 2, 3).float() / 255.0)
    out = ops.stitch6_u8(frames.to(dev))
    assert torch.allclose(out[..., :3].permute(0, 3, 1, 2).cpu(), ref, rtol=0, atol=1e-7)
    assert float(out[..., 3].abs().max()) == 0.0


def test_cu_budget_never_changes_results(dev):
    """dd_set_cu_budget shrinks the resident grids (room for RCCL beside the conv backward): same numbers."""
    from driving_dirty_amd import _lib, ops
    b, h, w = 2, 40, 300
    d = ops.conv_desc(b, h, w, 32, 1)
    x = hu((b, h, w, 32), "cux").to(dev)
    wt = hu((32, 32, 3, 3), "cuw", -0.2, 0.2).to(dev)
    bias = hu((32,), "cub").to(dev)
    g = hu((b, h, w, 32), "cug").to(dev)
    outs = []
    try:
        for budget in (256, 7):
            _lib.check(_lib.lib().dd_set_cu_budget(budget), "budget")
            y = ops.conv_fwd(x, ops.conv_pack(wt, d, 0), bias, d)
            dx = ops.conv_dgrad(g, ops.conv_pack(wt, d, 1), x, d)
            dw, db = ops.conv_wgrad(x, g, d)
            outs.append((y, dx, dw, db))
    finally:
        _lib.lib().dd_set_cu_budget(256)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert rel_err(outs[1][2], outs[0][2]) < 1e-5 and rel_err(outs[1][3], outs[0][3]) < 1e-5


@pytest.mark.parametrize("b,c,cs,h,w", [(2, 64, 64, 13, 17), (1, 3, 4, 5, 9), (3, 32, 32, 8, 64), (2, 5, 8, 7, 11), (1, 64, 64, 128, 153),
                                        (2, 96, 96, 6, 6), (1, 1, 8, 1, 1)])
def test_layout_round_trip(dev, b, c, cs, h, w):
    """NCHW <-> NHWC(c_store): exact copies, zero padding channels, both the tiled (8..64 stored channels) and the
    element-wise kernels."""
    from driving_dirty_amd import ops
    x = hu((b, c, h, w), f"lay{c}{h}{w}").to(dev)
    y = ops.nchw_to_nhwc(x, cs)
    assert torch.equal(y[..., :c], x.permute(0, 2, 3, 1))
    if cs > c:
        assert float(y[..., c:].abs().max()) == 0.0
    assert torch.equal(ops.nhwc_to_nchw(y, c), x)


def test_encoder_conv_stack_modes_agree(dev):
    """The encoder conv stack with c2 on the direct kernels, on Winograd F(2,3) along x and on F(2x2,3x3): same pooled
    feature and the same six parameter gradients up to summation order."""
    from driving_dirty_amd import ops
    b, h, w = 2, 18, 70
    x4 = hu((b, h, w, 4), "modes_x", 0.0, 1.0)
    x4[..., 3] = 0
    x4 = x4.to(dev)
    ws = [hu((32, 3, 3, 3), "mw1", -0.3, 0.3), hu((32,), "mb1", -0.1, 0.1), hu((32, 32, 3, 3), "mw2", -0.1, 0.1), hu((32,), "mb2", -0.1, 0.1),
          hu((32, 32, 3, 3), "mw3", -0.1, 0.1), hu((32,), "mb3", -0.1, 0.1)]
    gp = None
    results = []
    saved = (ops.WINOGRAD, ops.WINOGRAD_2D)
    try:
        for wino, wino2 in ((False, False), (True, False), (True, True)):
            ops.WINOGRAD, ops.WINOGRAD_2D = wino, wino2
            params = [t.clone().to(dev).requires_grad_(True) for t in ws]
            pooled = ops.EncoderConvStack.apply(x4, *params, 1, 0)
            if gp is None:
                gp = hu(tuple(pooled.shape), "modes_g").to(dev)
            pooled.backward(gp)
            results.append((pooled.detach(), [p.grad for p in params]))
    finally:
        ops.WINOGRAD, ops.WINOGRAD_2D = saved
    ref_p, ref_g = results[0]
    for pooled, grads in results[1:]:
        assert rel_err(pooled, ref_p.double()) < 1e-5
        for g, r in zip(grads, ref_g):
            assert rel_err(g, r.double()) < 1e-4
