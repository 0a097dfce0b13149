"""bf16 mixed-precision conv stack (BASELINE config 5) over the C ABI's ``dd_*bf16*`` entry points.

Activations / activation gradients: NHWC ``torch.bfloat16`` tensors (the ABI sees their raw uint16 storage);
weights, biases and their gradients: fp32.  Rounding happens exactly once, in the kernel that writes a tensor.
"""
import torch

from . import _lib, ops
from ._lib import call, size
from .ops import PACK_DGRAD_S1, PACK_DGRAD_S2, PACK_FWD, conv_desc, conv_out


def _bf(t, name, shape=None):
    return _lib.dev(t, name, shape, torch.bfloat16)


def stitch6_bf16(views):
    """[B,6,3,H,W] fp32 -> wide NHWC4 bf16 [B,H,6W,4] (view order [0,1,2,5,4,3], channel 3 zero)."""
    return ops.wide_call("dd_stitch6_bf16", views, *ops.stacked_views(views, "stitch6_bf16"), views.device)[0]


def stitch6_bf16_samples(samples):
    """Tuple of B per-sample [6,3,H,W] fp32 tensors (the reference's collate, helper.py:22-23) -> wide NHWC4 bf16, no stack copy."""
    return ops.wide_image(tuple(samples), "bf16")


def stitch6_bf16_u8(sample):
    """uint8 frames ([B,6,H,W,3] or a tuple of [6,H,W,3]) -> wide NHWC4 bf16: /255 (true division) and the bf16 rounding fused with
    the gather -- the values ``stitch6_bf16(frames.permute(..).float() / 255)`` gives."""
    table, b, h, w, dev, _keep = ops.u8_table(sample, "stitch6_bf16_u8")
    return ops.wide_call("dd_stitch6_bf16_u8_ptrs", table, b, h, w, dev)[0]


def to_bf16(t):
    ops._dev(t, "t")
    if t.numel() % 4:
        raise _lib.HotpathError("to_bf16: element count must be a multiple of 4")
    out = torch.empty(t.shape, device=t.device, dtype=torch.bfloat16)
    call("dd_f32_to_bf16", t, out, t.numel())
    return out


def to_f32(t):
    _bf(t, "t")
    if t.numel() % 4:
        raise _lib.HotpathError("to_f32: element count must be a multiple of 4")
    out = torch.empty(t.shape, device=t.device, dtype=torch.float32)
    call("dd_bf16_to_f32", t, out, t.numel())
    return out


def conv_pack(weight, desc, kind):
    ops._dev(weight, "weight", (32, desc.cin_real, 3, 3))
    n = size("dd_conv_bf16_packed_elems", desc)
    packed = torch.empty(n, device=weight.device, dtype=torch.bfloat16)
    call("dd_conv_bf16_pack", weight, desc, kind, packed)
    return packed


def conv_fwd(x, packed, bias, desc, want_bits=True):
    """bf16(relu(conv(x) + bias)) and (optionally) the ReLU signs as one uint32 per pixel."""
    ho, wo = conv_out(desc.height, desc.stride), conv_out(desc.width, desc.stride)
    _bf(x, "x", (desc.batch, desc.height, desc.width, desc.cin_store))
    _bf(packed, "packed")
    ops._dev(bias, "bias", (32,))
    y = torch.empty((desc.batch, ho, wo, 32), device=x.device, dtype=torch.bfloat16)
    bits = torch.empty((desc.batch, ho, wo), device=x.device, dtype=torch.int32) if want_bits else None
    call("dd_conv_bf16_fwd", x, packed, bias, y, bits, desc)
    return y, bits


def conv_dgrad(dy, packed_dgrad, bits, desc):
    ho, wo = conv_out(desc.height, desc.stride), conv_out(desc.width, desc.stride)
    _bf(dy, "dy", (desc.batch, ho, wo, 32))
    _bf(packed_dgrad, "packed")
    ops._relu_bits(bits, desc, "conv_bf16_dgrad")
    dx = torch.empty((desc.batch, desc.height, desc.width, 32), device=dy.device, dtype=torch.bfloat16)
    call("dd_conv_bf16_dgrad", dy, packed_dgrad, bits, dx, desc)
    return dx


def conv_wgrad(x, dy, desc):
    ho, wo = conv_out(desc.height, desc.stride), conv_out(desc.width, desc.stride)
    _bf(x, "x", (desc.batch, desc.height, desc.width, desc.cin_store))
    _bf(dy, "dy", (desc.batch, ho, wo, 32))
    nbytes = size("dd_conv_bf16_wgrad_workspace_bytes", desc)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    dw = torch.empty((32, desc.cin_real, 3, 3), device=x.device, dtype=torch.float32)
    db = torch.empty(32, device=x.device, dtype=torch.float32)
    call("dd_conv_bf16_wgrad", x, dy, dw, db, desc, ws, nbytes)
    return dw, db


_POOL4_BF16 = (torch.bfloat16, {"fwd": "dd_pool4_bf16_fwd", "relu_bwd": "dd_pool4_relu_bf16_bwd", "idx_elems": "dd_pool4_bf16_idx_elems",
                                 "fwd_idx": "dd_pool4_bf16_fwd_idx", "idx_relu_bwd": "dd_pool4_idx_relu_bf16_bwd"})      # bodies: ops._pool4_*


def pool4_fwd(feat):
    return ops._pool4_fwd(_POOL4_BF16, feat)


def pool4_relu_bwd(dpooled, feat):
    return ops._pool4_relu_bwd(_POOL4_BF16, dpooled, feat)


def pool4_has_idx(h, w, c):
    """Whether the tiled pool with routing codes takes this feature map (C == 32, H*W % 4 == 0)."""
    return c == 32 and (h * w) % 4 == 0


def pool4_fwd_idx(feat):
    """pooled, codes: max_pool1d(4) + the backward's routing (dd_pool4_bf16_fwd_idx)."""
    return ops._pool4_fwd_idx(_POOL4_BF16, feat)


def pool4_idx_relu_bwd(dpooled, idx, shape):
    return ops._pool4_idx_relu_bwd(_POOL4_BF16, dpooled, idx, shape)


class EncoderConvStackBf16(torch.autograd.Function):
    """c1 -> ReLU -> c2 -> ReLU -> c3 (stride 2) -> ReLU -> NCHW-order max_pool1d(4), bf16 operands / fp32 accumulation.

    Reference arithmetic: Encoder.forward, src/autoencoder/components.py:41-47 (the reference itself is fp32 only; the
    rounding points are those of torch autocast: every conv output is rounded to bf16 once).
    forward(x4 bf16 [B,H,W,4], w1,b1,w2,b2,w3,b3 fp32, pool) -> pooled fp32 [B, 32*Ho*Wo/4], or (pool = False: the ``c3_only``
    exit, components.py:44-45) the bf16-rounded c3 feature as an fp32 NHWC tensor [B,Ho,Wo,32] for the fp32 box heads.
    """

    @staticmethod
    def forward(ctx, x4, w1, b1, w2, b2, w3, b3, pool=True):
        b, h, w, _ = x4.shape
        d1, d2, d3 = conv_desc(b, h, w, 3, 1), conv_desc(b, h, w, 32, 1), conv_desc(b, h, w, 32, 2)
        a1, s1 = conv_fwd(x4, conv_pack(w1, d1, PACK_FWD), b1, d1)
        a2, s2 = conv_fwd(a1, conv_pack(w2, d2, PACK_FWD), b2, d2)
        a3, _ = conv_fwd(a2, conv_pack(w3, d3, PACK_FWD), b3, d3, want_bits=False)
        # the backward's operand images are packed here (see ops.EncoderConvStack.forward)
        need = ctx.needs_input_grad
        p2d = p3d = torch.empty(0, device=x4.device, dtype=torch.bfloat16)
        if need[1] or need[2] or need[3] or need[4]:
            p3d = conv_pack(w3, d3, PACK_DGRAD_S2)
        if need[1] or need[2]:
            p2d = conv_pack(w2, d2, PACK_DGRAD_S1)
        ctx.pool = bool(pool)
        ctx.a3_shape = tuple(a3.shape)
        ctx.pool_idx = ctx.pool and pool4_has_idx(*a3.shape[1:])
        if ctx.pool_idx:      # the pool's backward runs from 30 MB of routing codes: the 0.48 GB feature is neither kept nor read again
            out, codes = pool4_fwd_idx(a3)
            ctx.save_for_backward(x4, a1, a2, codes, p2d, p3d, s1, s2)
            return out
        ctx.save_for_backward(x4, a1, a2, a3, p2d, p3d, s1, s2)
        return pool4_fwd(a3) if pool else to_f32(a3)

    @staticmethod
    def backward(ctx, grad_out):
        x4, a1, a2, a3, p2d, p3d, s1, s2 = ctx.saved_tensors
        b, h, w, _ = x4.shape
        d1, d2, d3 = conv_desc(b, h, w, 3, 1), conv_desc(b, h, w, 32, 1), conv_desc(b, h, w, 32, 2)
        if ctx.pool_idx:
            g3 = pool4_idx_relu_bwd(grad_out.contiguous(), a3, ctx.a3_shape)      # a3 holds the routing codes here
        elif ctx.pool:
            g3 = pool4_relu_bwd(grad_out.contiguous(), a3)
        else:      # feature exit: ReLU mask in fp32, then the one rounding to bf16 the contract prescribes for a pre-activation gradient
            g3 = to_bf16(ops.relu_bwd(grad_out.contiguous(), to_f32(a3)))
        need = ctx.needs_input_grad
        dw3, db3 = conv_wgrad(a2, g3, d3) if (need[5] or need[6]) else (None, None)
        dw2 = db2 = dw1 = db1 = None
        if need[1] or need[2] or need[3] or need[4]:
            g2 = conv_dgrad(g3, p3d, s2, d3)
            del g3
            for obs in ops.BACKWARD_OBSERVERS:
                obs.backward_phase1()
            if need[3] or need[4]:
                dw2, db2 = conv_wgrad(a1, g2, d2)
            if need[1] or need[2]:
                g1 = conv_dgrad(g2, p2d, s1, d2)
                del g2
                dw1, db1 = conv_wgrad(x4, g1, d1)
        return None, dw1, db1, dw2, db2, dw3, db3, None


def encoder_conv_stack(x4, c1, c2, c3, pool=True):
    return EncoderConvStackBf16.apply(x4, c1.weight, c1.bias, c2.weight, c2.bias, c3.weight, c3.bias, pool)


# ------------------------------------------------------------------------------------------------ BasicAE pre-training in bf16
def stitch6_bf16_masked(sample, mask_slot=-1, want_target=False):
    """The masked-view task of BasicAE (autoencoder.py:59-73) on the bf16 image, in one pass: wide NHWC4 bf16 with wide slot
    ``mask_slot`` blanked and, with ``want_target``, that view as fp32 [B,3,H,W] (the fp32 path's target bit for bit).  ``sample``:
    fp32 [B,6,3,H,W], the collate's tuple of fp32 [6,3,H,W], or uint8 frames ([B,6,H,W,3] or a tuple of [6,H,W,3]).  Always the
    ``_masked`` entry point of the form, also for ``mask_slot`` -1."""
    slot = ops.mask_arg(mask_slot, "stitch6_bf16_masked")
    form, src, b, h, w, dev, _keep = ops.camera_source(sample, "stitch6_bf16_masked")
    out, _, tgt = ops.wide_call(ops.WIDE_ENTRIES["bf16", form][1], src, b, h, w, dev, slot, want_target)
    return (out, tgt) if want_target else out


def _dec_ws(layer, b, dh, dw, dev):
    n = size("dd_dec_bf16_wgrad_workspace_bytes", layer, b, dh, dw)
    return torch.empty(n, device=dev, dtype=torch.uint8), n


def _bits(t, shape, who):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise _lib.HotpathError(f"{who}: relu_bits must be a contiguous int32 {tuple(shape)} device tensor")
    return t


def dec_split64(h, dh, dw):
    """fc2's fp32 output [B, 64*dh*dw] (NCHW-flat) -> dc1's input as two bf16 NHWC images [B,dh,dw,32] (channels 0-31, 32-63)."""
    b = h.shape[0]
    ops._dev(h, "h", (b, 64 * dh * dw))
    lo = torch.empty((b, dh, dw, 32), device=h.device, dtype=torch.bfloat16)
    hi = torch.empty_like(lo)
    call("dd_dec_bf16_split64", h, lo, hi, b, dh, dw)
    return lo, hi


def dec_merge64(lo, hi):
    """Two bf16 NHWC halves [B,dh,dw,32] -> fp32 [B, 64*dh*dw] in fc2's NCHW-flat layout."""
    b, dh, dw, _ = lo.shape
    _bf(lo, "lo", (b, dh, dw, 32))
    _bf(hi, "hi", (b, dh, dw, 32))
    gh = torch.empty((b, 64 * dh * dw), device=lo.device, dtype=torch.float32)
    call("dd_dec_bf16_merge64", lo, hi, gh, b, dh, dw)
    return gh


def dec_dc1_fwd(x_lo, x_hi, w1, b1):
    """dc1 on the bf16 matrix cores: a1 bf16 [B,dh,dw,32] = bf16(relu(dc1(x) + b1)) and its ReLU sign words [B,dh,dw]."""
    b, dh, dw, _ = x_lo.shape
    _bf(x_lo, "x_lo", (b, dh, dw, 32))
    _bf(x_hi, "x_hi", (b, dh, dw, 32))
    ops._dev(w1, "w1", (64, 32, 3, 3))
    ops._dev(b1, "b1", (32,))
    a1 = torch.empty((b, dh, dw, 32), device=x_lo.device, dtype=torch.bfloat16)
    bits = torch.empty((b, dh, dw), device=x_lo.device, dtype=torch.int32)
    call("dd_dec_bf16_dc1_fwd", x_lo, x_hi, w1, b1, a1, bits, b, dh, dw)
    return a1, bits


def dec_dc1_bwd(x_lo, x_hi, g1, w1, want_dx=True):
    """dc1's backward from its bf16 pre-activation gradient g1 [B,dh,dw,32]: (gh fp32 [B, 64*dh*dw] bf16-rounded or None, dw1, db1).
    The equivalent convolution Wc = _as_conv(w1) [32,64,3,3] splits into two 32 -> 32 layers on the input-channel halves, each the
    encoder's c2 layer: the weight gradient is two fp32 sums (dd_conv_bf16_wgrad), the data gradient two bf16 outputs of disjoint
    channels (dd_conv_bf16_dgrad with no ReLU mask) -- the same values the 64-channel layer gives."""
    b, dh, dw, _ = g1.shape
    d = conv_desc(b, dh, dw, 32, 1)
    dlo, db1 = conv_wgrad(x_lo, g1, d)
    dhi, _ = conv_wgrad(x_hi, g1, d)
    dw1 = _as_conv(torch.cat((dlo, dhi), dim=1))              # [32,64,3,3] conv layout -> the ConvTranspose2d weight [64,32,3,3]
    gh = None
    if want_dx:
        wc = _as_conv(w1)
        ones = torch.full((b, dh, dw), -1, device=g1.device, dtype=torch.int32)
        glo = conv_dgrad(g1, conv_pack(wc[:, :32].contiguous(), d, PACK_DGRAD_S1), ones, d)
        ghi = conv_dgrad(g1, conv_pack(wc[:, 32:].contiguous(), d, PACK_DGRAD_S1), ones, d)
        gh = dec_merge64(glo, ghi)
    return gh, dw1, db1


def dec_dc34_fwd(a2, w3, b3, w4, b4):
    """a2 bf16 [B,dh,dw,32] -> a3 bf16 [B,2dh,2dw,32] = bf16(relu(dc3(a2))), y_hat fp32 [B,3,2dh,2dw] = bf16(dc4(a3))."""
    b, dh, dw, _ = a2.shape
    _bf(a2, "a2", (b, dh, dw, 32))
    ops._dev(w3, "w3", (32, 32, 2, 2))
    ops._dev(b3, "b3", (32,))
    ops._dev(w4, "w4", (32, 3, 1, 1))
    ops._dev(b4, "b4", (3,))
    a3 = torch.empty((b, 2 * dh, 2 * dw, 32), device=a2.device, dtype=torch.bfloat16)
    y = torch.empty((b, 3, 2 * dh, 2 * dw), device=a2.device, dtype=torch.float32)
    call("dd_dec_bf16_dc34_fwd", a2, w3, b3, w4, b4, a3, y, b, dh, dw)
    return a3, y


def dec_dc4_bwd(gy, a3, w4):
    """-> g3 bf16 (dc3's pre-activation gradient), dw4 [32,3,1,1], db4 [3]."""
    b, ho, wo, _ = a3.shape
    if ho % 2 or wo % 2:
        raise _lib.HotpathError(f"dec_dc4_bwd: a3 {tuple(a3.shape)} is not on a doubled grid")
    _bf(a3, "a3", (b, ho, wo, 32))
    ops._dev(gy, "gy", (b, 3, ho, wo))
    ops._dev(w4, "w4", (32, 3, 1, 1))
    ws, n = _dec_ws(4, b, ho // 2, wo // 2, a3.device)
    g3 = torch.empty_like(a3)
    dwt = torch.empty((32, 3, 1, 1), device=a3.device, dtype=torch.float32)
    db = torch.empty(3, device=a3.device, dtype=torch.float32)
    call("dd_dec_bf16_dc4_bwd", gy, a3, w4, g3, dwt, db, b, ho // 2, wo // 2, ws, n)
    return g3, dwt, db


def dec_dc3_dgrad(g3, w3, bits2):
    b, ho, wo, _ = g3.shape
    if ho % 2 or wo % 2:
        raise _lib.HotpathError(f"dec_dc3_dgrad: g3 {tuple(g3.shape)} is not on a doubled grid")
    dh, dw = ho // 2, wo // 2
    _bf(g3, "g3", (b, ho, wo, 32))
    ops._dev(w3, "w3", (32, 32, 2, 2))
    _bits(bits2, (b, dh, dw), "dec_dc3_dgrad")
    g2 = torch.empty((b, dh, dw, 32), device=g3.device, dtype=torch.bfloat16)
    call("dd_dec_bf16_dc3_dgrad", g3, w3, bits2, g2, b, dh, dw)
    return g2


def dec_dc3_wgrad(a2, g3):
    b, dh, dw, _ = a2.shape
    _bf(a2, "a2", (b, dh, dw, 32))
    _bf(g3, "g3", (b, 2 * dh, 2 * dw, 32))
    ws, n = _dec_ws(3, b, dh, dw, a2.device)
    dwt = torch.empty((32, 32, 2, 2), device=a2.device, dtype=torch.float32)
    db = torch.empty(32, device=a2.device, dtype=torch.float32)
    call("dd_dec_bf16_dc3_wgrad", a2, g3, dwt, db, b, dh, dw, ws, n)
    return dwt, db


def _as_conv(w):
    """ConvTranspose2d weight [Cin,Cout,3,3] <-> the Conv2d weight [Cout,Cin,3,3] of the same stride-1 map (heads.DecoderConvStack._as_conv)."""
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


class DecoderConvStackBf16(torch.autograd.Function):
    """heads.DecoderConvStack in bf16 mixed precision: same arguments, same fp32 NCHW-flat input [B, 64*dh*dw] and fp32 NCHW output
    [B,3,2dh,2dw].  dc1 k3 p1 +ReLU, dc2 k3 p1 +ReLU, dc3 k2 s2 +ReLU, dc4 k1 (reference components.py:88-92).

    Contract ("torch autocast equivalent", as oracle/bf16_parts.py states it for the encoder): every conv reads bf16-rounded inputs and
    weights, accumulates in fp32 and rounds its output to bf16 once, after bias and ReLU; dc4's output y_hat is rounded to bf16 once and
    returned as fp32.  Backward: dL/dy_hat and every pre-activation gradient are rounded to bf16 once, weight / bias gradients are fp32
    sums of bf16 products, and the gradient handed back to fc2 is the bf16-rounded dL/d(input) in fc2's fp32 NCHW-flat layout.
    Activations between the layers are NHWC bf16.  dc1's input is kept as two 32-channel bf16 halves: its forward is an MFMA kernel
    of csrc/decoder_bf16.hip, its gradients and all of dc2 run on the encoder's bf16 c2 kernels (dd_conv_bf16_*), dc3 + dc4 on
    csrc/decoder_bf16.hip.
    """

    @staticmethod
    def forward(ctx, h, dh, dw, w1, b1, w2, b2, w3, b3, w4, b4):
        b = h.shape[0]
        x_lo, x_hi = dec_split64(h.contiguous(), dh, dw)
        a1, s1 = dec_dc1_fwd(x_lo, x_hi, w1, b1)
        d2 = conv_desc(b, dh, dw, 32, 1)
        a2, s2 = conv_fwd(a1, conv_pack(_as_conv(w2), d2, PACK_FWD), b2, d2)
        a3, y = dec_dc34_fwd(a2, w3.contiguous(), b3, w4.contiguous(), b4)
        ctx.save_for_backward(x_lo, x_hi, a1, s1, a2, s2, a3, w1, w2, w3, w4)
        ctx.dims = (dh, dw)
        return y

    @staticmethod
    def backward(ctx, gy):
        x_lo, x_hi, a1, s1, a2, s2, a3, w1, w2, w3, w4 = ctx.saved_tensors
        dh, dw = ctx.dims
        b = x_lo.shape[0]
        g3, dw4, db4 = dec_dc4_bwd(gy.contiguous(), a3, w4.contiguous())
        dw3, db3 = dec_dc3_wgrad(a2, g3)
        g2 = dec_dc3_dgrad(g3, w3.contiguous(), s2)
        del g3
        d2 = conv_desc(b, dh, dw, 32, 1)
        dwc, db2 = conv_wgrad(a1, g2, d2)
        dw2 = _as_conv(dwc)                               # the map is its own inverse
        g1 = conv_dgrad(g2, conv_pack(_as_conv(w2), d2, PACK_DGRAD_S1), s1, d2)
        del g2
        gh, dw1, db1 = dec_dc1_bwd(x_lo, x_hi, g1, w1.contiguous(), want_dx=ctx.needs_input_grad[0])
        return gh, None, None, dw1, db1, dw2, db2, dw3, db3, dw4, db4


def decoder_conv_stack(h, dh, dw, dc1, dc2, dc3, dc4):
    return DecoderConvStackBf16.apply(h, dh, dw, dc1.weight, dc1.bias, dc2.weight, dc2.bias, dc3.weight, dc3.bias, dc4.weight, dc4.bias)
