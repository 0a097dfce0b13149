"""Conv -> BatchNorm2d -> ReLU encoder variant (reference src/autoencoder/components_v2.py:6-57) and its
ConvTranspose2d -> BatchNorm2d -> ReLU decoder (components_v2.py:59-98) on the HIP hot path.

The reference file is broken as committed: ``self.bn3 = nn.Conv2d(32)`` (components_v2.py:24) raises at construction
and nothing imports the module.  This build reads it as the evident ``nn.BatchNorm2d(32)``; everything else (layer
order, names ``bn1/bn2/bn3``, the pooled FC tail, ``c3_only``) follows the file.  Because the reference class cannot be
constructed, the oracle for this variant is a hand-composed ``F.conv2d -> F.batch_norm -> relu`` chain
(``oracle.ae_parts.EncoderNetV2``), not an import.

The v2 ``Decoder`` of the reference file DOES construct, so it is pinned by fixtures generated from the reference class
(``tests/golden/tiny_decoder_v2.npz``, ``full_decoder_v2.npz``).

Fusion (encoder): each conv kernel writes the pre-normalisation tensor and gathers the batch statistics in its epilogue (lane =
channel: no cross-lane traffic); ``relu(u*scale + shift)`` is applied by the kernels that READ the tensor (next conv's
row loader, pool, ReLU mask of the data gradient, weight-gradient input), so the normalised activation is never
written; the BN backward reductions use wavefront shuffles.
"""
import torch
from torch import nn

from . import _lib, ops
from ._lib import call, size
from .components import POOL, DenseBlock, _require_gpu
from .ops import PACK_DGRAD_S1, PACK_DGRAD_S2, PACK_FWD, conv_desc, conv_out, conv_pack


def _conv_stats(x, w, b, desc, in_aff):
    ho, wo = conv_out(desc.height, desc.stride), conv_out(desc.width, desc.stride)
    u = torch.empty((desc.batch, ho, wo, 32), device=x.device, dtype=torch.float32)
    stats = torch.empty(size("dd_conv_stats_floats"), device=x.device, dtype=torch.float32)
    call("dd_conv_fwd_stats", x, conv_pack(w, desc, PACK_FWD), b, in_aff, u, stats, desc)
    return u, stats


def _finalize(stats, count, bn, training):
    dev = bn.weight.device
    aff = torch.empty(128, device=dev, dtype=torch.float32)
    mean = torch.empty(32, device=dev, dtype=torch.float32)
    inv = torch.empty(32, device=dev, dtype=torch.float32)
    momentum = 0.1 if bn.momentum is None else bn.momentum
    call("dd_bn2d_finalize", stats, count, bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum, bn.eps, int(training), aff, mean, inv)
    if training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
    return aff, mean, inv


def _bn_bwd(g, u, gamma, mean, inv, training):
    du, dgamma, dbeta = torch.empty_like(u), torch.empty_like(gamma), torch.empty_like(gamma)
    ws = torch.empty(size("dd_bn2d_workspace_bytes"), device=u.device, dtype=torch.uint8)
    call("dd_bn2d_bwd", g, u, gamma, mean, inv, du, dgamma, dbeta, u.numel() // 32, int(training), ws)
    return du, dgamma, dbeta


class EncoderV2ConvStack(torch.autograd.Function):
    """x4 [B,H,W,4] -> pooled [B, 32*Ho*Wo/4] (pool=True) or the BN3+ReLU feature [B,Ho,Wo,32] (pool=False)."""

    @staticmethod
    def forward(ctx, x4, enc, training, pool, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, be3):
        b, h, w, _ = x4.shape
        d1, d2, d3 = conv_desc(b, h, w, 3, 1), conv_desc(b, h, w, 32, 1), conv_desc(b, h, w, 32, 2)
        ho, wo = conv_out(h, 2), conv_out(w, 2)
        u1, s1 = _conv_stats(x4, w1, b1, d1, None)
        a1, m1, i1 = _finalize(s1, b * h * w, enc.bn1, training)
        u2, s2 = _conv_stats(u1, w2, b2, d2, a1)
        a2, m2, i2 = _finalize(s2, b * h * w, enc.bn2, training)
        u3, s3 = _conv_stats(u2, w3, b3, d3, a2)
        a3, m3, i3 = _finalize(s3, b * ho * wo, enc.bn3, training)
        ctx.save_for_backward(x4, u1, u2, u3, a1, a2, a3, m1, i1, m2, i2, m3, i3, w2, w3, g1, g2, g3)
        ctx.cfg = (bool(training), bool(pool))
        if ops.TRACE is not None:      # test hook: the pre-normalisation tensors and their (scale, shift) tables -- relu(u * scale + shift) is
            ops.TRACE.update(v2=((u1, a1), (u2, a2), (u3, a3)))      # never written, the checker recomputes it with dd_bn2d_apply_relu
        if pool:
            pooled = torch.empty((b, (32 * ho * wo) // 4), device=x4.device, dtype=torch.float32)
            call("dd_pool4_bn_fwd", u3, a3, pooled, b, ho, wo)
            return pooled
        y3 = torch.empty_like(u3)
        call("dd_bn2d_apply_relu", u3, a3, y3, u3.numel() // 32)
        return y3

    @staticmethod
    def backward(ctx, grad):
        x4, u1, u2, u3, a1, a2, a3, m1, i1, m2, i2, m3, i3, w2, w3, g1, g2, g3 = ctx.saved_tensors
        training, pool = ctx.cfg
        b, h, w, _ = x4.shape
        ho, wo = conv_out(h, 2), conv_out(w, 2)
        d1, d2, d3 = conv_desc(b, h, w, 3, 1), conv_desc(b, h, w, 32, 1), conv_desc(b, h, w, 32, 2)
        grad = grad.contiguous()
        gh3 = torch.empty_like(u3)                       # dL/d(BN3 output), ReLU already applied
        if pool:
            call("dd_pool4_bn_bwd", grad, u3, a3, gh3, b, ho, wo)
        else:
            y3 = torch.empty_like(u3)
            call("dd_bn2d_apply_relu", u3, a3, y3, u3.numel() // 32)
            gh3 = ops.relu_bwd(grad, y3)
        du3, dg3, dbe3 = _bn_bwd(gh3, u3, g3, m3, i3, training)

        def wgrad_bn(u_in, aff, dy, desc):
            nbytes = size("dd_conv_wgrad_workspace_bytes", desc)
            ws = torch.empty(nbytes, device=dy.device, dtype=torch.uint8)
            dw = torch.empty((32, 32, 3, 3), device=dy.device, dtype=torch.float32)
            db = torch.empty(32, device=dy.device, dtype=torch.float32)
            call("dd_conv_wgrad_bn", u_in, aff, dy, dw, db, ws, nbytes, desc)
            return dw, db

        def dgrad_bn(dy, w, kind, u_in, aff, desc):
            dx = torch.empty((desc.batch, desc.height, desc.width, 32), device=dy.device, dtype=torch.float32)
            call("dd_conv_dgrad_bn", dy, conv_pack(w, desc, kind), u_in, aff, dx, desc)
            return dx

        dw3, db3 = wgrad_bn(u2, a2, du3, d3)
        gh2 = dgrad_bn(du3, w3, PACK_DGRAD_S2, u2, a2, d3)
        du2, dg2, dbe2 = _bn_bwd(gh2, u2, g2, m2, i2, training)
        dw2, db2 = wgrad_bn(u1, a1, du2, d2)
        gh1 = dgrad_bn(du2, w2, PACK_DGRAD_S1, u1, a1, d2)
        du1, dg1, dbe1 = _bn_bwd(gh1, u1, g1, m1, i1, training)
        dw1, db1 = ops.conv_wgrad(x4, du1, d1)
        return None, None, None, None, dw1, db1, dg1, dbe1, dw2, db2, dg2, dbe2, dw3, db3, dg3, dbe3


class Encoder(nn.Module):
    """components_v2.Encoder with ``bn3 = BatchNorm2d(32)``: same constructor signature and parameter names."""

    # the BatchNorm2d variants have no mixed-precision mode: asking for one is an error, not a quiet fp32 run
    @property
    def precision(self):
        return "fp32"

    @precision.setter
    def precision(self, value):
        if value != "fp32":
            raise ValueError(f"components_v2.Encoder: only precision 'fp32' is implemented (got {value!r})")

    def __init__(self, hidden_dim, latent_dim, in_channels, input_height, input_width):
        super().__init__()
        if in_channels != 3:
            raise ValueError("the MI355X conv stack is built for 3-channel camera images")
        self.hidden_dim, self.latent_dim = hidden_dim, latent_dim
        self.input_height, self.input_width, self.in_channels = input_height, input_width, in_channels
        self.c1 = nn.Conv2d(in_channels, 32, kernel_size=3, padding=1)
        self.bn1 = nn.BatchNorm2d(32)
        self.c2 = nn.Conv2d(32, 32, kernel_size=3, padding=1)
        self.bn2 = nn.BatchNorm2d(32)
        self.c3 = nn.Conv2d(32, 32, kernel_size=3, stride=2, padding=1)
        self.bn3 = nn.BatchNorm2d(32)
        self.pooling_size = POOL
        torch.rand(1, in_channels, input_height, input_width)      # RNG parity with the sizing dry run (:34)
        ho, wo = conv_out(input_height, 2), conv_out(input_width, 2)
        self.fc1 = DenseBlock((32 * ho * wo) // POOL, hidden_dim)
        self.fc2 = DenseBlock(hidden_dim, hidden_dim)
        self.fc_z_out = nn.Linear(hidden_dim, latent_dim)
        self.c3_only = False

    def forward_nhwc4(self, x4, keeps=(None, None)):
        args = (x4, self, self.bn1.training, not self.c3_only, self.c1.weight, self.c1.bias, self.bn1.weight, self.bn1.bias,
                self.c2.weight, self.c2.bias, self.bn2.weight, self.bn2.bias, self.c3.weight, self.c3.bias, self.bn3.weight,
                self.bn3.bias)
        out = EncoderV2ConvStack.apply(*args)
        if self.c3_only:
            return out.permute(0, 3, 1, 2)
        h = self.fc2(self.fc1(out, keeps[0]), keeps[1])
        return ops.linear(h, self.fc_z_out.weight, self.fc_z_out.bias)

    def forward(self, x, keeps=(None, None)):
        _require_gpu(x, "Encoder (v2)")
        return self.forward_nhwc4(ops.nchw_to_nhwc(x.contiguous(), 4), keeps)


# ------------------------------------------------------------------------------------------------ v2 decoder
def _stats(u):
    stats = torch.empty(size("dd_conv_stats_floats"), device=u.device, dtype=torch.float32)
    call("dd_bn2d_stats", u, stats, u.numel() // 32)
    return stats


def _apply_relu(u, aff):
    y = torch.empty_like(u)
    call("dd_bn2d_apply_relu", u, aff, y, u.numel() // 32)
    return y


class DecoderV2ConvStack(torch.autograd.Function):
    """[B, 64*dh*dw] (NCHW-flat, as fc2 emits it) -> [B,3,2dh,2dw]: (dc1 k3 p1, dc2 k3 p1, dc3 k2 s2) each followed by
    BatchNorm2d + ReLU, then dc4 k1 (components_v2.py:93-98).  The transposed convs run on the generic NHWC kernels
    (heads.DecoderConvStack's layers), the batch statistics on ``dd_bn2d_stats`` (wavefront-shuffle reductions), the
    BatchNorm backward on ``dd_bn2d_bwd``; each ReLU backward is the mask epilogue of the following layer's data gradient."""

    @staticmethod
    def forward(ctx, h, dec, training, dh, dw, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, be3, w4, b4):
        from .gconv import EPI_BIAS, View
        from .heads import DecoderConvStack as D
        b, dev = h.shape[0], h.device
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)      # noqa: E731
        x0 = ops.nchw_to_nhwc(h.contiguous().view(b, 64, dh, dw), 64)
        us, ys, stats = [], [x0], []
        for layer, w, bias, bn, shape in ((D.L1, w1, b1, dec.bn1, (b, dh, dw, 32)), (D.L2, w2, b2, dec.bn2, (b, dh, dw, 32)),
                                          (D.L3, w3, b3, dec.bn3, (b, 2 * dh, 2 * dw, 32))):
            u = new(*shape)
            layer.forward(w, bias, View(ys[-1]), View(u), EPI_BIAS)
            aff, mean, inv = _finalize(_stats(u) if training else None, u.numel() // 32, bn, training)
            us.append(u)
            stats.append((mean, inv))
            ys.append(_apply_relu(u, aff))
        y4 = torch.zeros((b, 2 * dh, 2 * dw, 4), device=dev, dtype=torch.float32)
        D.L4.forward(w4, b4, View(ys[3]), View(y4, 0, 3), EPI_BIAS)
        ctx.save_for_backward(*ys, *us, *[t for pair in stats for t in pair], w1, w2, w3, w4, g1, g2, g3)
        ctx.training = bool(training)
        return ops.nhwc_to_nchw(y4, 3)

    @staticmethod
    def backward(ctx, gy):
        from .gconv import View
        from .heads import DecoderConvStack as D
        sv = ctx.saved_tensors
        ys, us, st = sv[0:4], sv[4:7], sv[7:13]
        w1, w2, w3, w4, g1, g2, g3 = sv[13:]
        dev = gy.device
        g4 = ops.nchw_to_nhwc(gy.contiguous(), 4)
        dw4, db4 = D.L4.backward_weight(View(ys[3]), View(g4, 0, 3))
        g = torch.empty_like(ys[3])
        D.L4.backward_data(w4, View(g4), View(g), relu_src=ys[3])            # dL/d(BN3 output), ReLU applied
        grads = []
        for i, (layer, w, gamma) in reversed(list(enumerate(((D.L1, w1, g1), (D.L2, w2, g2), (D.L3, w3, g3))))):
            du, dgamma, dbeta = _bn_bwd(g, us[i], gamma, st[2 * i], st[2 * i + 1], ctx.training)
            dw, db = layer.backward_weight(View(ys[i]), View(du))
            grads.append((dw, db, dgamma, dbeta))
            if i > 0:
                g = torch.empty_like(ys[i])
                layer.backward_data(w, View(du), View(g), relu_src=ys[i])
            elif ctx.needs_input_grad[0]:
                g = torch.empty_like(ys[0])
                layer.backward_data(w, View(du), View(g))
        grads.reverse()
        gh = ops.nhwc_to_nchw(g, 64).view(g.shape[0], -1) if ctx.needs_input_grad[0] else None
        flat = [t for quad in grads for t in quad]
        return (gh, None, None, None, None, *flat, dw4, db4)


class Decoder(nn.Module):
    """components_v2.Decoder (components_v2.py:59-98): same constructor signature, parameter names and RNG consumption."""

    # the BatchNorm2d variants have no mixed-precision mode: asking for one is an error, not a quiet fp32 run
    @property
    def precision(self):
        return "fp32"

    @precision.setter
    def precision(self, value):
        if value != "fp32":
            raise ValueError(f"components_v2.Decoder: only precision 'fp32' is implemented (got {value!r})")

    def __init__(self, hidden_dim, latent_dim, in_channels, output_height, output_width):
        super().__init__()
        if in_channels != 3:
            raise ValueError("the MI355X decoder is built for 3-channel images")
        # RNG parity with the sizing dry run (components_v2.py:80-87): one rand + four throw-away convs
        torch.rand(1, in_channels, output_height, output_width)
        nn.Conv2d(in_channels, 32, 1)
        nn.Conv2d(32, 32, 2, stride=2)
        nn.Conv2d(32, 32, 3, padding=1)
        nn.Conv2d(32, 64, 3, padding=1)
        self.deconv_dim_h = (output_height - 2) // 2 + 1
        self.deconv_dim_w = (output_width - 2) // 2 + 1
        self.latent_dim = latent_dim
        self.fc1 = DenseBlock(latent_dim, hidden_dim)
        self.fc2 = DenseBlock(hidden_dim, self.deconv_dim_h * self.deconv_dim_w * 64)
        self.dc1 = nn.ConvTranspose2d(64, 32, kernel_size=3, padding=1)
        self.bn1 = nn.BatchNorm2d(32)
        self.dc2 = nn.ConvTranspose2d(32, 32, kernel_size=3, padding=1)
        self.bn2 = nn.BatchNorm2d(32)
        self.dc3 = nn.ConvTranspose2d(32, 32, kernel_size=2, stride=2)
        self.bn3 = nn.BatchNorm2d(32)
        self.dc4 = nn.ConvTranspose2d(32, in_channels, kernel_size=1, stride=1)

    def forward(self, z, keeps=(None, None)):
        _require_gpu(z, "Decoder (v2)")
        h = self.fc2(self.fc1(z, keeps[0]), keeps[1])
        return DecoderV2ConvStack.apply(h, self, self.bn1.training, self.deconv_dim_h, self.deconv_dim_w,
                                        self.dc1.weight, self.dc1.bias, self.bn1.weight, self.bn1.bias,
                                        self.dc2.weight, self.dc2.bias, self.bn2.weight, self.bn2.bias,
                                        self.dc3.weight, self.dc3.bias, self.bn3.weight, self.bn3.bias,
                                        self.dc4.weight, self.dc4.bias)
