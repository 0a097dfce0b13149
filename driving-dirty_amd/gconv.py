"""Host-side planning for the generic NHWC convolution kernels (``dd_gconv_*``, csrc/gconv.hip).

A ``Layer`` describes one ``nn.Conv2d`` / ``nn.ConvTranspose2d`` of the reference in its own terms (kernel,
stride, dilation, padding, output_padding) and knows how to express its forward, its data gradient and its
weight gradient as launches of the ONE implicit-GEMM kernel family:

  Conv2d                      forward: plain;            dgrad: flipped taps, pad' = d(k-1)-p, div = stride
  ConvTranspose2d stride 1    forward: flipped taps, pad' = d(k-1)-p (+output_padding rows/cols);  dgrad: plain conv
  ConvTranspose2d k = s = 2   forward: 4 launches of a 1x1 conv, one per output phase;  dgrad: k2 s2 conv
Buffers are NHWC; a layer may read a channel slice of its input buffer and write a channel slice / a
sub-rectangle of its output buffer (mosaic tiling and channel concat without copies).
"""
import ctypes as C
import os
from contextlib import contextmanager
from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import _lib
from ._lib import GConvDesc, call, size

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_RELU_MASK, EPI_BIAS_SIGMOID = 0, 1, 2, 3, 4

_stream, _p, _chk = _lib.stream, _lib.ptr, _lib.dev      # the operand helpers live in _lib; _p / _stream stay for heads.py and tools/


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


@dataclass
class View:
    """A rectangular, channel-sliced window of an NHWC buffer [B, mem_h, mem_w, cstore]."""
    buf: torch.Tensor
    coff: int = 0
    chans: int = None
    off_h: int = 0
    off_w: int = 0
    h: int = None
    w: int = None

    def __post_init__(self):
        t = self.buf      # every kernel reads it through data_ptr() with the dense strides of its shape
        if not (t.dim() == 4 and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.HotpathError(f"View: a contiguous 4-D fp32 device buffer [B, H, W, C] is required, got {t.dtype} on {t.device}, "
                                    f"shape {tuple(t.shape)}, strides {t.stride()}")
        b, mh, mw, cs = t.shape
        self.chans = cs - self.coff if self.chans is None else self.chans
        self.h = mh - self.off_h if self.h is None else self.h
        self.w = mw - self.off_w if self.w is None else self.w


def _desc(batch, src, dst, cin, cout, k, stride=(1, 1), dil=(1, 1), pad=(0, 0), div=(1, 1), out_hw=None,
          ostride=(1, 1), ooff=(0, 0), mask_pass=(0, 0)):
    """src/dst: View.  src window offsets are folded into the padding (a shifted origin)."""
    _, imh, imw, ics = src.buf.shape
    _, omh, omw, ocs = dst.buf.shape
    assert src.off_h == 0 and src.off_w == 0, "input windows are not needed by this path"
    oh, ow = out_hw if out_hw is not None else (dst.h, dst.w)
    return GConvDesc(batch, imh, imw, ics, src.coff, cin, oh, ow, omh, omw, ocs, dst.coff, cout, k[0], k[1],
                     stride[0], stride[1], dil[0], dil[1], pad[0], pad[1], div[0], div[1], ostride[0], ostride[1],
                     dst.off_h + ooff[0], dst.off_w + ooff[1], mask_pass[0], mask_pass[1])


@dataclass(frozen=True)
class WMap:
    """Where a launch finds its weights in the parameter tensor ``w``, in the words of include/dd_hotpath.h: "element (n, c, tap) is read
    from w[w_off + n*sn + c*sc + (flip ? T-1-tap : tap)]; n < n_real output channels, c < c_real input channels (zero beyond)".
    Derived in ONE place, ``Layer.wmap``; a wrong stride still reads inside the parameter, so nothing but a numeric test would notice."""
    off: int
    sn: int
    sc: int
    flip: bool
    n_real: int
    c_real: int

    def operands(self):
        """(w_off, sn, sc, flip, n_real, c_real): the six operands in header order."""
        return self.off, self.sn, self.sc, int(self.flip), self.n_real, self.c_real


class Ran(NamedTuple):
    """What ``_conv`` did: ``xs`` the split image of x where the split-product kernels ran, ``colsum`` whether the caller's sums were filled."""
    xs: torch.Tensor = None
    colsum: bool = False


def _pack(w, d, wm):
    packed = torch.empty(size("dd_gconv_packed_floats", d), device=w.device, dtype=torch.float32)
    call("dd_gconv_pack", w, packed, d, *wm.operands())
    return packed


def _workspace(dev, query, *args):
    """(buffer, its size in bytes) as the launch functions take them, sized by the ``*_workspace_bytes`` query."""
    nbytes = size(query, *args)
    return torch.empty(nbytes, device=dev, dtype=torch.uint8), nbytes


def _fwd(x, packed, bias, mask, y, d, epi):
    call("dd_gconv_fwd", x, packed, bias, mask, y, d, epi)


# A/B switches: module attributes, read at call time (the tests and tools/ set them in process).
# The dilated stride-1 layers (the box heads' up-convs) have their own phase-decomposed, LDS-staged kernel (csrc/dconv.hip);
DCONV = True            # False = those layers on the generic gather engine again (same results up to summation order)
K2S2_WGRAD = True       # False = the k2 s2 32->32 weight gradient by four phase launches
SSCONV_FWD = True       # False = ss_conv's forward on the generic engine
SSCONV_DGRAD = True     # False = ss_conv's data gradient by seven phase launches
STRIP6 = True           # False = the six strip convs of SpatialMappingCNN on the generic engine (round 4)

# Precision mode "fp32x3" (csrc/dconv_split.hip; off by default): the forward, data gradient and weight gradient of up_conv_1 / up_conv_2
# with every fp32 product taken as six bf16 x bf16 products (exact 3-way operand split, fp32 accumulation) on the bf16 matrix pipe; error
# bound: DESIGN.md 3.3d.  Selected per module -- ``hparams.precision = "fp32x3"`` on BBSpatialRoadMap / JointRoadMapBBox, or
# ``box_merge.precision = "fp32x3"`` -- through ``split_products()`` below; ``gconv.SPLIT_BF16 = True`` is the process-wide default
# (DD_DCONV_SPLIT=1 sets it at import: tools' A/B).  The default everywhere stays the exact-fp32 MFMA kernels.
SPLIT_BF16 = os.environ.get("DD_DCONV_SPLIT", "0") == "1"


@contextmanager
def split_products(on):
    """``with split_products(True):`` -- the layers run inside take the split-product kernels where those serve them (False: the exact
    ones; None: whatever the process-wide default says).  heads.MergeFn records the mode of its forward and re-enters it in its
    backward, so a module's choice holds for the whole step however the backward is started."""
    global SPLIT_BF16
    prev = SPLIT_BF16
    if on is not None:
        SPLIT_BF16 = bool(on)
    try:
        yield
    finally:
        SPLIT_BF16 = prev


def _whole(*views, coff0=False):
    """Every View covers every pixel of its buffer (no window for the kernels that take whole-buffer dimensions); ``coff0``: from channel 0."""
    return all(v.off_h == 0 and v.off_w == 0 and v.h == v.buf.shape[1] and v.w == v.buf.shape[2] and not (coff0 and v.coff) for v in views)


def split_rows(view):
    """The three-plane bf16 image (csrc/dconv_split.hip) of the channels of a whole-buffer View: [B][H][chans / 16][W][112 B]."""
    if not (_whole(view) and view.chans % 16 == 0):
        raise _lib.HotpathError("split_rows: a whole-buffer View with a multiple of 16 channels")
    b, h, w, cs = view.buf.shape
    xs = torch.empty(b * h * (view.chans // 16) * w * 112, device=view.buf.device, dtype=torch.uint8)
    call("dd_dconv_split_rows", _chk(view.buf, "x"), xs, b * h, w, cs, view.coff, view.chans)
    return xs


def _ops():
    from . import ops      # ops imports nothing from here; deferred so that either module can be imported first
    return ops


def _dconv_ok(d):
    return DCONV and bool(_lib.lib().dd_dconv_supported(C.byref(d)))


def _conv(x, weight, bias, mask, y, d, epi, wm, xs=None, emit=None, colsum=None):
    """pack + launch on the dilated kernel when the descriptor qualifies, on the generic one otherwise -> ``Ran``.  ``xs``: the split
    image of x when a caller already holds it.  ``emit`` (a dict): on the split path the kernel also writes the split image of its
    OUTPUT from its epilogue (``emit['ys']``: the next layer's operand, no split pass).  ``colsum``: see Layer.backward_data."""
    lib = _lib.lib()
    if SPLIT_BF16 and lib.dd_dconv_split_supported(C.byref(d)) and (
            (d.pad_h > 0 and mask is None and epi in (EPI_NONE, EPI_BIAS, EPI_BIAS_RELU)) or (d.pad_h == 0 and epi in (EPI_NONE, EPI_RELU_MASK))):
        packed = torch.empty(size("dd_dconv_split_packed_bytes", d), device=x.device, dtype=torch.uint8)
        if xs is None:
            xs = torch.empty(size("dd_dconv_split_input_bytes", d), device=x.device, dtype=torch.uint8)
            call("dd_dconv_split_input", x, xs, d)
        call("dd_dconv_split_pack", weight, packed, d, *wm.operands())
        ys = None
        if emit is not None and d.cout % 16 == 0 and d.out_coff == 0 and d.ooff_h == 0 and d.ooff_w == 0 and d.omem_h == d.out_h and d.omem_w == d.out_w:
            ys = torch.empty(d.batch * d.out_h * (d.cout // 16) * d.out_w * 112, device=x.device, dtype=torch.uint8)
            emit["ys"] = ys
        call("dd_dconv_fwd_split", xs, packed, bias, mask, y, ys, d, epi)
        return Ran(xs=xs)
    if not _dconv_ok(d):
        _fwd(x, _pack(weight, d, wm), bias, mask, y, d, epi)
        return Ran()
    packed = torch.empty(size("dd_dconv_packed_floats", d), device=weight.device, dtype=torch.float32)
    call("dd_dconv_pack", weight, packed, d, *wm.operands())
    if (colsum is not None and bias is None and epi in (EPI_NONE, EPI_RELU_MASK)
            and lib.dd_dconv_colsum_supported(C.byref(d), epi, int(mask is not None))):
        # the launch also leaves the per-channel sums of its output: the bias gradient of the layer below (csrc/dconv_m.hip)
        call("dd_dconv_fwd_colsum", x, packed, mask, y, colsum, d, epi, *_workspace(x.device, "dd_dconv_colsum_workspace_bytes"))
        return Ran(colsum=True)
    call("dd_dconv_fwd", x, packed, bias, mask, y, d, epi)
    return Ran()


def _wgrad(x, dy, dw, db, d, wm, accumulate):
    call("dd_gconv_wgrad", x, dy, dw, db, d, *wm.operands(), int(accumulate), *_workspace(x.device, "dd_gconv_wgrad_workspace_bytes", d))


class Layer:
    """One Conv2d (``transposed=False``, weight OIHW) or ConvTranspose2d (``transposed=True``, weight IOHW)."""

    def __init__(self, cin, cout, k, stride=1, dil=1, pad=0, transposed=False, output_padding=0):
        self.cin, self.cout = cin, cout
        self.k, self.stride, self.dil, self.pad = _pair(k), _pair(stride), _pair(dil), _pair(pad)
        self.opad = _pair(output_padding)
        self.transposed = transposed
        self.T = self.k[0] * self.k[1]
        self.cin_store = (cin + 3) // 4 * 4
        self.k2s2 = transposed and self.k == (2, 2) and self.stride == (2, 2)
        if transposed and not self.k2s2 and self.stride != (1, 1):
            raise _lib.HotpathError("ConvTranspose2d: only stride 1 (dilated) and k2 s2 are built")
        # the geometries with kernels of their own: ss_conv, ss_deconv / the decoder's dc3, the box heads' square dilated up-convs
        self.ssconv = not transposed and (cin, cout, self.k, self.stride, self.dil, self.pad) == (32, 32, (1, 24), (1, 7), (1, 1), (0, 0))
        self.k2s2_c32 = self.k2s2 and cin == 32 and cout == 32
        self.square_dilated = transposed and not self.k2s2 and self.k[0] == self.k[1] and self.dil[0] == self.dil[1] and self.pad == (0, 0)
        self.w_fwd, self.w_dgrad = self.wmap(), self.wmap(dgrad=(0, cin))      # the whole-layer maps, built once

    def wmap(self, dgrad=None, tap=None, T=None):
        """The ONE derivation of weight addressing (``WMap``), from the parameter layout: W = [cout, cin, kh, kw] (Conv2d, taps as they
        lie) or [cin, cout, kh, kw] (ConvTranspose2d stride 1, taps flipped); n is the launch's output channel, T = kh * kw.
          wmap()                 forward and weight gradient: (n, c, t) is W[n, c][t], transposed W[c, n][T-1-t]
          wmap(tap=ph)           one tap as a 1x1 launch (k2 s2 by output phase): W[c, n][ph], nothing to flip
          wmap(dgrad=(n0, nn))   data gradient of channels [n0, n0 + nn): the forward map with n and c swapped, the flip toggled and the
                                 chunk's offset -- W[c, n0+n][T-1-t], transposed W[n0+n, c][t] (also the role-swapped weight gradient)
        ``T``: the tap count of a contiguous sub-weight handed over in W's place (the phased data gradient's sub-kernels)."""
        T = self.T if T is None else T
        sn, sc = (T, self.cout * T) if self.transposed else (self.cin * T, T)
        if tap is not None:
            return WMap(tap, sn, sc, False, self.cout, self.cin)
        if dgrad is None:
            return WMap(0, sn, sc, self.transposed, self.cout, self.cin)
        n0, nn = dgrad
        return WMap(n0 * sc, sc, sn, not self.transposed, nn, self.cout)

    # ---- shapes
    def out_hw(self, h, w):
        k, s, d, p = self.k, self.stride, self.dil, self.pad
        if self.transposed:
            return tuple((n - 1) * s[i] - 2 * p[i] + d[i] * (k[i] - 1) + self.opad[i] + 1 for i, n in enumerate((h, w)))
        return tuple((n + 2 * p[i] - d[i] * (k[i] - 1) - 1) // s[i] + 1 for i, n in enumerate((h, w)))

    def _flip_pad(self):
        return tuple(self.dil[i] * (self.k[i] - 1) - self.pad[i] for i in range(2))

    # ---- forward: writes dst (View) from src (View)
    def forward(self, weight, bias, src, dst, epilogue, mask=None, keep=None, xs=None, emit=None):
        """``keep`` (a dict): receives ``keep['xs']``, the split image of the input, when the split-product experiment ran -- the
        weight gradient of the same layer takes it back (``backward_weight(xs=...)``) instead of splitting x again.  ``xs``: that image
        when the caller already holds it (the previous layer's ``emit['ys']``); ``emit`` (a dict): also write the output's."""
        b = src.buf.shape[0]
        cs = src.chans if src.chans % 4 == 0 else self.cin_store
        _chk(weight, "weight")
        if (self.ssconv and mask is None and epilogue in (EPI_BIAS, EPI_BIAS_RELU) and SSCONV_FWD and _whole(src, dst, coff0=True)
                and _ops().ssconv_dgrad_ok(dst.buf, src.buf)):
            _ops().ssconv_fwd(src.buf, weight.contiguous(), bias, dst.buf, relu=epilogue == EPI_BIAS_RELU)      # ss_conv (csrc/ssconv.hip)
        elif not self.transposed:
            d = _desc(b, src, dst, cs, self.cout, self.k, self.stride, self.dil, self.pad)
            _conv(src.buf, weight, bias, mask, dst.buf, d, epilogue, self.w_fwd)
        elif self.k2s2:
            ih, iw = src.buf.shape[1:3]
            for ph in range(4):
                d = _desc(b, src, dst, cs, self.cout, (1, 1), out_hw=(ih, iw), ostride=(2, 2), ooff=(ph // 2, ph % 2))
                _fwd(src.buf, _pack(weight, d, self.wmap(tap=ph)), bias, mask, dst.buf, d, epilogue)
        else:
            d = _desc(b, src, dst, cs, self.cout, self.k, (1, 1), self.dil, self._flip_pad())
            ran = _conv(src.buf, weight, bias, mask, dst.buf, d, epilogue, self.w_fwd, xs=xs, emit=emit)
            if keep is not None and ran.xs is not None:
                keep["xs"] = ran.xs

    # ---- data gradient: dsrc (View with the input's geometry, >= 4-aligned channels) from ddst (View of dy)
    def backward_data(self, weight, ddst, dsrc, relu_src=None, mask_pass=(0, 0), gs=None, emit=None, colsum=None):
        """dsrc.buf[..., dsrc.coff : +cin] = dL/dx (x masked by ``relu_src > 0`` when given; channels
        [mask_pass[0], mask_pass[1]) of the dsrc buffer are exempt: a concat slice that is not a ReLU output).
        ``colsum`` (a [cin] float tensor): where the kernel can, it also receives the per-channel sums of what was written -- the bias
        gradient of the layer that produced x.  -> True when ``colsum`` was filled, False otherwise."""
        b = ddst.buf.shape[0]
        epi = EPI_RELU_MASK if relu_src is not None else EPI_NONE
        cin = self.cin
        cos = (self.cout + 3) // 4 * 4
        if self.transposed and not self.k2s2 and cin <= 96:
            # the dilated kernel takes up to 96 output channels in one launch (three column tiles per wave)
            d = _desc(b, ddst, dsrc, cos, cin, self.k, (1, 1), self.dil, self.pad, mask_pass=mask_pass)
            if _dconv_ok(d):
                return _conv(ddst.buf, weight, None, relu_src, dsrc.buf, d, epi, self.w_dgrad, xs=gs, emit=emit, colsum=colsum).colsum
        if (self.ssconv and relu_src is None and SSCONV_DGRAD and _whole(ddst, dsrc, coff0=True)
                and _ops().ssconv_dgrad_ok(ddst.buf, dsrc.buf)):
            _ops().ssconv_dgrad(ddst.buf, weight.contiguous(), dsrc.buf)      # ss_conv: all seven phases in one launch (csrc/ssconv.hip)
        elif not self.transposed and self.stride != (1, 1) and self.dil == (1, 1) and self.pad == (0, 0) and cin <= 64:
            self._backward_data_phased(weight, ddst, dsrc, relu_src, mask_pass, epi, cos)
        else:
            for n0 in range(0, cin, 64):                    # the generic kernel writes at most 64 channels per launch
                nn = min(64, cin - n0)
                out = View(dsrc.buf, dsrc.coff + n0, nn, dsrc.off_h, dsrc.off_w, dsrc.h, dsrc.w)
                wm = self.wmap(dgrad=(n0, nn))
                if not self.transposed:
                    d = _desc(b, ddst, out, cos, nn, self.k, (1, 1), self.dil, self._flip_pad(), div=self.stride, mask_pass=mask_pass)
                    if _dconv_ok(d):      # stride-1 3x3 layers (out_conv, rm_conv_2): the LDS-tiled kernel
                        _conv(ddst.buf, weight, None, relu_src, out.buf, d, epi, wm)
                        continue
                elif self.k2s2:
                    d = _desc(b, ddst, out, cos, nn, (2, 2), (2, 2), mask_pass=mask_pass)
                else:
                    d = _desc(b, ddst, out, cos, nn, self.k, (1, 1), self.dil, self.pad, mask_pass=mask_pass)
                _fwd(ddst.buf, _pack(weight, d, wm), None, relu_src, out.buf, d, epi)
        return False

    def _backward_data_phased(self, weight, ddst, dsrc, relu_src, mask_pass, epi, cos):
        """Data gradient of a strided Conv2d (no padding, no dilation) by input phase: input pixels of equal residue
        (iy mod sh, ix mod sw) = (ry, rx) only ever meet the taps ky = ry + sh*jy, kx = rx + sw*jx, so
            dx[sh*my + ry, sw*mx + rx] = sum_j g[my - jy, mx - jx] * w[ry + sh*jy, rx + sw*jx]
        is a stride-1 transposed convolution of g with the (ry, rx) sub-kernel, written at output stride (sh, sw), offset
        (ry, rx).  The gather with a divisibility test visits all kh*kw taps for every pixel (ss_conv, k 1x24 stride 7: 24 taps
        for the 3.4 that contribute -- 3.6 ms at bs 32); the sh*sw phase launches do exactly the useful work (0.5 ms)."""
        b = ddst.buf.shape[0]
        sh, sw = self.stride
        out = View(dsrc.buf, dsrc.coff, self.cin, dsrc.off_h, dsrc.off_w, dsrc.h, dsrc.w)
        for ry in range(min(sh, self.k[0])):
            for rx in range(min(sw, self.k[1])):
                sub = weight[:, :, ry::sh, rx::sw].contiguous()                  # [cout, cin, njy, njx]
                njy, njx = sub.shape[2:]
                mh, mw = (dsrc.h - ry + sh - 1) // sh, (dsrc.w - rx + sw - 1) // sw      # pixels of this phase
                d = _desc(b, ddst, out, cos, self.cin, (njy, njx), (1, 1), (1, 1), (njy - 1, njx - 1), out_hw=(mh, mw),
                          ostride=(sh, sw), ooff=(ry, rx), mask_pass=mask_pass)
                _fwd(ddst.buf, _pack(sub, d, self.wmap(dgrad=(0, self.cin), T=njy * njx)), None, relu_src, out.buf, d, epi)
        # phases past the kernel extent (stride > kernel) receive no gradient
        for ry in range(sh):
            for rx in range(sw):
                if ry >= self.k[0] or rx >= self.k[1]:
                    dsrc.buf[:, dsrc.off_h + ry:dsrc.off_h + dsrc.h:sh, dsrc.off_w + rx:dsrc.off_w + dsrc.w:sw, dsrc.coff:dsrc.coff + self.cin] = 0

    # ---- weight (+bias) gradient
    def split_wgrad_ok(self, src, ddst):
        """The split-product weight gradient (csrc/dconv_split.hip) serves this call: the experiment is on, a k7 d7 layer it is built
        for, whole-buffer Views."""
        return (SPLIT_BF16 and self.square_dilated and src.chans == self.cin and ddst.chans == self.cout and _whole(src, ddst)
                and bool(_lib.lib().dd_dconv_wgrad_split_supported(self.k[0], self.dil[0], self.cin, self.cout)))

    def backward_weight(self, src, ddst, want_bias=True, xs=None, gs=None):
        b, ih, iw, ics = src.buf.shape
        _, gh, gw, gcs = ddst.buf.shape
        dev = src.buf.device
        cs = src.chans if src.chans % 4 == 0 else self.cin_store
        dw = torch.empty(((self.cin, self.cout) if self.transposed else (self.cout, self.cin)) + self.k, device=dev, dtype=torch.float32)
        db = torch.empty(self.cout, device=dev, dtype=torch.float32) if want_bias else None
        if not self.transposed:
            d = _desc(b, src, ddst, cs, self.cout, self.k, self.stride, self.dil, self.pad)
            _wgrad(src.buf, ddst.buf, dw, db, d, self.w_fwd, 0)
            return dw, db
        if self.k2s2_c32 and K2S2_WGRAD and _whole(src, ddst) and src.coff == 0 and ics == 32 and iw >= 2 and (gh, gw) == (2 * ih, 2 * iw):
            # ss_deconv / the decoder's dc3: the four phases in one launch (csrc/gconv.hip, deconv2x2_c32_wgrad_kernel)
            call("dd_deconv2x2_c32_wgrad", src.buf, ddst.buf, dw, db, b, ih, iw, gcs, ddst.coff, *_workspace(dev, "dd_deconv2x2_c32_wgrad_workspace_bytes"))
            return dw, db
        if self.k2s2:
            for ph in range(4):
                d = _desc(b, src, ddst, cs, self.cout, (1, 1), out_hw=(ih, iw), ostride=(2, 2), ooff=(ph // 2, ph % 2))
                _wgrad(src.buf, ddst.buf, dw, db, d, self.wmap(tap=ph), 2 if ph > 0 else 0)
            return dw, db
        # stride-1 transposed layers; all but the last form leave the bias gradient (the sum of dy) to a per-channel sum of its own
        if self.split_wgrad_ok(src, ddst):
            # EXPERIMENT: both operands as three bf16 planes, six bf16 x bf16 products per fp32 product (csrc/dconv_split.hip); the
            # split images of x (from the forward) and of dL/dy (from the data gradient) are taken over when the caller holds them
            xs = split_rows(src) if xs is None else xs
            gs = split_rows(ddst) if gs is None else gs
            call("dd_dconv_wgrad_split", xs, gs, dw, b, ih, iw, self.cin, gh, gw, self.cout, 0,
                 *_workspace(dev, "dd_dconv_wgrad_split_workspace_bytes", self.cin, self.cout))
        elif (DCONV and self.square_dilated and src.chans == self.cin and ddst.chans == self.cout and _whole(src, ddst)
              and _lib.lib().dd_dconv_wgrad_supported(self.k[0], self.dil[0], self.cin, self.cout)):
            # the box heads' dilated up-convs: LDS-staged weight-gradient kernel (csrc/dconv.hip)
            call("dd_dconv_wgrad", src.buf, ddst.buf, dw, b, ih, iw, ics, src.coff, self.cin, gh, gw, gcs, ddst.coff, self.cout, self.k[0],
                 self.dil[0], 0, *_workspace(dev, "dd_dconv_wgrad_workspace_bytes", self.k[0], self.dil[0], self.cin, self.cout))
        elif self.cin <= 96 and self.cout % 4 == 0 and ddst.off_h == 0 and ddst.off_w == 0:
            # role-swapped: dWt[c][o][t] = sum over INPUT pixels p of x[p][c] * dy[p + t*d - pad][o] is the weight gradient of the plain
            # conv  dx = conv(dy, Wt)  with x in the role of its output gradient.  Every tap of every pixel is inside dy there, whereas
            # the flipped-tap form spends (out/in)^2 - 1 of its MFMAs on the zero border.
            d = _desc(b, ddst, src, self.cout, self.cin, self.k, (1, 1), self.dil, self.pad)
            _wgrad(ddst.buf, src.buf, dw, None, d, self.w_dgrad, 0)
        else:
            d = _desc(b, src, ddst, cs, self.cout, self.k, (1, 1), self.dil, self._flip_pad())
            _wgrad(src.buf, ddst.buf, dw, db, d, self.w_fwd, 0)
            return dw, db
        if want_bias:
            channel_sum(ddst, db)
        return dw, db


def copy_channels(src, dst):
    """dst.buf[..., dst.coff : +chans] = src.buf[..., src.coff : +chans] over the Views' windows (equal h x w; whole buffers of equal
    pixel count take the one-dimensional kernel)."""
    assert src.chans == dst.chans and src.buf.shape[0] == dst.buf.shape[0] and (src.h, src.w) == (dst.h, dst.w)
    if not _whole(src, dst):
        call("dd_copy_channels_window", _chk(src.buf, "src"), _chk(dst.buf, "dst"), src.buf.shape[0], src.h, src.w, src.chans, src.buf.shape[1],
             src.buf.shape[2], src.off_h, src.off_w, src.buf.shape[3], src.coff, dst.buf.shape[1], dst.buf.shape[2], dst.off_h, dst.off_w,
             dst.buf.shape[3], dst.coff)
        return
    npix = src.buf.shape[0] * src.buf.shape[1] * src.buf.shape[2]
    call("dd_copy_channels", _chk(src.buf, "src"), _chk(dst.buf, "dst"), npix, src.chans, src.buf.shape[3], src.coff, dst.buf.shape[3], dst.coff)


def channel_sum(view, out, accumulate=False):
    """out[c] = sum over all pixels of view.buf[..., view.coff + c] (dense buffers only)."""
    b, mh, mw, cs = view.buf.shape
    assert _whole(view)
    ws = torch.empty(size("dd_channel_sum_workspace_bytes"), device=view.buf.device, dtype=torch.uint8)
    call("dd_channel_sum", view.buf, out, b * mh * mw, cs, view.coff, view.chans, int(accumulate), ws)


_VIEW_ENTRIES = {"views": "dd_view_to_nhwc4", "samples": "dd_view_to_nhwc4_ptrs", "frames": "dd_view_to_nhwc4_u8_ptrs"}      # by ops.camera_source's form


def view_to_nhwc4(views, view, transform):
    """views [B,6,3,H,W] -- or the collate's tuple / list of B per-sample [6,3,H,W] tensors, read through a pointer table
    (no torch.stack) -- -> one view as NHWC4 with SpatialMappingCNN's rot90/flip applied (see dd_view_to_nhwc4).  uint8 frames
    ([B,6,H,W,3] or a tuple of [6,H,W,3]) are read as they are, ToTensor's /255 fused (dd_view_to_nhwc4_u8_ptrs)."""
    form, src, b, h, w, dev, _keep = _ops().camera_source(views, "view_to_nhwc4")
    y = torch.empty((b, w, h, 4) if transform in (1, 2) else (b, h, w, 4), device=dev, dtype=torch.float32)
    call(_VIEW_ENTRIES[form], src, y, b, h, w, view, transform)
    return y


def strip6_supported(h, w):
    return STRIP6 and bool(_lib.lib().dd_strip6_supported(int(h), int(w)))


def _ptr6(tensors, who, shapes=None):
    for i, t in enumerate(tensors):
        _chk(t, f"{who}[{i}]")
        if shapes is not None and tuple(t.shape) != tuple(shapes[i]):
            raise _lib.HotpathError(f"{who}[{i}]: shape {tuple(t.shape)} != {tuple(shapes[i])}")
    return (C.c_void_p * 6)(*[t.data_ptr() for t in tensors])


_STRIP_SHAPES = [(32, 3, 1, 50), (32, 3, 1, 50), (32, 3, 52, 1), (32, 3, 52, 1), (32, 3, 1, 50), (32, 3, 1, 50)]      # bl, fl, b, f, br, fr


def strip6_fwd(views, weights, biases, want_bits=False):
    """The six strip convs of SpatialMappingCNN (+ bias + ReLU) in one launch, written into their tiles of the 3 x 2 mosaic
    (dd_strip6_fwd; spatial_bb/components.py:34-73).  ``weights`` / ``biases``: bl, fl, b, f, br, fr.  -> mosaic [B, 3 th, 2 tw, 32];
    with ``want_bits`` also its sign words, int32 [B, 3 th, 2 tw] (the ReLU mask of out_conv's data gradient on the Winograd kernels)."""
    table, b, h, w, dev, u8, _keep = _ops().sample_table(views, "strip6_fwd")
    th, tw = (h - 1) // 3 + 1, (w - 50) // 2 + 1
    weights = [x.contiguous() for x in weights]
    mosaic = torch.empty((b, 3 * th, 2 * tw, 32), device=dev, dtype=torch.float32)
    bits = torch.empty((b, 3 * th, 2 * tw), device=dev, dtype=torch.int32) if want_bits else None
    call("dd_strip6_fwd", table, u8, _ptr6(weights, "weight", _STRIP_SHAPES), _ptr6(biases, "bias", [(32,)] * 6), mosaic, bits if want_bits else None,
         b, h, w)
    return (mosaic, bits) if want_bits else mosaic


def strip6_wgrad(views, g):
    """Weight and bias gradients of the six strip convs from dL/d(mosaic) (ReLU-masked) in one launch + a fixed-order reduce
    (dd_strip6_wgrad).  -> ([dw] * 6, [db] * 6) in the order bl, fl, b, f, br, fr."""
    table, b, h, w, dev, u8, _keep = _ops().sample_table(views, "strip6_wgrad")
    th, tw = (h - 1) // 3 + 1, (w - 50) // 2 + 1
    _chk(g, "g")
    if tuple(g.shape) != (b, 3 * th, 2 * tw, 32):
        raise _lib.HotpathError(f"strip6_wgrad: g {tuple(g.shape)} != {(b, 3 * th, 2 * tw, 32)}")
    dws = [torch.empty(s, device=dev, dtype=torch.float32) for s in _STRIP_SHAPES]
    dbs = [torch.empty(32, device=dev, dtype=torch.float32) for _ in range(6)]
    call("dd_strip6_wgrad", table, u8, g, _ptr6(dws, "dw"), _ptr6(dbs, "db"), b, h, w, *_workspace(dev, "dd_strip6_wgrad_workspace_bytes"))
    return dws, dbs


def add(a, b):
    out = torch.empty_like(a)
    call("dd_add", _chk(a, "a"), _chk(b, "b"), out, a.numel())
    return out
