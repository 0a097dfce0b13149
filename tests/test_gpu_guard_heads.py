"""Guard-band cases (tests/_guard.py) for the single-launch kernels of the decoder tail and the box heads that are called directly:
csrc/ssconv.hip (dd_ssconv_fwd, dd_ssconv_dgrad) and, in csrc/gconv.hip, dd_deconv2x2_c32_fwd / _fwd_slice / _wgrad,
dd_conv1x1_c32_c3_nchw and dd_deconv2x2_c1_fwd / _bwd.  What a case asserts: tests/test_gpu_guard_dense.py.  None of these launchers picks a kernel by address.

An over-read whose value is discarded cannot be seen by these tests.

Run time on an MI355X: see tests/test_gpu_guard_layout.py (the guard files are timed together)."""
import pytest
import torch
from torch.nn import functional as F

from _guard import Case, Check, run_case

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

TOL = 2e-5             # tests/test_gpu_gconv.py::test_decoder_tail_kernels: of the tensor's peak
ONE_LAUNCH_TOL = 2e-6  # tests/test_gpu_round4.py::test_ss_conv_forward_in_one_launch, ::test_ss_conv_data_gradient_in_one_launch,
#                        ::test_k2s2_weight_gradient_in_one_launch: of the reference's peak
f32 = torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def hu(shape, name, lo=-1.0, hi=1.0):
    return synth.hash_uniform(shape, synth.key_salt(name), lo, hi)


def call(name, *a):
    from driving_dirty_amd import _lib
    _lib.call(name, *a)


def size(name, *a):
    from driving_dirty_amd import _lib
    return _lib.size(name, *a)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


CASES = []


def case(name, entry, **kw):
    def deco(fn):
        CASES.append(Case(name, entry, fn, **kw))
        return fn
    return deco


# ------------------------------------------------------------------------------------------------ ss_conv: Conv2d(32, 32, (1, 24), stride (1, 7))
def _ssconv_fwd(b, h, xw, with_bias):
    def fn(arena, mode):
        gw = (xw - 24) // 7 + 1
        w0, b0, x0 = hu((32, 32, 1, 24), "sfw", -0.1, 0.1), hu((32,), "sfb", -0.5, 0.5), hu((b, h, xw, 32), f"sfx{h}{xw}")
        x, wt = arena.put(x0, 16, "x"), arena.put(w0, 16, "w")
        bias = arena.put(b0, 16, "bias") if with_bias else None
        y = arena.out((b, h, gw, 32), f32, 16, "y")
        call("dd_ssconv_fwd", x, wt, bias, y, b, h, xw, gw, 1)
        ref = F.relu(F.conv2d(nchw(x0).double(), w0.double(), b0.double() if with_bias else None, stride=(1, 7)))
        return [Check("y", nchw(arena.verify()["y"]), ref, ONE_LAUNCH_TOL)]
    return fn


for _b, _h, _xw, _bias in ((3, 7, 311, True), (1, 4, 24, True), (2, 3, 919, False)):      # a ragged last m-tile; one output pixel; trailing pixels no tap reaches
    case(f"dd_ssconv_fwd[{_b},{_h},{_xw},bias={_bias}]", "dd_ssconv_fwd", capacity=16 << 20)(_ssconv_fwd(_b, _h, _xw, _bias))


def _ssconv_dgrad(b, h, xw):
    def fn(arena, mode):
        from driving_dirty_amd import _lib
        gw = (xw - 24) // 7 + 1
        assert _lib.lib().dd_ssconv_dgrad_supported(h, gw, xw), "the shape must reach csrc/ssconv.hip"
        w0, g0 = hu((32, 32, 1, 24), "ssw", -0.1, 0.1), hu((b, h, gw, 32), f"ssg{h}{gw}")
        g, wt = arena.put(g0, 16, "g"), arena.put(w0, 16, "w")
        dx = arena.out((b, h, xw, 32), f32, 16, "dx")      # every element is written: pixels no tap reaches get 0
        call("dd_ssconv_dgrad", g, wt, dx, b, h, gw, xw)
        ref = F.conv_transpose2d(nchw(g0).double(), w0.double(), stride=(1, 7))
        ref = F.pad(ref, (0, xw - ref.shape[3]))
        return [Check("dx", nchw(arena.verify()["dx"]), ref, ONE_LAUNCH_TOL)]
    return fn


for _b, _h, _xw in ((3, 7, 311), (1, 128, 24), (2, 3, 919)):
    case(f"dd_ssconv_dgrad[{_b},{_h},{_xw}]", "dd_ssconv_dgrad", capacity=16 << 20)(_ssconv_dgrad(_b, _h, _xw))


# ------------------------------------------------------------------------------------------------ the decoder's tail
def _decoder_tail(b, h, w):
    def fn(arena, mode):
        x64 = hu((b, 32, h, w), "dtx").double()
        w3, b3 = hu((32, 32, 2, 2), "dtw3", -0.2, 0.2).double(), hu((32,), "dtb3", -0.2, 0.2).double()
        w4, b4 = hu((32, 3, 1, 1), "dtw4", -0.2, 0.2).double(), hu((3,), "dtb4", -0.2, 0.2).double()
        a3_ref = F.relu(F.conv_transpose2d(x64, w3, b3, stride=2))
        x = arena.put(nhwc(x64.float()), 16, "x")
        w3d, b3d = arena.put(w3.float(), 16, "w3"), arena.put(b3.float(), 16, "b3")
        w4d, b4d = arena.put(w4.float(), 16, "w4"), arena.put(b4.float(), 16, "b4")
        a3 = arena.out((b, 2 * h, 2 * w, 32), f32, 16, "a3")
        call("dd_deconv2x2_c32_fwd", x, w3d, b3d, a3, b, h, w, 1)
        lin = arena.out((b, 2 * h, 2 * w, 32), f32, 16, "linear")      # no bias, no ReLU
        call("dd_deconv2x2_c32_fwd", x, w3d, None, lin, b, h, w, 0)
        wide0 = hu((b, 2 * h, 2 * w, 56), "dtwide")                   # channels [8, 40) of a 56-channel buffer: the neighbours are guards
        wide = arena.inout(wide0, 16, "a3_slice")
        call("dd_deconv2x2_c32_fwd_slice", x, w3d, b3d, wide, b, h, w, 1, 56, 8)
        y = arena.out((b, 3, 2 * h, 2 * w), f32, 16, "y_nchw")
        call("dd_conv1x1_c32_c3_nchw", a3, w4d, b4d, y, b, 2 * h, 2 * w)
        outs = arena.verify()
        a3_got = outs["a3"]
        y_ref = F.conv_transpose2d(nchw(a3_got).double(), w4, b4)      # dc4 of what dc3 delivered: each kernel against fp64 on its own input
        sl = outs["a3_slice"]
        return [Check("a3", nchw(a3_got), a3_ref, TOL), Check("linear", nchw(outs["linear"]), F.conv_transpose2d(x64, w3, None, stride=2), TOL),
                Check("slice", sl[..., 8:40], a3_got, how="exact"), Check("slice left", sl[..., :8], wide0[..., :8], how="exact"),
                Check("slice right", sl[..., 40:], wide0[..., 40:], how="exact"), Check("y", outs["y_nchw"], y_ref, TOL)]
    return fn


_TAIL = ("dd_deconv2x2_c32_fwd", "dd_deconv2x2_c32_fwd_slice", "dd_conv1x1_c32_c3_nchw")
for _b, _h, _w in ((2, 5, 37), (1, 9, 32)):      # m-tiles that straddle rows and images; the narrowest width
    case(f"dd_deconv2x2_c32_fwd+slice+conv1x1[{_b},{_h},{_w}]", _TAIL)(_decoder_tail(_b, _h, _w))


def _k2s2_wgrad(b, h, w, gcs, coff, with_db):
    def fn(arena, mode):
        x0, g0 = hu((b, h, w, 32), "k2x"), hu((b, 2 * h, 2 * w, gcs), "k2g")
        wt = torch.zeros(32, 32, 2, 2, dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(32, dtype=torch.float64, requires_grad=True)
        yy = F.conv_transpose2d(nchw(x0).double(), wt, bias, stride=2)
        (yy * nchw(g0[..., coff:coff + 32]).double()).sum().backward()
        x, g = arena.put(x0, 16, "x"), arena.put(g0, 16, "g")
        dw = arena.out((32, 32, 2, 2), f32, 16, "dw")
        db = arena.out((32,), f32, 16, "db") if with_db else None
        nbytes = size("dd_deconv2x2_c32_wgrad_workspace_bytes")
        ws = arena.workspace(nbytes, 16)
        call("dd_deconv2x2_c32_wgrad", x, g, dw, db, b, h, w, gcs, coff, ws, nbytes)
        outs = arena.verify()
        return [Check("dw", outs["dw"], wt.grad, ONE_LAUNCH_TOL)] + ([Check("db", outs["db"], bias.grad, ONE_LAUNCH_TOL)] if with_db else [])
    return fn


for _b, _h, _w, _gcs, _coff, _db in ((2, 5, 7, 32, 0, True), (1, 9, 3, 40, 8, True), (1, 1, 2, 32, 0, False)):      # odd pixel counts; a slice; fewer pixels than waves
    case(f"dd_deconv2x2_c32_wgrad[{_b},{_h},{_w},{_gcs},{_coff},db={_db}]", "dd_deconv2x2_c32_wgrad", capacity=32 << 20)(_k2s2_wgrad(_b, _h, _w, _gcs, _coff, _db))


def _deconv_c1(b, h, w):
    """The box heads' last layer, ConvTranspose2d(8 -> 1, k2 s2) + sigmoid, and its backward (sigmoid', the (x > 0) mask of the ReLU
    that produced x, dwt, dbias through a workspace).  The pair has no kernel-level test (the heads' model tests hold it); the bound
    is TOL, that of the other single-launch transposed-conv kernels here."""
    def fn(arena, mode):
        x64 = torch.relu(hu((b, 8, h, w), f"c1x{h}{w}")).double().requires_grad_(True)
        wt64 = hu((8, 1, 2, 2), "c1w", -0.5, 0.5).double().requires_grad_(True)
        b64 = hu((1,), "c1b", -0.2, 0.2).double().requires_grad_(True)
        p64 = torch.sigmoid(F.conv_transpose2d(x64, wt64, b64, stride=2)).squeeze(1)
        dp64 = hu(tuple(p64.shape), f"c1g{h}{w}").double()
        p64.backward(dp64)
        x = arena.put(nhwc(x64.detach().float()), 16, "x")
        wt, bias = arena.put(wt64.detach().float(), 16, "wt"), arena.put(b64.detach().float(), 16, "bias")
        probs = arena.out((b, 2 * h, 2 * w), f32, 16, "probs")
        call("dd_deconv2x2_c1_fwd", x, wt, bias, probs, b, h, w, 8)
        dprobs = arena.put(dp64.float(), 16, "dprobs")
        dx, dwt, db = arena.out((b, h, w, 8), f32, 16, "dx"), arena.out((8, 1, 2, 2), f32, 16, "dwt"), arena.out((1,), f32, 16, "dbias")
        ws = arena.workspace(size("dd_deconv2x2_c1_workspace_bytes", 8), 16)
        call("dd_deconv2x2_c1_bwd", x, wt, probs, dprobs, dx, dwt, db, b, h, w, 8, ws)
        outs = arena.verify()
        return [Check("probs", outs["probs"], p64.detach(), TOL), Check("dx", nchw(outs["dx"]), x64.grad * (x64.detach() > 0), TOL),
                Check("dwt", outs["dwt"], wt64.grad, TOL), Check("dbias", outs["dbias"], b64.grad, TOL)]
    return fn


for _b, _h, _w in ((2, 5, 7), (1, 1, 1), (3, 16, 33)):      # an odd pixel count, one pixel (one block of the workspace), more than one block
    case(f"dd_deconv2x2_c1_fwd+bwd[{_b},{_h},{_w}]", ("dd_deconv2x2_c1_fwd", "dd_deconv2x2_c1_bwd"))(_deconv_c1(_b, _h, _w))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
