"""Guard-band cases (tests/_guard.py) for the fp32 3x3 convolution kernels: the direct family of csrc/conv3x3.hip (dd_conv_pack, _fwd,
_fwd_relu_bits, _dgrad, _dgrad_relu_bits, _wgrad) and the two Winograd families of csrc/conv_wino.inc and csrc/conv_wino2.inc (dd_conv_wino_*, dd_conv_wino2_*, with
_dgrad_w1, _wgrad_partials and _wgrad_finish) and the BatchNorm2d variant (dd_conv_fwd_stats, dd_conv_dgrad_bn, dd_conv_wgrad_bn).  Packed-weight buffers are exactly ``*_packed_floats`` floats, workspaces exactly
their queries (76 MB of per-wave partials for the 32-channel weight gradient, whatever the image size), both left 0xFF.  What a case asserts: tests/test_gpu_guard_dense.py.  None of these launchers looks at an address.

An over-read whose value is discarded cannot be seen by these tests.

Run time on an MI355X: see tests/test_gpu_guard_layout.py (the guard files are timed together)."""
import pytest
import torch
from torch.nn import functional as F

from _guard import Case, Check, run_case

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

KERNEL_TOL = 2e-5        # tests/test_gpu_parity.py::test_conv_fwd_dgrad_wgrad, ::test_conv_winograd_fwd_dgrad_wgrad: of the tensor's peak
f32, i32 = torch.float32, torch.int32
PACK_FWD, PACK_DGRAD_S1, PACK_DGRAD_S2 = 0, 1, 2
EPI_BIAS_RELU = 2


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


def desc_of(b, h, w, cin, stride, rows):
    from driving_dirty_amd import _lib
    return _lib.ConvDesc(b, h, w, cin, 4 if cin == 3 else cin, 32, 3, stride, 1, rows)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def bits_of(x_nchw):
    """Sign words [B,H,W]: bit c = channel c > 0."""
    v = ((x_nchw > 0).long() << torch.arange(32).view(1, 32, 1, 1)).sum(1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(i32)


def store(x_nchw, cs):
    """NCHW fp64 -> NHWC fp32 with cs stored channels (the 4th of an NHWC4 image is zero)."""
    b, c, h, w = x_nchw.shape
    out = torch.zeros(b, h, w, cs)
    out[..., :c] = nhwc(x_nchw.float())
    return out


CASES = []


def case(name, entry, **kw):
    def deco(fn):
        CASES.append(Case(name, entry, fn, **kw))
        return fn
    return deco


def pack(arena, family, w_dev, desc, kind, name):
    n = size(family + "_packed_floats", desc, kind) if family == "dd_conv" else size(family + "_packed_floats", desc)
    packed = arena.workspace(n * 4, 16, name).view(f32)      # exactly the floats of the query, left 0xFF
    call(family + "_pack", w_dev, packed, desc, kind)
    return packed


# ------------------------------------------------------------------------------------------------ direct kernels
def _direct(b, h, w, cin, stride, rows):
    def fn(arena, mode):
        x64 = hu((b, cin, h, w), f"x{b}{h}{w}{cin}", 0.0, 1.0).double().requires_grad_(True)
        wt64 = hu((32, cin, 3, 3), f"w{cin}{stride}", -0.3, 0.3).double().requires_grad_(True)
        bias64 = hu((32,), f"b{cin}{stride}", -0.2, 0.2).double().requires_grad_(True)
        y64 = F.relu(F.conv2d(x64, wt64, bias64, stride=stride, padding=1))
        gy64 = hu(tuple(y64.shape), f"gy{b}{h}{w}{stride}").double() * (y64.detach() > 0)      # already masked by this layer's ReLU
        y64.backward(gy64)
        ho, wo = y64.shape[2], y64.shape[3]
        desc = desc_of(b, h, w, cin, stride, rows)
        cs = 4 if cin == 3 else 32
        x = arena.put(store(x64.detach(), cs), 16, "x")
        wd, bd = arena.put(wt64.detach().float(), 16, "weight"), arena.put(bias64.detach().float(), 16, "bias")
        pf = pack(arena, "dd_conv", wd, desc, PACK_FWD, "packed_fwd")
        y = arena.out((b, ho, wo, 32), f32, 16, "y")
        call("dd_conv_fwd", x, pf, bd, None, y, desc, EPI_BIAS_RELU)
        yb, sb = arena.out((b, ho, wo, 32), f32, 16, "y_bits"), arena.out((b, ho, wo), i32, 16, "relu_bits")
        call("dd_conv_fwd_relu_bits", x, pf, bd, yb, sb, desc)
        g = arena.put(nhwc(gy64.float()), 16, "dy")
        nbytes = size("dd_conv_wgrad_workspace_bytes", desc)
        ws = arena.workspace(nbytes, 16, "wgrad_workspace")
        dw, db = arena.out((32, cin, 3, 3), f32, 16, "dw"), arena.out((32,), f32, 16, "dbias")
        call("dd_conv_wgrad", x, g, dw, db, ws, nbytes, desc)
        if cin == 32:
            pd = pack(arena, "dd_conv", wd, desc, PACK_DGRAD_S1 if stride == 1 else PACK_DGRAD_S2, "packed_dgrad")
            dx = arena.out((b, h, w, 32), f32, 16, "dx")
            call("dd_conv_dgrad", g, pd, None, dx, desc)
            xm64 = x64.detach() - 0.5      # the previous layer's output, whose ReLU mask the data gradient applies
            src = arena.put(nhwc(xm64.float()), 16, "relu_src")
            dxm = arena.out((b, h, w, 32), f32, 16, "dx_masked")
            call("dd_conv_dgrad", g, pd, src, dxm, desc)
            mbits = arena.put(bits_of(xm64.float()), 16, "mask_bits")
            dxb = arena.out((b, h, w, 32), f32, 16, "dx_bits")
            call("dd_conv_dgrad_relu_bits", g, pd, mbits, dxb, desc)
        outs = arena.verify()
        checks = [Check("y", nchw(outs["y"]), y64, KERNEL_TOL), Check("y_bits", outs["y_bits"], outs["y"], how="exact"),
                  Check("relu_bits", outs["relu_bits"], bits_of(nchw(outs["y"])), how="exact"),
                  Check("dw", outs["dw"], wt64.grad, KERNEL_TOL), Check("dbias", outs["dbias"], bias64.grad, KERNEL_TOL)]
        if cin == 32:
            checks += [Check("dx", nchw(outs["dx"]), x64.grad, KERNEL_TOL),
                       Check("dx_masked", nchw(outs["dx_masked"]), x64.grad * (xm64 > 0), KERNEL_TOL),
                       Check("dx_bits", outs["dx_bits"], outs["dx_masked"], how="exact")]
        return checks
    return fn


_DIRECT = ("dd_conv_pack", "dd_conv_fwd", "dd_conv_fwd_relu_bits", "dd_conv_wgrad")
for _b, _h, _w in ((2, 7, 45), (1, 5, 131)):
    for _cin, _stride in ((3, 1), (32, 1), (32, 2)):
        for _rows in (0, 5):
            case(f"dd_conv[{_b},{_h},{_w},cin={_cin},stride={_stride},rows={_rows}]",
                 _DIRECT + (("dd_conv_dgrad", "dd_conv_dgrad_relu_bits") if _cin == 32 else ()), capacity=96 << 20)(_direct(_b, _h, _w, _cin, _stride, _rows))


# ------------------------------------------------------------------------------------------------ Winograd F(2,3) and F(2x2,3x3)
def _wino(b, h, w, rows):
    def fn(arena, mode):
        x64 = hu((b, 32, h, w), f"wx{b}{h}{w}", 0.0, 1.0).double().requires_grad_(True)
        wt64 = hu((32, 32, 3, 3), "ww", -0.3, 0.3).double().requires_grad_(True)
        bias64 = hu((32,), "wb", -0.2, 0.2).double().requires_grad_(True)
        y64 = F.relu(F.conv2d(x64, wt64, bias64, padding=1))
        gy64 = hu(tuple(y64.shape), f"wgy{b}{h}{w}").double() * (y64.detach() > 0)
        y64.backward(gy64)
        xm = x64.detach().float() - 0.5
        dx_ref = x64.grad * (xm > 0)
        img64 = hu((b, 3, h, w), f"wimg{b}{h}{w}", 0.0, 1.0).double()      # the 3 -> 32 layer's input, for dd_conv_wino2_dgrad_w1
        w1 = torch.zeros(32, 3, 3, 3, dtype=torch.float64, requires_grad=True)
        b1 = torch.zeros(32, dtype=torch.float64, requires_grad=True)
        F.conv2d(img64, w1, b1, padding=1).backward(dx_ref)
        desc = desc_of(b, h, w, 32, 1, rows)
        x = arena.put(store(x64.detach(), 32), 16, "x")
        wd, bd = arena.put(wt64.detach().float(), 16, "weight"), arena.put(bias64.detach().float(), 16, "bias")
        g = arena.put(nhwc(gy64.float()), 16, "dy")
        mbits = arena.put(bits_of(xm), 16, "mask_bits")
        img4 = arena.put(store(img64, 4), 16, "x_nhwc4")
        for fam in ("dd_conv_wino", "dd_conv_wino2"):
            t = fam[8:]
            pf, pd = pack(arena, fam, wd, desc, 0, t + "_packed_fwd"), pack(arena, fam, wd, desc, 1, t + "_packed_dgrad")
            y, bits = arena.out((b, h, w, 32), f32, 16, t + "_y"), arena.out((b, h, w), i32, 16, t + "_relu_bits")
            call(fam + "_fwd_relu_bits", x, pf, bd, y, bits, desc)
            dx = arena.out((b, h, w, 32), f32, 16, t + "_dx")
            call(fam + "_dgrad_relu_bits", g, pd, mbits, dx, desc)
            nbytes = size(fam + "_wgrad_workspace_bytes", desc)
            ws = arena.workspace(nbytes, 16, t + "_wgrad_workspace")
            dw, db = arena.out((32, 32, 3, 3), f32, 16, t + "_dw"), arena.out((32,), f32, 16, t + "_dbias")
            call(fam + "_wgrad", x, g, dw, db, ws, nbytes, desc)
            if fam == "dd_conv_wino2":
                ws2 = arena.workspace(nbytes, 16, "wino2_wgrad_workspace_2")      # the same in two calls
                dw2, db2 = arena.out((32, 32, 3, 3), f32, 16, "wino2_dw_2"), arena.out((32,), f32, 16, "wino2_dbias_2")
                call("dd_conv_wino2_wgrad_partials", x, g, ws2, nbytes, desc)
                call("dd_conv_wino2_wgrad_finish", ws2, nbytes, dw2, db2, desc)
                n1 = size("dd_conv_wino2_dgrad_w1_workspace_bytes", desc)
                ws1 = arena.workspace(n1, 16, "dgrad_w1_workspace")
                dw1, db1 = arena.out((32, 3, 3, 3), f32, 16, "dw1"), arena.out((32,), f32, 16, "dbias1")
                call("dd_conv_wino2_dgrad_w1", g, pd, mbits, img4, dw1, db1, ws1, n1, desc)
        outs = arena.verify()
        checks = []
        for t in ("wino", "wino2"):
            checks += [Check(t + " y", nchw(outs[t + "_y"]), y64, KERNEL_TOL),
                       Check(t + " relu_bits", outs[t + "_relu_bits"], bits_of(nchw(outs[t + "_y"])), how="exact"),
                       Check(t + " dx", nchw(outs[t + "_dx"]), dx_ref, KERNEL_TOL),
                       Check(t + " dw", outs[t + "_dw"], wt64.grad, KERNEL_TOL), Check(t + " dbias", outs[t + "_dbias"], bias64.grad, KERNEL_TOL)]
        checks += [Check("wino2 dw in two calls", outs["wino2_dw_2"], outs["wino2_dw"], how="exact"),
                   Check("wino2 dbias in two calls", outs["wino2_dbias_2"], outs["wino2_dbias"], how="exact"),
                   Check("dw1", outs["dw1"], w1.grad, KERNEL_TOL), Check("dbias1", outs["dbias1"], b1.grad, KERNEL_TOL)]
        return checks
    return fn


_WINO = tuple(f"dd_conv_{t}_{k}" for t in ("wino", "wino2") for k in ("pack", "fwd_relu_bits", "dgrad_relu_bits", "wgrad")) + (
    "dd_conv_wino2_wgrad_partials", "dd_conv_wino2_wgrad_finish", "dd_conv_wino2_dgrad_w1")
for _b, _h, _w, _rows in ((1, 1, 1, 0), (2, 4, 33, 0), (2, 4, 33, 3), (1, 3, 64, 0)):
    case(f"dd_conv_wino+wino2[{_b},{_h},{_w},rows={_rows}]", _WINO, capacity=224 << 20)(_wino(_b, _h, _w, _rows))


# ------------------------------------------------------------------------------------------------ the Conv -> BatchNorm2d -> ReLU variant
def _conv_bn(b, h, w, cin, stride):
    """dd_conv_fwd_stats (u = conv(relu(x * scale + shift)) + bias with the batch statistics gathered in the epilogue), the table
    handed to dd_bn2d_finalize; dd_conv_dgrad_bn and dd_conv_wgrad_bn, which see a pre-BN tensor through `affine` ([0:64) as the
    input transform, [64:128) as the mask transform: the two pairs differ here, so a kernel that reads the wrong one fails).  The
    statistics table is exactly dd_conv_stats_floats() floats, left 0xFF: the conv epilogue must leave every row defined.  Bounds:
    KERNEL_TOL, that of the same kernels without the transform (tests/test_gpu_parity.py::test_conv_fwd_dgrad_wgrad); the layer is
    otherwise held through the whole-model checks of tests/test_gpu_round3.py."""
    def fn(arena, mode):
        aff64 = torch.cat([hu((32,), "cbs", 0.5, 1.5), hu((32,), "cbh", -0.5, 0.5), hu((32,), "cbms", 0.5, 1.5), hu((32,), "cbmh", -0.7, 0.3)]).double()
        pre64 = hu((b, cin, h, w), f"cbx{b}{h}{w}{cin}", -1.0 if cin == 32 else 0.0, 1.0).double()
        col = lambda v: v.view(1, 32, 1, 1)
        xin64 = (F.relu(pre64 * col(aff64[:32]) + col(aff64[32:64])) if cin == 32 else pre64).requires_grad_(True)
        wt64 = hu((32, cin, 3, 3), f"cbw{cin}{stride}", -0.3, 0.3).double().requires_grad_(True)
        bias64 = hu((32,), f"cbb{cin}{stride}", -0.2, 0.2).double().requires_grad_(True)
        u64 = F.conv2d(xin64, wt64, bias64, stride=stride, padding=1)
        gy64 = hu(tuple(u64.shape), f"cbg{b}{h}{w}{stride}").double()
        u64.backward(gy64)
        ho, wo = u64.shape[2], u64.shape[3]
        desc = desc_of(b, h, w, cin, stride, 0)
        x = arena.put(store(pre64, 4 if cin == 3 else 32), 16, "pre_bn")
        wd, bd = arena.put(wt64.detach().float(), 16, "weight"), arena.put(bias64.detach().float(), 16, "bias")
        aff = arena.put(aff64.float(), 16, "affine")
        pf = pack(arena, "dd_conv", wd, desc, PACK_FWD, "packed_fwd")
        u = arena.out((b, ho, wo, 32), f32, 16, "u")
        nstats = size("dd_conv_stats_floats")
        stats = arena.workspace(nstats * 4, 16, "stats").view(f32)
        call("dd_conv_fwd_stats", x, pf, bd, aff if cin == 32 else None, u, stats, desc)
        ones, zeros = arena.put(torch.ones(32), 16, "gamma"), arena.put(torch.zeros(32), 16, "beta")
        rm, rv = arena.inout(torch.zeros(32), 16, "running_mean"), arena.inout(torch.ones(32), 16, "running_var")
        aff_out, sm, si = arena.out((128,), f32, 16, "affine_out"), arena.out((32,), f32, 16, "save_mean"), arena.out((32,), f32, 16, "save_invstd")
        call("dd_bn2d_finalize", stats, b * ho * wo, ones, zeros, rm, rv, 0.1, 1e-5, 1, aff_out, sm, si)
        if cin == 32:
            g = arena.put(nhwc(gy64.float()), 16, "dy")
            pd = pack(arena, "dd_conv", wd, desc, PACK_DGRAD_S1 if stride == 1 else PACK_DGRAD_S2, "packed_dgrad")
            dx = arena.out((b, h, w, 32), f32, 16, "dx")
            call("dd_conv_dgrad_bn", g, pd, x, aff, dx, desc)
            nbytes = size("dd_conv_wgrad_workspace_bytes", desc)
            ws = arena.workspace(nbytes, 16, "wgrad_workspace")
            dw, db = arena.out((32, 32, 3, 3), f32, 16, "dw"), arena.out((32,), f32, 16, "dbias")
            call("dd_conv_wgrad_bn", x, aff, g, dw, db, ws, nbytes, desc)
        outs = arena.verify()
        assert bool(torch.isfinite(stats.cpu()).all()), "dd_conv_fwd_stats must leave every row of the statistics table defined"
        ud = u64.detach()
        checks = [Check("u", nchw(outs["u"]), ud, KERNEL_TOL), Check("batch mean", outs["save_mean"], ud.mean((0, 2, 3)), KERNEL_TOL),
                  Check("batch invstd", outs["save_invstd"], 1 / (ud.var((0, 2, 3), unbiased=False) + 1e-5).sqrt(), KERNEL_TOL)]
        if cin == 32:
            mask = (pre64 * col(aff64[64:96]) + col(aff64[96:128])) > 0
            checks += [Check("dx", nchw(outs["dx"]), xin64.grad * mask, KERNEL_TOL), Check("dw", outs["dw"], wt64.grad, KERNEL_TOL),
                       Check("dbias", outs["dbias"], bias64.grad, KERNEL_TOL)]
        return checks
    return fn


for _b, _h, _w in ((2, 6, 10), (4, 16, 22)):
    for _cin, _stride in ((3, 1), (32, 1), (32, 2)):
        case(f"dd_conv_fwd_stats+dgrad_bn+wgrad_bn[{_b},{_h},{_w},cin={_cin},stride={_stride}]",
             ("dd_conv_fwd_stats",) + (("dd_conv_dgrad_bn", "dd_conv_wgrad_bn") if _cin == 32 else ()), capacity=96 << 20)(_conv_bn(_b, _h, _w, _cin, _stride))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
