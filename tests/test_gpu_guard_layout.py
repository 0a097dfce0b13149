"""Guard-band cases (tests/_guard.py) for the layout, gather, pooling, copy and BatchNorm2d entry points: csrc/layout_pool.hip and the
stacked-batch gathers of csrc/camera_gather.hip (dd_stitch6*, dd_view_to_nhwc4; dd_subsample_nhwc4 included), dd_pool4_bn_fwd / _bwd of csrc/bn2d.hip, the helpers
of csrc/conv3x3.hip (sign words, padded ReLU backward), csrc/gconv.hip's channel copies and sums, the fp32 <-> bf16 converters of
csrc/conv3x3_bf16.hip and csrc/bn2d.hip's stand-alone kernels.  What a case asserts: tests/test_gpu_guard_dense.py.

An over-read whose value is discarded cannot be seen by these tests.

Run time on an MI355X, measured: 6.1 s for the 211 tests of the eight tests/test_gpu_guard_*.py files run together; the whole
``-m gpu`` run with them: 329 s, 862 tests, all passing (tests/test_gpu_batch_boundaries.py recorded 310 s for 478)."""
import pytest
import torch
from torch.nn import functional as F

from _guard import Case, Check, run_case

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

KERNEL_TOL = 2e-5        # tests/test_gpu_parity.py: of the tensor's peak magnitude
CHANNEL_SUM_TOL = 2e-6   # tests/test_gpu_gconv.py::test_channel_sum: of the largest per-channel sum of absolute values (4e-6 accumulating)
f32, f64, i32, i16, bf16 = torch.float32, torch.float64, torch.int32, torch.int16, torch.bfloat16

# Launchers of these files that pick a kernel by the alignment of an operand:
ALIGNMENT_PICKS = {
    "dd_channel_sum": "csrc/gconv.hip:1029  cstore % 4 == 0 && cstore <= 256 && buf % 16 == 0 -> channel_sum_stream, else channel_sum_partial",
    "dd_pool4_fwd_idx": "csrc/layout_pool.hip:500  c == 32 && feat % 16 == 0 && idx % 4 == 0 -> pool4_fwd_tile32, else pool4_fwd_quad<true>",
    "dd_pool4_idx_relu_bwd": "csrc/layout_pool.hip:516  c == 32 && dfeat % 16 == 0 && idx % 4 == 0 -> pool4_bwd_tile32, else pool4_bwd_idx_quad",
}
# The two pool kernels' other side still reads feat / writes dfeat as 16-byte vectors, so only idx (uint16 codes) may be less
# aligned: the crossing cases put idx on 2 bytes.  Both sides route the same values, so these cases keep the bit-for-bit comparison
# of pooled / dfeat; the codes themselves are compared with the reference routing in both modes.


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


# ------------------------------------------------------------------------------------------------ NCHW <-> NHWC
def _layout(b, c, cs, h, w):
    def fn(arena, mode):
        x0 = hu((b, c, h, w), f"lay{b}{c}{h}{w}")
        src = arena.put(x0, 16, "src_nchw")
        mid = arena.out((b, h, w, cs), f32, 16, "nhwc")
        call("dd_nchw_to_nhwc", src, mid, b, c, h, w, cs)
        back = arena.out((b, c, h, w), f32, 16, "back_nchw")
        call("dd_nhwc_to_nchw", mid, back, b, c, h, w, cs)
        outs = arena.verify()
        want = torch.zeros(b, h, w, cs)
        want[..., :c] = nhwc(x0)      # the extra channels are written as zero
        return [Check("nhwc", outs["nhwc"], want, how="exact"), Check("nchw", outs["back_nchw"], x0, how="exact")]
    return fn


for _b, _c, _cs, _h, _w in ((2, 5, 8, 7, 11), (1, 3, 4, 5, 9)):      # layout_tile_kernel (8 <= c_store <= 64) and the NHWC4 kernels
    case(f"dd_nchw_to_nhwc+back[{_b},{_c}->{_cs},{_h},{_w}]", ("dd_nchw_to_nhwc", "dd_nhwc_to_nchw"))(_layout(_b, _c, _cs, _h, _w))


# ------------------------------------------------------------------------------------------------ the 6-view gathers on a stacked batch
VIEW_ORDER = (0, 1, 2, 5, 4, 3)


def wide_of(v):
    """[B,6,C,H,W] -> [B,C,H,6W] in the reference's view order (oracle.steps.wide_stitch)."""
    x = v[:, list(VIEW_ORDER)]
    b, n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1, 4).reshape(b, c, h, n * w)


def nhwc4(x_nchw):
    b, c, h, w = x_nchw.shape
    out = torch.zeros(b, h, w, 4, dtype=x_nchw.dtype)
    out[..., :c] = x_nchw.permute(0, 2, 3, 1)
    return out


def _stitch(b, h, w, slot):
    """dd_stitch6 (all three outputs), dd_stitch6_u8, dd_stitch6_bf16 and dd_stitch6_bf16_masked on one stacked batch: pure gathers,
    compared exactly (tests/test_gpu_parity.py::test_stitch6, tests/test_gpu_bf16.py); the uint8 path's division by 255 within 1e-7
    (tests/test_gpu_parity.py::test_stitch6_uint8_pipeline)."""
    def fn(arena, mode):
        v0 = hu((b, 6, 3, h, w), "views", 0.0, 1.0)
        f0 = (hu((b, 6, h, w, 3), "frames", 0.0, 1.0) * 255).round().to(torch.uint8)
        ref = wide_of(v0).clone()
        tgt_ref = None
        if slot >= 0:
            tgt_ref = ref[..., slot * w:(slot + 1) * w].clone()
            ref[..., slot * w:(slot + 1) * w] = 0
        views, frames = arena.put(v0, 16, "views"), arena.put(f0, 16, "frames")
        wide4, wide = arena.out((b, h, 6 * w, 4), f32, 16, "wide_nhwc4"), arena.out((b, 3, h, 6 * w), f32, 16, "wide_nchw")
        tgt = arena.out((b, 3, h, w), f32, 16, "target") if slot >= 0 else None
        call("dd_stitch6", views, wide4, wide, tgt, b, h, w, slot)
        wide_u8 = arena.out((b, h, 6 * w, 4), f32, 16, "wide_u8")
        call("dd_stitch6_u8", frames, wide_u8, b, h, w)
        wide_bf = arena.out((b, h, 6 * w, 4), bf16, 16, "wide_bf16")
        call("dd_stitch6_bf16", views, wide_bf, b, h, w)
        wide_bfm = arena.out((b, h, 6 * w, 4), bf16, 16, "wide_bf16_masked")
        tgt_m = arena.out((b, 3, h, w), f32, 16, "target_masked") if slot >= 0 else None
        call("dd_stitch6_bf16_masked", views, wide_bfm, tgt_m, b, h, w, slot)
        outs = arena.verify()
        u8_ref = nhwc4(wide_of(f0.permute(0, 1, 4, 2, 3).float() / 255))
        checks = [Check("wide_nhwc4", outs["wide_nhwc4"], nhwc4(ref), how="exact"), Check("wide_nchw", outs["wide_nchw"], ref, how="exact"),
                  Check("wide_u8", outs["wide_u8"], u8_ref, 1e-7, "abs"),
                  Check("wide_bf16", outs["wide_bf16"].float(), nhwc4(wide_of(v0)).to(bf16).float(), how="exact"),
                  Check("wide_bf16_masked", outs["wide_bf16_masked"].float(), nhwc4(ref).to(bf16).float(), how="exact")]
        if slot >= 0:
            checks += [Check("target", outs["target"], tgt_ref, how="exact"), Check("target_masked", outs["target_masked"], tgt_ref, how="exact")]
        return checks
    return fn


_STITCH = ("dd_stitch6", "dd_stitch6_u8", "dd_stitch6_bf16", "dd_stitch6_bf16_masked")
for _b, _h, _w, _slot in ((2, 5, 7, -1), (3, 16, 22, 2), (1, 9, 306, 4)):      # tests/test_gpu_parity.py::test_stitch6
    case(f"dd_stitch6+u8+bf16+masked[{_b},{_h},{_w},slot={_slot}]", _STITCH)(_stitch(_b, _h, _w, _slot))


def _view(b, h, w, view, tf):
    def fn(arena, mode):
        v0 = hu((b, 6, 3, h, w), "views", 0.0, 1.0)
        x = v0[:, view]
        x = (x, torch.rot90(x, 1, [2, 3]), torch.rot90(x, 1, [3, 2]), torch.flip(x, [2, 3]))[tf]
        views = arena.put(v0, 16, "views")
        out = arena.out((b, x.shape[2], x.shape[3], 4), f32, 16, "out")
        call("dd_view_to_nhwc4", views, out, b, h, w, view, tf)
        return [Check("out", arena.verify()["out"], nhwc4(x.contiguous()), how="exact")]
    return fn


for _view_i, _tf in ((0, 0), (4, 1), (1, 2), (5, 3)):      # the four transforms SpatialMappingCNN applies, on the views it applies them to
    case(f"dd_view_to_nhwc4[2,5,7,view={_view_i},transform={_tf}]", "dd_view_to_nhwc4")(_view(2, 5, 7, _view_i, _tf))


@case("dd_subsample_nhwc4[2,20x23 -> 8x9, stride 3, offset -1]", "dd_subsample_nhwc4")
def _subsample(arena, mode):
    b, h, w, oh, ow, stride, off = 2, 20, 23, 8, 9, 3, -1
    s0 = hu((b, h, w), "subs")
    src, dst = arena.put(s0, 16, "src"), arena.out((b, oh, ow, 4), f32, 16, "dst")
    call("dd_subsample_nhwc4", src, dst, b, h, w, oh, ow, stride, off)
    want = torch.zeros(b, oh, ow, 4)
    for u in range(oh):
        for v in range(ow):
            y, x = stride * u + off, stride * v + off
            if 0 <= y < h and 0 <= x < w:      # zero outside the image
                want[:, u, v, 0] = s0[:, y, x]
    return [Check("dst", arena.verify()["dst"], want, how="exact")]


# ------------------------------------------------------------------------------------------------ max_pool1d(4) in NCHW order
def _pool_ref(b, c, h, w, ties):
    feat = torch.relu(hu((b, c, h, w), f"pf{c}{h}{w}"))
    if ties:
        feat = (feat * 4).round() / 4      # many ties and all-zero windows
    feat.requires_grad_(True)
    ref = F.max_pool1d(feat.reshape(b, 1, -1), 4).squeeze(1)
    gp = hu(tuple(ref.shape), f"pg{c}{h}{w}")
    ref.backward(gp)
    return feat.detach(), ref.detach(), gp, feat.grad * (feat.detach() > 0)


def _pool4(b, c, h, w):
    def fn(arena, mode):
        feat0, ref, gp0, dref = _pool_ref(b, c, h, w, ties=False)
        feat = arena.put(nhwc(feat0), 16, "feat")
        pooled = arena.out(tuple(ref.shape), f32, 16, "pooled")
        call("dd_pool4_fwd", feat, pooled, b, h, w, c)
        gp = arena.put(gp0, 16, "dpooled")
        dfeat = arena.out((b, h, w, c), f32, 16, "dfeat")
        call("dd_pool4_relu_bwd", gp, feat, dfeat, b, h, w, c)
        outs = arena.verify()
        return [Check("pooled", outs["pooled"], ref, how="exact"), Check("dfeat", nchw(outs["dfeat"]), dref, how="exact")]
    return fn


for _s in ((3, 32, 5, 7), (2, 32, 8, 11), (1, 8, 2, 2)):      # H*W % 4 != 0: the *_any kernels; the quad kernels; one quad
    case(f"dd_pool4_fwd+relu_bwd{list(_s)}", ("dd_pool4_fwd", "dd_pool4_relu_bwd"))(_pool4(*_s))


def _pool4_idx(b, c, h, w, cross):
    """cross: idx on 2 bytes in the minimal mode, which sends both launchers to the quad kernels (ALIGNMENT_PICKS)."""
    def fn(arena, mode):
        feat0, ref, gp0, dref = _pool_ref(b, c, h, w, ties=True)
        n = size("dd_pool4_idx_elems", b, h, w, c)
        assert n == b * (h * w // 4) * (c // 4)
        feat = arena.put(nhwc(feat0), 16, "feat")
        pooled = arena.out(tuple(ref.shape), f32, 16, "pooled")
        idx = arena.out((n,), i16, 2 if (cross and mode == "minimal") else 16, "idx")
        if cross:
            assert c == 32 and (idx.data_ptr() % 4 == 0) == (mode == "natural"), "one mode per kernel of csrc/layout_pool.hip:500 / :516"
        call("dd_pool4_fwd_idx", feat, pooled, idx, b, h, w, c)
        gp = arena.put(gp0, 16, "dpooled")
        dfeat = arena.out((b, h, w, c), f32, 16, "dfeat")
        call("dd_pool4_idx_relu_bwd", gp, idx, dfeat, b, h, w, c)
        outs = arena.verify()
        return [Check("pooled", outs["pooled"], ref, how="exact"), Check("dfeat", nchw(outs["dfeat"]), dref, how="exact")]
    return fn


case("dd_pool4_fwd_idx+idx_relu_bwd[2,32,8,11]", ("dd_pool4_fwd_idx", "dd_pool4_idx_relu_bwd"))(_pool4_idx(2, 32, 8, 11, False))
case("dd_pool4_fwd_idx+idx_relu_bwd[1,8,2,2]", ("dd_pool4_fwd_idx", "dd_pool4_idx_relu_bwd"))(_pool4_idx(1, 8, 2, 2, False))
case("dd_pool4_fwd_idx+idx_relu_bwd[2,32,8,11,tile32 | quad]", ("dd_pool4_fwd_idx", "dd_pool4_idx_relu_bwd"),
     crosses=("dd_pool4_fwd_idx", "dd_pool4_idx_relu_bwd"))(_pool4_idx(2, 32, 8, 11, True))


@case("dd_pool4_relu_bwd_add[2,32,8,11]", "dd_pool4_relu_bwd_add")
def _pool4_add(arena, mode):
    b, c, h, w = 2, 32, 8, 11
    feat0, ref, gp0, dref = _pool_ref(b, c, h, w, ties=True)
    g0 = hu((b, h, w, c), "pga")
    gp, feat, gfeat = arena.put(gp0, 16, "dpooled"), arena.put(nhwc(feat0), 16, "feat"), arena.put(g0, 16, "gfeat")
    dfeat = arena.out((b, h, w, c), f32, 16, "dfeat")
    call("dd_pool4_relu_bwd_add", gp, feat, gfeat, dfeat, b, h, w, c)
    # one fp32 add per element: (feat > 0) * (gfeat + routed), the fp64 sum rounded once
    want = ((g0.double() + nhwc(dref).double()) * (nhwc(feat0) > 0)).float()
    return [Check("dfeat", arena.verify()["dfeat"], want, how="exact")]


# ------------------------------------------------------------------------------------------------ sign words, padded ReLU backward, copies
def _bits(x):
    v = ((x > 0).to(torch.int64) << torch.arange(32)).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(i32)


def _sign_and_pad(b, h, w):
    def fn(arena, mode):
        x0 = hu((b, h + 2, w + 2, 32), f"sx{h}{w}")
        x0[0, 0, 0, :] = 0.0      # zero is not positive
        x = arena.put(x0, 16, "x")
        bits = arena.out((b, h + 2, w + 2), i32, 16, "bits")
        call("dd_relu_sign_bits", x, bits, b * (h + 2) * (w + 2))
        wide0 = hu((b, h, w, 96), f"sw{h}{w}")      # dy = channels [32, 64) of a 96-channel buffer, read where it lies
        wide = arena.put(wide0, 16, "dy_wide")
        out = arena.out((b, h + 2, w + 2, 32), f32, 16, "out_pad")
        call("dd_relu_bwd_pad_bits", wide, bits, out, b, h, w, 96, 32)
        outs = arena.verify()
        want = torch.zeros_like(x0)
        want[:, 1:-1, 1:-1] = wide0[..., 32:64] * (x0[:, 1:-1, 1:-1] > 0)
        return [Check("bits", outs["bits"], _bits(x0), how="exact"), Check("out_pad", outs["out_pad"], want, how="exact")]
    return fn


case("dd_relu_sign_bits+relu_bwd_pad_bits[2,5,7]", ("dd_relu_sign_bits", "dd_relu_bwd_pad_bits"))(_sign_and_pad(2, 5, 7))
case("dd_relu_sign_bits+relu_bwd_pad_bits[3,19,33]", ("dd_relu_sign_bits", "dd_relu_bwd_pad_bits"))(_sign_and_pad(3, 19, 33))


@case("dd_copy_channels[35 pixels, 8 of 16 -> 12]", "dd_copy_channels")
def _copy_channels(arena, mode):
    npix = 35
    s0, d0 = hu((npix, 16), "ccs"), hu((npix, 12), "ccd")
    src, dst = arena.put(s0, 16, "src"), arena.inout(d0, 16, "dst")
    call("dd_copy_channels", src, dst, npix, 8, 16, 4, 12, 4)
    want = d0.clone()
    want[:, 4:12] = s0[:, 4:12]
    return [Check("dst", arena.verify()["dst"], want, how="exact")]


@case("dd_copy_channels_window[2,5,7 from a padded buffer]", "dd_copy_channels_window")
def _copy_window(arena, mode):
    b, h, w = 2, 5, 7
    s0, d0 = hu((b, h + 2, w + 2, 32), "cws"), hu((b, h, w, 64), "cwd")
    src, dst = arena.put(s0, 16, "src"), arena.inout(d0, 16, "dst")
    call("dd_copy_channels_window", src, dst, b, h, w, 32, h + 2, w + 2, 1, 1, 32, 0, h, w, 0, 0, 64, 32)
    want = d0.clone()
    want[..., 32:] = s0[:, 1:-1, 1:-1, :]
    return [Check("dst", arena.verify()["dst"], want, how="exact")]


def _channel_sum(shape, coff, chans, accumulate):
    def fn(arena, mode):
        b0 = hu(shape, f"chs{shape[1]}")
        cstore = shape[3]
        crosses = cstore % 4 == 0 and cstore <= 256
        buf = arena.put(b0, 4 if mode == "minimal" else 16, "buf")      # the header: any alignment a float can have
        if crosses:
            assert (buf.data_ptr() % 16 == 0) == (mode == "natural"), "one mode per kernel of csrc/gconv.hip:1029"
        o0 = hu((chans,), "chso")
        out = arena.inout(o0, 16, "out") if accumulate else arena.out((chans,), f32, 16, "out")
        ws = arena.workspace(size("dd_channel_sum_workspace_bytes"), 16)
        call("dd_channel_sum", buf, out, shape[0] * shape[1] * shape[2], cstore, coff, chans, int(accumulate), ws)
        ref = b0.double().sum(dim=(0, 1, 2))[coff:coff + chans] + (o0.double() if accumulate else 0.0)
        scale = float(b0.double().abs().sum(dim=(0, 1, 2)).max())
        return [Check("out", arena.verify()["out"], ref, CHANNEL_SUM_TOL * scale, "abs")]
    return fn


for _shape, _coff, _ch in (((3, 16, 20, 96), 32, 32), ((1, 5, 7, 8), 0, 8), ((2, 9, 9, 4), 1, 2), ((1, 4, 6, 3), 0, 3), ((1, 1, 1, 32), 0, 32)):
    for _acc in (False, True):
        case(f"dd_channel_sum[{list(_shape)},coff={_coff},{_ch},accumulate={_acc}]", "dd_channel_sum",
             picks_kernel_by_alignment=_shape[3] % 4 == 0)(_channel_sum(_shape, _coff, _ch, _acc))


# ------------------------------------------------------------------------------------------------ fp32 <-> bf16
def _bf16_round_trip(n):
    def fn(arena, mode):
        x0 = hu((n,), f"bf{n}", -3.0, 3.0)
        x0[0] = 1.0 + 2.0 ** -8      # a tie: round to nearest even keeps 1.0
        src = arena.put(x0, 16, "src")
        half = arena.out((n,), bf16, 16, "bf16")
        call("dd_f32_to_bf16", src, half, n)
        back = arena.out((n,), f32, 16, "f32")
        call("dd_bf16_to_f32", half, back, n)
        outs = arena.verify()
        return [Check("bf16", outs["bf16"].view(i16), x0.to(bf16).view(i16), how="exact"), Check("f32", outs["f32"], x0.to(bf16).float(), how="exact")]
    return fn


for _n in (4, 4100):      # n % 4 == 0 is the contract
    case(f"dd_f32_to_bf16+bf16_to_f32[n={_n}]", ("dd_f32_to_bf16", "dd_bf16_to_f32"))(_bf16_round_trip(_n))


# ------------------------------------------------------------------------------------------------ bn2d.hip
def _bn2d(b, h, w, training):
    """dd_bn2d_stats -> dd_bn2d_finalize -> dd_bn2d_apply_relu -> dd_bn2d_bwd in one arena; the statistics table is exactly
    dd_conv_stats_floats() floats, left 0xFF: every row the finalize kernel reads must have been written by dd_bn2d_stats.
    Their numerics at offsets, past the grid cap and with gamma of either sign: tests/test_gpu_bn2d.py (and the whole-model three-way
    checks of tests/test_gpu_round2.py / test_gpu_round3.py); the bounds here are those of the BatchNorm1d kernels, which compute the same quantities
    (tests/test_gpu_parity.py::test_bn_relu_dropout: KERNEL_TOL, 10 x KERNEL_TOL for the gradients)."""
    def fn(arena, mode):
        eps, mom, npix = 1e-5, 0.1, b * h * w
        u64 = hu((b, h, w, 32), f"bn2u{h}{w}", -2.0, 2.0).double().requires_grad_(True)
        g64 = hu((32,), "bn2g", 0.5, 1.5).double().requires_grad_(True)
        be64 = hu((32,), "bn2b", -0.5, 0.5).double().requires_grad_(True)
        rm0, rv0 = hu((32,), "bn2rm", -0.3, 0.3), hu((32,), "bn2rv", 0.5, 1.5)
        rm64, rv64 = rm0.double().clone(), rv0.double().clone()
        z64 = F.batch_norm(u64.permute(0, 3, 1, 2), rm64, rv64, g64, be64, training, mom, eps).permute(0, 2, 3, 1)
        y64 = F.relu(z64)
        gy64 = hu((b, h, w, 32), f"bn2gy{h}{w}").double() * (y64.detach() > 0)      # g: already ReLU-masked
        z64.backward(gy64)
        u = arena.put(u64.detach().float(), 16, "u")
        nstats = size("dd_conv_stats_floats")
        stats = arena.workspace(nstats * 4, 16, "stats").view(f32)
        call("dd_bn2d_stats", u, stats, npix)
        gamma, beta = arena.put(g64.detach().float(), 16, "gamma"), arena.put(be64.detach().float(), 16, "beta")
        rm, rv = arena.inout(rm0, 16, "running_mean"), arena.inout(rv0, 16, "running_var")
        aff, sm, si = arena.out((128,), f32, 16, "affine"), arena.out((32,), f32, 16, "save_mean"), arena.out((32,), f32, 16, "save_invstd")
        call("dd_bn2d_finalize", stats, npix, gamma, beta, rm, rv, mom, eps, int(training), aff, sm, si)
        y = arena.out((b, h, w, 32), f32, 16, "y")
        call("dd_bn2d_apply_relu", u, aff, y, npix)
        g = arena.put(gy64.float(), 16, "g")
        du, dg, db = arena.out((b, h, w, 32), f32, 16, "du"), arena.out((32,), f32, 16, "dgamma"), arena.out((32,), f32, 16, "dbeta")
        ws = arena.workspace(size("dd_bn2d_workspace_bytes"), 16)
        call("dd_bn2d_bwd", g, u, gamma, sm, si, du, dg, db, npix, int(training), ws)
        outs = arena.verify()
        assert bool(torch.isfinite(stats.cpu()).all()), "dd_bn2d_stats must leave every row of the table defined"
        ud = u64.detach()
        mean = ud.mean((0, 1, 2)) if training else rm0.double()
        inv = 1 / ((ud.var((0, 1, 2), unbiased=False) if training else rv0.double()) + eps).sqrt()
        sc = g64.detach() * inv
        return [Check("y", outs["y"], y64, KERNEL_TOL), Check("du", outs["du"], u64.grad, 10 * KERNEL_TOL),
                Check("dgamma", outs["dgamma"], g64.grad, 10 * KERNEL_TOL), Check("dbeta", outs["dbeta"], be64.grad, 10 * KERNEL_TOL),
                Check("running_mean", outs["running_mean"], rm64, KERNEL_TOL), Check("running_var", outs["running_var"], rv64, KERNEL_TOL),
                Check("save_mean", outs["save_mean"], mean, KERNEL_TOL), Check("save_invstd", outs["save_invstd"], inv, KERNEL_TOL),
                Check("affine", outs["affine"], torch.cat([sc, be64.detach() - mean * sc] * 2), KERNEL_TOL)]
    return fn


for _b, _h, _w in ((2, 6, 10), (4, 16, 22)):
    for _tr in (True, False):
        case(f"dd_bn2d_stats+finalize+apply_relu+bwd[{_b},{_h},{_w},training={_tr}]",
             ("dd_bn2d_stats", "dd_bn2d_finalize", "dd_bn2d_apply_relu", "dd_bn2d_bwd"))(_bn2d(_b, _h, _w, _tr))


def _pool4_bn(b, h, w):
    """dd_pool4_bn_fwd / _bwd: the NCHW-order max_pool1d(4) over relu(u * scale + shift), the activation never stored.  Signed gamma, ties
    and a shape past the grid cap: tests/test_gpu_bn2d.py; the bound is KERNEL_TOL, as for dd_bn2d_apply_relu above (the same affine + ReLU, then a selection)."""
    def fn(arena, mode):
        u64 = hu((b, h, w, 32), f"pbu{h}{w}", -2.0, 2.0).double()
        aff64 = torch.cat([hu((32,), "pbsc", 0.5, 1.5), hu((32,), "pbsh", -0.5, 0.5)] * 2).double()
        feat = F.relu(u64 * aff64[:32] + aff64[32:64]).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        ref = F.max_pool1d(feat.reshape(b, 1, -1), 4).squeeze(1)
        gp64 = hu(tuple(ref.shape), f"pbg{h}{w}").double()
        ref.backward(gp64)
        dref = feat.grad * (feat.detach() > 0)
        u, aff = arena.put(u64.float(), 16, "u"), arena.put(aff64.float(), 16, "affine")
        pooled = arena.out(tuple(ref.shape), f32, 16, "pooled")
        call("dd_pool4_bn_fwd", u, aff, pooled, b, h, w)
        gp = arena.put(gp64.float(), 16, "dpooled")
        dfeat = arena.out((b, h, w, 32), f32, 16, "dfeat")
        call("dd_pool4_bn_bwd", gp, u, aff, dfeat, b, h, w)
        outs = arena.verify()
        return [Check("pooled", outs["pooled"], ref.detach(), KERNEL_TOL), Check("dfeat", nchw(outs["dfeat"]), dref, KERNEL_TOL)]
    return fn


for _b, _h, _w in ((2, 6, 10), (4, 16, 22), (1, 2, 2)):      # H*W % 4 == 0 is the contract
    case(f"dd_pool4_bn_fwd+bwd[{_b},{_h},{_w}]", ("dd_pool4_bn_fwd", "dd_pool4_bn_bwd"))(_pool4_bn(_b, _h, _w))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
