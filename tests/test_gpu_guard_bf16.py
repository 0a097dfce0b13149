"""Guard-band cases (tests/_guard.py) for the bf16 encoder kernels of csrc/conv3x3_bf16.hip: dd_conv_bf16_pack / _fwd / _dgrad /
_wgrad and the four dd_pool4_bf16 entry points, at the smallest shapes of tests/test_gpu_bf16.py and with its criteria: activations
within one bf16 ulp of the fp64 oracle on the bf16-rounded inputs (``assert_bf16_close``), weight gradients at 2e-5 of the peak, the
pool exact.  The header asks for 16-byte aligned bf16 buffers and no more; the LDS transposes and tile fills run here at exactly
that.  What a case asserts besides: tests/test_gpu_guard_dense.py.  None of these launchers picks a kernel by address.

An over-read whose value is discarded cannot be seen by these tests.

Run time on an MI355X: see tests/test_gpu_guard_layout.py (the guard files are timed together)."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F
from torch.nn import grad as nngrad

from _guard import Case, Check, run_case
from test_gpu_bf16 import assert_bf16_close, bf16r

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

WGRAD_TOL = 2e-5      # tests/test_gpu_bf16.py::test_conv_fwd_dgrad_wgrad: of the peak (dbias: peak at least 1e-3)
f32, i32, i16, bf16 = torch.float32, torch.int32, torch.int16, torch.bfloat16
PACK_FWD, PACK_DGRAD_S1, PACK_DGRAD_S2 = 0, 1, 2


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


def _conv(b, h, w, cin, stride):
    def fn(arena, mode):
        from driving_dirty_amd import _lib
        x0 = bf16r(hu((b, cin, h, w), "x", 0.0, 1.0))
        wt0, bias0 = hu((32, cin, 3, 3), "w", -0.2, 0.2), hu((32,), "b", -0.1, 0.1)
        wr = bf16r(wt0).double()
        ref = bf16r(F.relu(F.conv2d(x0.double(), wr, bias0.double(), stride=stride, padding=1)).float()).double()
        ho, wo = ref.shape[2:]
        g0 = bf16r(hu((b, 32, ho, wo), "g"))
        desc = _lib.ConvDesc(b, h, w, cin, 4 if cin == 3 else cin, 32, 3, stride, 1, 0)
        cs = desc.cin_store
        xs = torch.zeros(b, h, w, cs)
        xs[..., :cin] = nhwc(x0)
        x = arena.put(xs.to(bf16), 16, "x")
        wd, bd = arena.put(wt0, 16, "weight"), arena.put(bias0, 16, "bias")
        n = size("dd_conv_bf16_packed_elems", desc)
        pf = arena.workspace(2 * n, 16, "packed_fwd")      # exactly the elements of the query, left 0xFF
        call("dd_conv_bf16_pack", wd, desc, PACK_FWD, pf)
        y, bits = arena.out((b, ho, wo, 32), bf16, 16, "y"), arena.out((b, ho, wo), i32, 16, "relu_bits")
        call("dd_conv_bf16_fwd", x, pf, bd, y, bits, desc)
        g = arena.put(nhwc(g0).to(bf16), 16, "dy")
        nbytes = size("dd_conv_bf16_wgrad_workspace_bytes", desc)
        ws = arena.workspace(nbytes, 16, "wgrad_workspace")
        dw, db = arena.out((32, cin, 3, 3), f32, 16, "dweight"), arena.out((32,), f32, 16, "dbias")
        call("dd_conv_bf16_wgrad", x, g, dw, db, desc, ws, nbytes)
        if cin == 32:
            mask = (hu((b, h, w, 32), "m") > 0).numpy()
            words = (mask.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=3).astype(np.uint32).view(np.int32)
            mbits = arena.put(torch.from_numpy(words), 16, "mask_bits")
            pd = arena.workspace(2 * n, 16, "packed_dgrad")
            call("dd_conv_bf16_pack", wd, desc, PACK_DGRAD_S1 if stride == 1 else PACK_DGRAD_S2, pd)
            dx = arena.out((b, h, w, 32), bf16, 16, "dx")
            call("dd_conv_bf16_dgrad", g, pd, mbits, dx, desc)
        outs = arena.verify()
        yf = outs["y"].float()
        assert_bf16_close(nchw(yf), ref, "forward")
        want_bits = ((yf > 0).long() << torch.arange(32)).sum(-1)
        want_bits = torch.where(want_bits >= 2 ** 31, want_bits - 2 ** 32, want_bits).to(i32)
        dw_ref = nngrad.conv2d_weight(x0.double(), wr.shape, g0.double(), stride=stride, padding=1)
        db_ref = g0.double().sum(dim=(0, 2, 3))
        checks = [Check("y", yf, nhwc(ref), how="asserted"), Check("relu_bits", outs["relu_bits"], want_bits, how="exact"),
                  Check("dweight", outs["dweight"], dw_ref, WGRAD_TOL), Check("dbias", outs["dbias"], db_ref, WGRAD_TOL, floor=1e-3)]
        if cin == 32:
            dx_ref = nngrad.conv2d_input((b, 32, h, w), wr, g0.double(), stride=stride, padding=1) * torch.from_numpy(mask).permute(0, 3, 1, 2)
            dx_ref = bf16r(dx_ref.float()).double()
            assert_bf16_close(nchw(outs["dx"].float()), dx_ref, "dgrad")
            checks.append(Check("dx", outs["dx"].float(), nhwc(dx_ref), how="asserted"))
        return checks
    return fn


_CONV = ("dd_conv_bf16_pack", "dd_conv_bf16_fwd", "dd_conv_bf16_wgrad")
for _b, _h, _w, _cin, _stride in ((1, 5, 40, 32, 1), (1, 2, 5, 32, 2), (1, 8, 33, 32, 2), (1, 3, 31, 3, 1), (1, 1, 64, 32, 1)):
    case(f"dd_conv_bf16[{_b},{_h},{_w},cin={_cin},stride={_stride}]", _CONV + (("dd_conv_bf16_dgrad",) if _cin == 32 else ()),
         capacity=96 << 20)(_conv(_b, _h, _w, _cin, _stride))


def _pool(b, h, w):
    def fn(arena, mode):
        feat0 = bf16r(hu((b, 32, h, w), "featt", -1.0, 1.0))
        flat = feat0.reshape(b, -1)
        flat[:, 0:4] = 0.25                                          # four equal values: the first takes the gradient
        flat[:, 4:8] = torch.tensor([-0.5, -0.25, -0.25, -1.0])      # negative maximum: the ReLU in front is closed
        flat[:, 8:12] = torch.tensor([0.0, -1.0, 0.0, -1.0])         # maximum exactly zero: closed as well
        flat[:, 12:16] = torch.tensor([0.5, 0.75, 0.75, 0.125])      # tie between positions 1 and 2
        ref = F.max_pool1d(feat0.reshape(b, 1, -1), 4).squeeze(1)
        gp0 = hu(tuple(ref.shape), "gpt")
        featr = feat0.clone().requires_grad_(True)
        F.max_pool1d(F.relu(featr).reshape(b, 1, -1), 4).squeeze(1).backward(gp0)
        dref = bf16r(featr.grad)
        feat, gp = arena.put(nhwc(feat0).to(bf16), 16, "feat"), arena.put(gp0, 16, "dpooled")
        pooled, dfeat = arena.out(tuple(ref.shape), f32, 16, "pooled"), arena.out((b, h, w, 32), bf16, 16, "dfeat")
        call("dd_pool4_bf16_fwd", feat, pooled, b, h, w, 32)
        call("dd_pool4_relu_bf16_bwd", gp, feat, dfeat, b, h, w, 32)
        n = size("dd_pool4_bf16_idx_elems", b, h, w, 32)
        pooled_i, idx = arena.out(tuple(ref.shape), f32, 16, "pooled_idx"), arena.out((n,), i16, 16, "idx")
        dfeat_i = arena.out((b, h, w, 32), bf16, 16, "dfeat_idx")
        call("dd_pool4_bf16_fwd_idx", feat, pooled_i, idx, b, h, w, 32)
        call("dd_pool4_idx_relu_bf16_bwd", gp, idx, dfeat_i, b, h, w, 32)
        outs = arena.verify()
        return [Check("pooled", outs["pooled"], ref, how="exact"), Check("dfeat", nchw(outs["dfeat"].float()), dref, how="exact"),
                Check("pooled (codes)", outs["pooled_idx"], ref, how="exact"), Check("dfeat (codes)", nchw(outs["dfeat_idx"].float()), dref, how="exact")]
    return fn


_POOL = ("dd_pool4_bf16_fwd", "dd_pool4_relu_bf16_bwd", "dd_pool4_bf16_fwd_idx", "dd_pool4_idx_relu_bf16_bwd")
for _b, _h, _w in ((2, 4, 6), (1, 8, 66), (3, 16, 130)):      # less than one 64-window tile, ragged last tiles
    case(f"dd_pool4_bf16[{_b},{_h},{_w}]", _POOL)(_pool(_b, _h, _w))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
