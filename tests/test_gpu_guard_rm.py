"""Guard-band cases (tests/_guard.py) for the road-map and strip kernels of the box heads: csrc/conv1ch.hip (dd_conv1ch_fwd, _wgrad, their
phase-major forms, dd_phase3_scatter / _gather) through the ``ops`` wrappers with every allocation of theirs redirected into the
arena (``Redirect`` of tests/test_gpu_guard_gconv.py), and csrc/strip6.hip (dd_strip6_fwd, dd_strip6_wgrad) called directly with
pointer tables built from arena views.  References and bounds: fp64 torch at tests/test_gpu_gconv.py's TOL for the dense 7x7
layer, the phase-major forms bit for bit against the dense ones (tests/test_gpu_round5.py::
test_phase_major_rm_conv_1_and_the_scatter_gather_pair), the strips at 2e-6 / 2e-5 of the peak (tests/test_gpu_round5.py::
test_strip6_forward_and_weight_gradient_against_fp64).  What a case asserts besides: tests/test_gpu_guard_dense.py.

An over-read whose value is discarded cannot be seen by these tests.

Run time on an MI355X: see tests/test_gpu_guard_layout.py (the guard files are timed together)."""
import pytest
import torch
from torch.nn import functional as F

from _guard import Case, Check, ptr_table, run_case
from test_gpu_gconv import TOL
from test_gpu_guard_gconv import Redirect
from test_gpu_round5 import _strip_reference

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

STRIP_FWD_TOL, STRIP_GRAD_TOL = 2e-6, 2e-5
f32, i32 = torch.float32, torch.int32


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


CASES = []


def _rm_conv_1(b, sh, sw):
    def fn(arena, mode):
        from driving_dirty_amd import heads, ops
        dev = arena.dev
        rm = hu((b, sh, sw), f"rm{sh}{sw}", 0.0, 1.0)
        w0, b0 = hu((32, 1, 7, 7), "rmw", -0.4, 0.4), hu((32,), "rmb", -0.4, 0.4)
        y64 = F.relu(F.conv2d(rm.double().unsqueeze(1), w0.double(), b0.double()))
        oh, ow = y64.shape[2:]
        g0 = hu((b, oh, ow, 32), f"rmg{sh}{sw}")
        w64 = w0.double().requires_grad_(True)
        b64 = b0.double().requires_grad_(True)
        (F.conv2d(rm.double().unsqueeze(1), w64, b64) * g0.double().permute(0, 3, 1, 2)).sum().backward()
        rm4 = torch.zeros(b, sh, sw, 4)
        rm4[..., 0] = rm
        taps, wd, bd, g = arena.put(rm4, 16, "taps4"), arena.put(w0, 16, "w"), arena.put(b0, 16, "bias"), arena.put(g0, 16, "g")
        ph, pw = (oh + 2) // 3, (ow + 2) // 3
        padded0 = hu((9 * b, ph + 2, pw + 2, 32), f"rmp{sh}{sw}")
        padded = arena.put(padded0, 16, "padded_phase")
        wide0 = hu((b, oh, ow, 96), f"rmwide{sh}{sw}")
        wide = arena.inout(wide0, 16, "wide")      # the scatter writes channels [64, 96): the rest are inline guards
        red, real = Redirect(arena), ops.call
        ops.call = red
        try:
            dense = ops.conv1ch_fwd(taps, wd, bd, relu=True)
            yp, bits = ops.conv1ch_fwd_phase3(taps, wd, bd, relu=True)
            gp = ops.phase3_gather(g, 0, ph, pw, 0)
            dw, db = ops.conv1ch_wgrad(taps, g)
            dwp, dbp = ops.conv1ch_wgrad_phase3(taps, gp)
            ops.phase3_scatter(padded, wide, 64, 1)
            back = ops.phase3_gather(wide, 64, ph + 2, pw + 2, 1)
        finally:
            ops.call = real
        outs = red.finish()
        want = {"dd_conv1ch_fwd", "dd_conv1ch_fwd_phase3", "dd_conv1ch_wgrad", "dd_conv1ch_wgrad_phase3", "dd_phase3_scatter", "dd_phase3_gather"}
        assert want <= set(red.called), want - set(red.called)
        dense, yp, bits, gp, dw, db, dwp, dbp, back = (t.cpu() for t in (dense, yp, bits, gp, dw, db, dwp, dbp, back))
        unphase = heads.MergeFn._dense_from_phase3
        want_bits = ((yp > 0).long() << torch.arange(32)).sum(-1)
        want_bits = torch.where(want_bits >= 2 ** 31, want_bits - 2 ** 32, want_bits).to(i32)
        return [Check("dense y", dense.permute(0, 3, 1, 2), y64, TOL), Check("dw", dw, w64.grad, TOL), Check("dbias", db, b64.grad, TOL),
                Check("phase-major y", unphase(yp, oh, ow), dense, how="exact"), Check("sign words", bits, want_bits, how="exact"),
                Check("gathered g", unphase(gp, oh, ow), g0, how="exact"), Check("phase-major dw", dwp, dw, how="exact"),
                Check("phase-major dbias", dbp, db, how="exact"),
                Check("scattered slice", outs["wide"][..., 64:], unphase(padded0[:, 1:, 1:].contiguous(), oh, ow), how="exact"),
                Check("channels beside the slice", outs["wide"][..., :64], wide0[..., :64], how="exact"),
                Check("gathered back", unphase(back[:, 1:, 1:].contiguous(), oh, ow), outs["wide"][..., 64:], how="exact"),
                Check("gather's border cells", torch.cat([back[:, 0].reshape(-1), back[:, :, 0].reshape(-1)]),
                      torch.zeros(back[:, 0].numel() + back[:, :, 0].numel()), how="exact")]
    return fn


_RM = ("dd_conv1ch_fwd", "dd_conv1ch_fwd_phase3", "dd_conv1ch_wgrad", "dd_conv1ch_wgrad_phase3", "dd_phase3_scatter", "dd_phase3_gather")
for _b, _sh, _sw in ((2, 40, 46), (3, 19, 33)):      # the smallest of the existing test: classes of unequal size, several images
    CASES.append(Case(f"dd_conv1ch+phase3[{_b},{_sh},{_sw}]", _RM, _rm_conv_1(_b, _sh, _sw), capacity=64 << 20))


def _strip6(h, w, batch):
    def fn(arena, mode):
        from driving_dirty_amd import _lib
        assert _lib.lib().dd_strip6_supported(h, w)
        views0 = hu((batch, 6, 3, h, w), f"s6v{h}", 0.0, 1.0)
        shapes = [(32, 3, 1, 50), (32, 3, 1, 50), (32, 3, 52, 1), (32, 3, 52, 1), (32, 3, 1, 50), (32, 3, 1, 50)]
        ws0 = [hu(s, f"s6w{i}", -0.1, 0.1) for i, s in enumerate(shapes)]
        bs0 = [hu((32,), f"s6b{i}", -0.1, 0.1) for i in range(6)]
        th, tw = (h - 1) // 3 + 1, (w - 50) // 2 + 1
        gm0 = hu((batch, 3 * th, 2 * tw, 32), f"s6g{h}", -0.5, 0.5)
        w64, b64 = [x.double().requires_grad_(True) for x in ws0], [x.double().requires_grad_(True) for x in bs0]
        pre = _strip_reference(views0.double(), w64, b64)
        (pre * gm0.double().permute(0, 3, 1, 2)).sum().backward()
        samples = [arena.put(views0[i], 16, f"sample{i}") for i in range(batch)]      # one allocation per sample, as the collate hands them over
        ws = [arena.put(x, 16, f"weight{i}") for i, x in enumerate(ws0)]
        bs = [arena.put(x, 16, f"bias{i}") for i, x in enumerate(bs0)]
        mosaic, bits = arena.out((batch, 3 * th, 2 * tw, 32), f32, 16, "mosaic"), arena.out((batch, 3 * th, 2 * tw), i32, 16, "relu_bits")
        call("dd_strip6_fwd", ptr_table(samples), 0, ptr_table(ws), ptr_table(bs), mosaic, bits, batch, h, w)
        g = arena.put(gm0, 16, "g")
        dws = [arena.out(s, f32, 16, f"dweight{i}") for i, s in enumerate(shapes)]
        dbs = [arena.out((32,), f32, 16, f"dbias{i}") for i in range(6)]
        nbytes = size("dd_strip6_wgrad_workspace_bytes")
        wsp = arena.workspace(nbytes, 16)
        call("dd_strip6_wgrad", ptr_table(samples), 0, g, ptr_table(dws), ptr_table(dbs), batch, h, w, wsp, nbytes)
        outs = arena.verify()
        want_bits = ((outs["mosaic"] > 0).long() << torch.arange(32)).sum(-1)
        want_bits = torch.where(want_bits >= 2 ** 31, want_bits - 2 ** 32, want_bits).to(i32)
        checks = [Check("mosaic", outs["mosaic"], pre.relu().permute(0, 2, 3, 1).detach(), STRIP_FWD_TOL), Check("relu_bits", outs["relu_bits"], want_bits, how="exact")]
        for i in range(6):
            checks += [Check(f"dweight{i}", outs[f"dweight{i}"], w64[i].grad, STRIP_GRAD_TOL), Check(f"dbias{i}", outs[f"dbias{i}"], b64[i].grad, STRIP_GRAD_TOL)]
        return checks
    return fn


CASES.append(Case("dd_strip6_fwd+wgrad[64,114,batch 2]", ("dd_strip6_fwd", "dd_strip6_wgrad"), _strip6(64, 114, 2), capacity=64 << 20))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
