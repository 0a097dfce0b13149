"""Guard-band cases (tests/_guard.py) for the ``gconv.Layer`` family -- the generic engine (csrc/gconv.hip), the dilated kernels
(csrc/dconv.hip, dconv_t.hip, dconv_m.hip) and what ``Layer`` dispatches to them -- driven through ``gconv.View`` objects as the box
heads and the decoder drive them: one ragged row of tests/test_gpu_gconv.py::CASES per layer kind plus one full-width row, forward,
data gradient (plain and with ``relu_src``) and weight gradient, at that file's TOL against fp64 torch.

Every input / output View sits inside a wider arena buffer with ``coff = 8`` and ``cstore = c + 16``: the neighbouring channels
are inline guards (pre-filled, compared exactly afterwards) on top of the 64 KiB gaps.  What ``Layer`` allocates itself (packed
weights, weight-gradient outputs, workspaces, the sub-kernels of the phased data gradient) is redirected into the arena by
``Redirect``, which stands in for ``gconv.call``: an operand outside the arena is mirrored by an arena operand of the same size --
an input (a ``const`` pointer of the header) copied in, an output or workspace left 0xFF -- so these too run at 16-byte alignment,
exactly as large as ``Layer`` asked its queries, between guards.  ``Redirect`` also records the entry points a row reaches: each
case asserts that its row runs the kernels it is listed for (``Layer``'s dispatch predicates -- dd_dconv_supported through
``_dconv_ok``, dd_dconv_wgrad_supported -- decided as in production), so a row cannot silently test the generic engine.

An over-read whose value is discarded cannot be seen by these tests.

Run time on an MI355X: see tests/test_gpu_guard_layout.py (the guard files are timed together)."""
import os
import re

import pytest
import torch
from torch import nn
from torch.nn import functional as F

from _guard import Case, Check, run_case
from test_gpu_gconv import CASES as LAYER_ROWS, TOL, to_nhwc

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

COFF, EXTRA = 8, 16      # every View: channels [8, 8 + c) of c + 16 stored ones (the split-product and column-sum rows: whole buffers)
COLSUM_TOL = 2e-6        # tests/test_gpu_gconv.py::test_channel_sum: of the largest per-channel sum of absolute values


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def hu(shape, name, lo=-1.0, hi=1.0):
    return synth.hash_uniform(shape, synth.key_salt(name), lo, hi)


def pointer_params(name, _cache={}):
    """[(is_pointer, is_const, parameter name)] of a launch function, in header order without the stream."""
    if not _cache:
        from driving_dirty_amd.build import HEADER
        text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
        for m in re.finditer(r"\bint\s+(dd_\w+)\s*\(([^;{]*?)\)\s*;", text):
            params = []
            for p in m.group(2).split(","):
                p = " ".join(p.split())
                params.append(("*" in p, p.startswith("const "), re.findall(r"\w+", p)[-1]))
            _cache[m.group(1)] = params[:-1] if params and params[-1][2] == "stream" else params
    return _cache[name]


class Redirect:
    """Stands in for ``gconv.call``: see the module docstring."""

    def __init__(self, arena, inout=()):
        """inout: parameter names whose mirrors take over what the caller's tensor holds (outputs an entry point is documented to
        write only in part)."""
        self.arena, self.mirrors, self.called, self.keep, self.inout = arena, {}, [], [], frozenset(inout)
        self.lo = arena.buf.data_ptr()
        self.hi = self.lo + arena.buf.numel()

    def __call__(self, name, *operands):
        from driving_dirty_amd import _lib
        self.called.append(name)
        params = pointer_params(name)
        assert len(params) == len(operands), (name, len(params), len(operands))
        out = []
        for (is_ptr, const, pname), a in zip(params, operands):
            if isinstance(a, torch.Tensor) and a.is_cuda and not (self.lo <= a.data_ptr() < self.hi):
                assert is_ptr and a.is_contiguous(), (name, pname)
                key = a.data_ptr()
                if key not in self.mirrors:
                    self.keep.append(a)      # alive until the end of the case: the allocator hands its address to nothing else
                    label = f"{name}.{pname}#{len(self.mirrors)}"
                    if const:
                        view = self.arena.put(a, 16, label)
                    elif pname in self.inout:
                        view = self.arena.inout(a, 16, label)
                    elif pname == "workspace":
                        view = self.arena.workspace(a.numel() * a.element_size(), 16, label)
                    else:      # a packed image may have slots no kernel reads; every other output must come back finite
                        view = self.arena.out(tuple(a.shape), a.dtype, 16, label, check_finite=pname != "packed")
                    self.mirrors[key] = (view, a, label, const)
                a = self.mirrors[key][0]
            out.append(a)
        _lib.call(name, *out)

    def finish(self):
        """verify(), then hand what the mirrored outputs hold back to the tensors ``Layer`` returned."""
        outs = self.arena.verify()
        for view, orig, label, const in self.mirrors.values():
            if label in outs:
                orig.copy_(outs[label])
        return outs


# row of tests/test_gpu_gconv.py::CASES -> the entry points the row must reach (Layer's dispatch, recorded on an MI355X)
EXPECT = {
    "strip_1x50": ("dd_gconv_pack", "dd_gconv_fwd", "dd_gconv_wgrad"), "strip_52x1": ("dd_gconv_pack", "dd_gconv_fwd", "dd_gconv_wgrad"),
    "out_conv_k3": ("dd_dconv_pack", "dd_dconv_fwd", "dd_gconv_wgrad"), "ss_conv_1x24_s7": ("dd_gconv_pack", "dd_gconv_fwd", "dd_gconv_wgrad"),
    "rm_conv_1_k7s3d3": ("dd_gconv_pack", "dd_gconv_fwd", "dd_gconv_wgrad"), "rm_conv_2_k3d3": ("dd_dconv_pack", "dd_dconv_fwd", "dd_gconv_wgrad"),
    "up1_96_64_k7d7": ("dd_dconv_pack", "dd_dconv_fwd", "dd_dconv_wgrad", "dd_channel_sum"),
    "up3_17_two_tiles": ("dd_dconv_pack", "dd_dconv_fwd", "dd_gconv_wgrad", "dd_channel_sum"),
    "up4_31_gather": ("dd_dconv_pack", "dd_dconv_fwd", "dd_dconv_wgrad", "dd_channel_sum"),
    "up4_cout4": ("dd_dconv_pack", "dd_dconv_fwd", "dd_gconv_pack", "dd_gconv_fwd", "dd_gconv_wgrad", "dd_channel_sum"),
    "dc1_64_32_k3p1": ("dd_dconv_pack", "dd_dconv_fwd", "dd_gconv_wgrad", "dd_channel_sum"),
    "dc3_k2s2": ("dd_gconv_pack", "dd_gconv_fwd", "dd_gconv_wgrad"), "dc4_32_3_k1": ("dd_gconv_pack", "dd_gconv_fwd", "dd_gconv_wgrad"),
    "bm_up1_64_32_k8d8": ("dd_dconv_pack", "dd_dconv_fwd", "dd_dconv_wgrad", "dd_channel_sum"),
    "bm_up3_k6d6_op2": ("dd_dconv_pack", "dd_dconv_fwd", "dd_dconv_wgrad", "dd_channel_sum"),
    "up1_ragged_250": ("dd_dconv_pack", "dd_dconv_fwd", "dd_dconv_wgrad", "dd_channel_sum"),
}
ROWS = ("strip_1x50", "strip_52x1", "out_conv_k3", "ss_conv_1x24_s7", "rm_conv_1_k7s3d3", "rm_conv_2_k3d3", "up1_96_64_k7d7",
        "up3_17_two_tiles", "up4_31_gather", "up4_cout4", "dc1_64_32_k3p1", "dc3_k2s2", "dc4_32_3_k1", "bm_up1_64_32_k8d8",
        "bm_up3_k6d6_op2", "up1_ragged_250")


def _layer(name, make, shape, whole=False, split=False, colsum=False, expect=None):
    """whole: Views that cover their buffers (coff 0, no extra channels) -- what the split-product kernels and the column-sum
    epilogue are built for; split: inside ``gconv.split_products(True)``; colsum: one more masked data gradient that also leaves
    the per-channel sums of what it wrote (dd_dconv_fwd_colsum)."""
    COFF, EXTRA = (0, 0) if whole else (8, 16)
    expect = EXPECT[name] if expect is None else expect

    def slab(arena, data, c_real, c_store, name, kind):
        """[B,H,W,c_store + EXTRA] filled with hash noise, ``data`` (NCHW) in channels [COFF, COFF + c_real) (zero up to c_store)."""
        b, _, h, w = data.shape
        full = hu((b, h, w, c_store + EXTRA), "slab" + name, -3.0, 3.0)
        full[..., COFF:COFF + c_store] = to_nhwc(data.float(), c_store)
        return (arena.put if kind == "in" else arena.inout)(full, 16, name), full

    def guards_of(t, c_store):
        return torch.cat([t[..., :COFF], t[..., COFF + c_store:]], dim=3)

    def fn(arena, mode):
        from driving_dirty_amd import gconv
        mod = synth.fill_module(make(), seed=21).double()
        x = hu(shape, "gx" + name, 0.0, 1.0).double().requires_grad_(True)
        y_ref = F.relu(mod(x))
        gy = hu(tuple(y_ref.shape), "gg" + name).double()
        gy_m = gy * (y_ref > 0)
        y_ref.backward(gy)
        tr = isinstance(mod, nn.ConvTranspose2d)
        layer = gconv.Layer(mod.in_channels, mod.out_channels, mod.kernel_size, mod.stride, mod.dilation, mod.padding,
                            transposed=tr, output_padding=mod.output_padding if tr else 0)
        b, cin, h, w = shape
        cout = mod.out_channels
        oh, ow = layer.out_hw(h, w)
        cis, cos = (cin + 3) // 4 * 4, (cout + 3) // 4 * 4
        xm = (x.detach() - 0.5).float()
        xb, _ = slab(arena, x.detach(), cin, cis, "x", "in")
        wd, bd = arena.put(mod.weight.detach().float(), 16, "weight"), arena.put(mod.bias.detach().float(), 16, "bias")
        yb, y0 = slab(arena, torch.zeros(b, cout, oh, ow), cout, cos, "y", "inout")
        gb, _ = slab(arena, gy_m, cout, cos, "dy", "in")
        dxb, dx0 = slab(arena, torch.zeros(b, cin, h, w), cin, cis, "dx", "inout")
        mb, _ = slab(arena, xm, cin, cis, "relu_src", "in")
        dxm, _ = slab(arena, torch.zeros(b, cin, h, w), cin, cis, "dx_masked", "inout")
        if colsum:
            dxc, _ = slab(arena, torch.zeros(b, cin, h, w), cin, cis, "dx_colsum", "inout")
            sums = arena.out((cin,), torch.float32, 16, "colsum")
        red, real = Redirect(arena), gconv.call
        gconv.call = red
        try:
            with gconv.split_products(split):
                layer.forward(wd, bd, gconv.View(xb, COFF, cis), gconv.View(yb, COFF, cout), gconv.EPI_BIAS_RELU)
                if split:
                    assert layer.split_wgrad_ok(gconv.View(xb, COFF, cis), gconv.View(gb, COFF, cout))
                dw, db = layer.backward_weight(gconv.View(xb, COFF, cis), gconv.View(gb, COFF, cout))
                layer.backward_data(wd, gconv.View(gb, COFF, cos), gconv.View(dxb, COFF, cin))
                layer.backward_data(wd, gconv.View(gb, COFF, cos), gconv.View(dxm, COFF, cin), relu_src=mb)
                if colsum:      # True: dd_dconv_colsum_supported accepted the descriptor and the sums were written
                    assert layer.backward_data(wd, gconv.View(gb, COFF, cos), gconv.View(dxc, COFF, cin), relu_src=mb, colsum=sums) is True
        finally:
            gconv.call = real
        outs = red.finish()
        called = set(red.called)
        print(f"REACHED {name}: {sorted(called)}")
        if os.environ.get("DD_GUARD_DISCOVER") != "1":
            assert set(expect) <= called, (name, "does not reach", sorted(set(expect) - called))
        sl = lambda t, c: t[..., COFF:COFF + c].permute(0, 3, 1, 2)
        more = []
        if colsum:
            masked = x.grad * (xm > 0)
            more = [Check("dx beside the column sums", outs["dx_colsum"], outs["dx_masked"], how="exact"),
                    Check("colsum", outs["colsum"], masked.sum(dim=(0, 2, 3)), COLSUM_TOL * float(masked.abs().sum(dim=(0, 2, 3)).max()), "abs")]
        return more + [Check("y", sl(outs["y"], cout), y_ref, TOL), Check("y: neighbouring channels", guards_of(outs["y"], cos), guards_of(y0, cos), how="exact"),
                Check("dw", dw.cpu(), mod.weight.grad, TOL), Check("db", db.cpu(), mod.bias.grad, TOL),
                Check("dx", sl(outs["dx"], cin), x.grad, TOL), Check("dx: neighbouring channels", guards_of(outs["dx"], cis), guards_of(dx0, cis), how="exact"),
                Check("dx masked", sl(outs["dx_masked"], cin), x.grad * (xm > 0), TOL)]
    return fn


CASES = []
_by_name = {r[0]: r for r in LAYER_ROWS}
for _name in ROWS:
    CASES.append(Case(f"Layer[{_name}]", EXPECT[_name], _layer(*_by_name[_name]), capacity=256 << 20))
# the split-product experiment (csrc/dconv_split.hip; bound: the exact kernels' own, tests/test_gpu_round4.py::
# test_split_bf16_forward_and_data_gradient_against_fp64_and_the_exact_kernels) and the data gradient with column sums (csrc/dconv_m.hip)
SPLIT = ("dd_dconv_split_input", "dd_dconv_split_pack", "dd_dconv_fwd_split", "dd_dconv_split_rows", "dd_dconv_wgrad_split")
for _name in ("up1_96_64_k7d7", "up1_ragged_250", "up2_64_32_k7d7"):
    CASES.append(Case(f"Layer[{_name},split products]", SPLIT, _layer(*_by_name[_name], whole=True, split=True, expect=SPLIT), capacity=256 << 20))
# dd_dconv_colsum_supported (csrc/dconv_m.hip, dd_dconv_mwin_takes): k7 d7, 17 to 64 gradient channels, at least 7 rows -- the smallest
# shapes it accepts, one with a ragged width
_COLSUM_ROWS = (("up2_7x20", lambda: nn.ConvTranspose2d(64, 32, 7, dilation=7), (1, 64, 7, 20)),
                ("up3_8x33", lambda: nn.ConvTranspose2d(32, 16, 7, dilation=7), (2, 32, 8, 33)))
for _row in _COLSUM_ROWS:
    CASES.append(Case(f"Layer[{_row[0]},column sums]", ("dd_dconv_fwd_colsum",), _layer(*_row, whole=True, colsum=True, expect=("dd_dconv_fwd_colsum",)),
                      capacity=256 << 20))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
