"""Guard-band cases (tests/_guard.py) for the dense part of the C ABI: csrc/dense.hip (losses, BatchNorm1d + ReLU + dropout), csrc/adam.hip,
csrc/mlp_tail.hip, csrc/adam_rankb.hip, csrc/gradnorm.hip, csrc/linear.hip, csrc/box_loss.hip.

Every case calls the entry point itself (``_lib.call``) on operands that are views into one 0xFF-filled arena, 64 KiB of guard on
both sides of each, the workspace exactly as large as its query says, once with every payload on a 256-byte boundary and once at
the alignment include/dd_hotpath.h asks for and no more.  Asserted per case: gaps untouched, inputs unchanged, outputs finite and
within the tolerance of the kernel's existing test (quoted where used) of an fp64 reference computed on the CPU, and the two
alignments bit-identical -- except for the launchers of ALIGNMENT_PICKS, which choose their kernel by the addresses; there the
minimal mode places the operands so that the other kernel runs, and the case asserts the launcher's own predicate on the addresses.

An over-read whose value is discarded cannot be seen by these tests.

Run time on an MI355X: see tests/test_gpu_guard_layout.py (the guard files are timed together)."""
import math

import pytest
import torch
from torch.nn import functional as F

from _guard import Case, Check, adam_table, ptr_table, run_case

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

KERNEL_TOL = 2e-5        # tests/test_gpu_parity.py: of the tensor's peak magnitude
LOSS_RTOL = 1e-6         # tests/test_gpu_parity.py::test_losses, tests/test_gpu_box_loss.py: relative error of a mean loss
TS_ATOL = 1e-6           # tests/test_gpu_parity.py::test_threat_score_and_validation_step
ADAM_P_TOL, ADAM_MV_TOL = 1e-6, 2e-6      # tests/test_gpu_parity.py::test_adam_matches_torch, tests/test_gpu_round5.py::test_adam_rankb_matches_fp64
COLSUM_ATOL = 1e-5       # tests/test_gpu_round5.py::test_column_sum_matches_fp64
GRAD_OF_PEAK, STATS_RTOL = 2e-5, 1e-6     # tests/test_gpu_box_loss.py
EPS52, EPS23 = 2.0 ** -52, 2.0 ** -23     # tests/test_gpu_grad_clip.py
f32, f64, u8, i64 = torch.float32, torch.float64, torch.uint8, torch.int64

# Launchers that pick a kernel by the alignment of their operands (found by reading every launcher of the files above):
ALIGNMENT_PICKS = {
    "dd_linear_wgrad": "csrc/linear.hip:554  k >= 512 && k % 4 == 0 && x % 16 == 0 && dw % 16 == 0 -> linear_wgrad_wide_kernel, else the scalar tiles",
    "dd_bn_relu_drop_fwd": "csrc/dense.hip dd_bn_relu_drop_fwd  rows <= 32 && feat >= 65536 && feat % 4 == 0 && every operand % 16 == 0 -> bn_relu_drop_fwd_vec4",
    "dd_bn_relu_drop_bwd": "csrc/dense.hip dd_bn_relu_drop_bwd  rows <= 32 && feat >= 65536 && feat % 2 == 0 && every operand % 8 == 0 -> bn_relu_drop_bwd_vec2",
}
# dd_column_sum (csrc/linear.hip:543) does not pick by address: n % 4 == 0 demands 16 bytes and n % 4 != 0 takes any; the kernel's
# branch is on n alone.  The two forms of the BatchNorm kernels sum over the rows in the same order, but the running statistics
# come out one rounding apart (the vector form's (1 - momentum) * running + momentum * batch contracts differently from the scalar
# form's): measured on running_mean at 3 x 65536, so these cases are held to fp64 on both sides and not to each other.


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


def case(name, entry, **kw):
    def deco(fn):
        CASES.append(Case(name, entry, fn, **kw))
        return fn
    return deco


# ------------------------------------------------------------------------------------------------ dense.hip: losses
def _bce_logits(n, kind, want_dz, want_probs, batch=None):
    """kind: 'f32' dd_bce_logits, 'u8' dd_bce_logits_u8, 'ptrs' dd_bce_logits_u8_ptrs (batch samples of n // batch)."""
    def fn(arena, mode):
        z64 = hu((n,), "gz", -6.0, 6.0).double()
        t64 = (hu((n,), "gt", 0.0, 1.0) < 0.3).double()
        z = arena.put(z64.float(), 16, "logits")
        if kind == "ptrs":
            per = n // batch
            masks = [arena.put(t64[i * per:(i + 1) * per].to(u8), 4, f"mask{i}") for i in range(batch)]
        else:
            t = arena.put(t64.to(u8) if kind == "u8" else t64.float(), 4 if kind == "u8" else 16, "target")
        loss = arena.out((1,), f32, 16, "loss_out")
        dz = arena.out((n,), f32, 16, "dlogits") if want_dz else None
        probs = arena.out((n,), f32, 16, "probs") if want_probs else None
        ws = arena.workspace(size("dd_loss_workspace_bytes", n), 16)
        if kind == "ptrs":
            call("dd_bce_logits_u8_ptrs", z, ptr_table(masks), batch, per, loss, dz, probs, 2.0, ws)
        else:
            call("dd_bce_logits_u8" if kind == "u8" else "dd_bce_logits", z, t, loss, dz, probs, n, 2.0, ws)
        outs = arena.verify()
        checks = [Check("loss", outs["loss_out"], F.binary_cross_entropy_with_logits(z64, t64).reshape(1), LOSS_RTOL, "scalar")]
        if want_dz:
            checks.append(Check("dlogits", outs["dlogits"], (torch.sigmoid(z64) - t64) * 2.0 / n, KERNEL_TOL))
        if want_probs:
            checks.append(Check("probs", outs["probs"], torch.sigmoid(z64), KERNEL_TOL))
        return checks
    return fn


for _n in (7, 4099):      # the n % 4 tails
    for _kind, _entry in (("f32", "dd_bce_logits"), ("u8", "dd_bce_logits_u8")):
        for _dz, _pr in ((True, True), (False, True), (True, False)):
            case(f"{_entry}[n={_n},dz={_dz},probs={_pr}]", _entry)(_bce_logits(_n, _kind, _dz, _pr))
for _dz, _pr in ((True, True), (False, True), (True, False)):
    case(f"dd_bce_logits_u8_ptrs[3x8,dz={_dz},probs={_pr}]", "dd_bce_logits_u8_ptrs")(_bce_logits(24, "ptrs", _dz, _pr, batch=3))


def _pair_loss(entry, n, want_grad):
    def fn(arena, mode):
        if entry == "dd_bce_probs":
            a64 = hu((n,), "gp", 0.02, 0.98).double()
            b64 = (hu((n,), "gt", 0.0, 1.0) < 0.3).double()
            ref = F.binary_cross_entropy(a64, b64)
            gref = (-(b64 / a64) + (1 - b64) / (1 - a64)) * 2.0 / n
        else:
            a64, b64 = hu((n,), "ga").double(), hu((n,), "gb").double()
            ref = F.mse_loss(a64, b64)
            gref = 2.0 * (a64 - b64) * 2.0 / n
        a, b = arena.put(a64.float(), 16, "a"), arena.put(b64.float(), 16, "b")
        loss = arena.out((1,), f32, 16, "loss_out")
        grad = arena.out((n,), f32, 16, "grad") if want_grad else None
        ws = arena.workspace(size("dd_loss_workspace_bytes", n), 16)
        call(entry, a, b, loss, grad, n, 2.0, ws)
        outs = arena.verify()
        checks = [Check("loss", outs["loss_out"], ref.reshape(1), LOSS_RTOL, "scalar")]
        if want_grad:      # dd_bce_probs' gradient: tests/test_gpu_box_loss.py::test_unit_weight_is_bce_probs holds it to GRAD_OF_PEAK = KERNEL_TOL
            checks.append(Check("grad", outs["grad"], gref, KERNEL_TOL))
        return checks
    return fn


for _entry in ("dd_bce_probs", "dd_mse"):
    for _n in (7, 4099):
        for _g in (True, False):
            case(f"{_entry}[n={_n},grad={_g}]", _entry)(_pair_loss(_entry, _n, _g))


def _threat(n, round_b):
    def fn(arena, mode):
        a64 = (hu((n,), "ta", 0.0, 1.0) < 0.4).double()
        b64 = hu((n,), "tb", 0.0, 1.0).double()
        a, b = arena.put(a64.float(), 16, "a"), arena.put(b64.float(), 16, "b")
        out = arena.out((1,), f32, 16, "out")
        ws = arena.workspace(size("dd_threat_score_workspace_bytes"), 16)
        call("dd_threat_score", a, b, out, n, int(round_b), ws)
        bb = b64.round() if round_b else b64
        tp = (a64 * bb).sum()
        return [Check("ts", arena.verify()["out"], (tp / (a64.sum() + bb.sum() - tp)).reshape(1), TS_ATOL, "abs")]
    return fn


for _n in (7, 4099):
    for _r in (False, True):
        case(f"dd_threat_score[n={_n},round={_r}]", "dd_threat_score")(_threat(_n, _r))


def _elementwise(entry, n):
    def fn(arena, mode):
        a64, b64 = hu((n,), "ea", -4.0, 4.0).double(), hu((n,), "eb", 0.0, 1.0).double()
        if entry == "dd_sigmoid":
            z, p = arena.put(a64.float(), 16, "z"), arena.out((n,), f32, 16, "p")
            call(entry, z, p, n)
            return [Check("p", arena.verify()["p"], torch.sigmoid(a64), KERNEL_TOL)]
        a, b, o = arena.put(a64.float(), 16, "a"), arena.put(b64.float(), 16, "b"), arena.out((n,), f32, 16, "out")
        if entry == "dd_sigmoid_bwd":
            call(entry, a, b, o, n)
            return [Check("dlogits", arena.verify()["out"], a64 * b64 * (1 - b64), KERNEL_TOL)]
        if entry == "dd_add":      # one correctly rounded fp32 add: the fp64 sum rounded once is the same number
            call(entry, a, b, o, n)
            return [Check("sum", arena.verify()["out"], (a64 + b64).float(), how="exact")]
        y64 = hu((n,), "ey").double()
        y = arena.put(y64.float(), 16, "y")
        call("dd_relu_bwd", a, y, o, n)      # (dy, y, out)
        return [Check("relu_bwd", arena.verify()["out"], (a64 * (y64 > 0)).float(), how="exact")]
    return fn


for _entry in ("dd_sigmoid", "dd_sigmoid_bwd", "dd_add", "dd_relu_bwd"):
    for _n in (4, 4096):      # f32x4 only: n % 4 == 0
        case(f"{_entry}[n={_n}]", _entry)(_elementwise(_entry, _n))


def _scale_by_scalar(n, s):
    def fn(arena, mode):
        x64 = hu((n,), "sx").double()
        x = arena.inout(x64.float(), 16, "x")
        sc = arena.put(torch.tensor([s]), 4, "scalar")      # a device scalar: 4 bytes
        call("dd_scale_by_device_scalar", x, sc, n)
        return [Check("x", arena.verify()["x"], (x64 * float(torch.tensor(s, dtype=f32))).float(), how="exact")]
    return fn


for _n in (7, 4099):
    for _s in (1.0, 0.37):      # 1.0: skipped on the device, nothing is touched
        case(f"dd_scale_by_device_scalar[n={_n},s={_s}]", "dd_scale_by_device_scalar")(_scale_by_scalar(_n, _s))


def _ts_hist(n, bins, byte_target):
    def fn(arena, mode):
        p0 = hu((n,), f"hp{n}", 0.0, 1.0)
        p0[0], p0[1], p0[2] = 0.0, 1.0, float("nan")      # slot 0, slot bins, NaN -> slot 0
        t0 = hu((n,), f"ht{n}", 0.0, 1.0) < 0.3
        prob = arena.put(p0, 16, "prob")
        target = arena.put(t0.to(u8) if byte_target else t0.float(), 4 if byte_target else 16, "target")
        before = torch.arange(2 * (bins + 1), dtype=i64).reshape(2, bins + 1)      # the counts are ADDED to what hist holds
        hist = arena.inout(before, 8, "hist")
        call("dd_ts_hist", prob, target, 1 if byte_target else 0, n, bins, hist)
        slot = torch.ceil(p0.double() * bins).clamp(0, bins)
        slot = torch.where(torch.isnan(slot), torch.zeros_like(slot), slot).long()
        want = before.clone()
        for row in (0, 1):
            want[row] += torch.bincount(slot[t0 == bool(row)], minlength=bins + 1)
        return [Check("hist", arena.verify()["hist"], want, how="exact")]
    return fn


for _n, _bins, _bt in ((4, 2, False), (4100, 256, True), (4100, 1024, False)):
    case(f"dd_ts_hist[n={_n},bins={_bins},u8={_bt}]", "dd_ts_hist")(_ts_hist(_n, _bins, _bt))


# ------------------------------------------------------------------------------------------------ Adam
B1, B2 = float(torch.tensor(0.9, dtype=f32)), float(torch.tensor(0.999, dtype=f32))      # the kernels take the betas as fp32


def adam64(p, m, v, g, lr, eps, step):
    """torch.optim.Adam's arithmetic in fp64 (tests/test_gpu_round5.py::_adam64)."""
    m = m * B1 + g * (1 - B1)
    v = v * B2 + g * g * (1 - B2)
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    return p - lr / bc1 * m / (v.sqrt() / bc2 ** 0.5 + eps), m, v


def _pgmv(shape, salt):
    return (hu(shape, f"p{salt}"), hu(shape, f"g{salt}", -0.1, 0.1), hu(shape, f"m{salt}", -0.05, 0.05), hu(shape, f"v{salt}", 1e-4, 1e-2))


def _adam_flat(n, on_dev):
    def fn(arena, mode):
        p0, g0, m0, v0 = _pgmv((n,), "flat")
        p, g, m, v = arena.inout(p0, 16, "p"), arena.put(g0, 16, "g"), arena.inout(m0, 16, "m"), arena.inout(v0, 16, "v")
        if on_dev:
            sc = arena.put(torch.tensor([0.5]), 4, "grad_scale_dev")
            call("dd_adam_step_dev", p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 3, sc)
        else:
            call("dd_adam_step", p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 3, 0.5)
        outs = arena.verify()
        pr, mr, vr = adam64(p0.double(), m0.double(), v0.double(), g0.double() * 0.5, 1e-3, 1e-8, 3)
        return [Check("p", outs["p"], pr, ADAM_P_TOL), Check("m", outs["m"], mr, ADAM_MV_TOL), Check("v", outs["v"], vr, ADAM_MV_TOL)]
    return fn


case("dd_adam_step[n=10007]", "dd_adam_step")(_adam_flat(10007, False))
case("dd_adam_step_dev[n=10007]", "dd_adam_step_dev")(_adam_flat(10007, True))

MULTI_SIZES = [1, 3, 32, 255, 256, 257, 864, 4097] + [7 + i for i in range(50)]      # tests/test_gpu_parity.py::test_adam_multi_tensor_matches_torch


def _adam_multi(on_dev):
    def fn(arena, mode):
        host = [_pgmv((n,), f"multi{i}") for i, n in enumerate(MULTI_SIZES)]
        quads = [(arena.inout(p, 16, f"p{i}"), arena.put(g, 16, f"g{i}"), arena.inout(m, 16, f"m{i}"), arena.inout(v, 16, f"v{i}"))
                 for i, (p, g, m, v) in enumerate(host)]
        table = adam_table(quads)
        if on_dev:
            sc = arena.put(torch.tensor([0.5]), 4, "grad_scale_dev")
            call("dd_adam_step_multi_dev", table, len(quads), 1e-3, 0.9, 0.999, 1e-8, 2, sc)
        else:
            call("dd_adam_step_multi", table, len(quads), 1e-3, 0.9, 0.999, 1e-8, 2, 0.5)
        outs = arena.verify()
        ref = [adam64(p.double(), m.double(), v.double(), g.double() * 0.5, 1e-3, 1e-8, 2) for p, g, m, v in host]
        cat = lambda k: torch.cat([outs[f"{k}{i}"] for i in range(len(host))])
        return [Check("p", cat("p"), torch.cat([r[0] for r in ref]), ADAM_P_TOL), Check("m", cat("m"), torch.cat([r[1] for r in ref]), ADAM_MV_TOL),
                Check("v", cat("v"), torch.cat([r[2] for r in ref]), ADAM_MV_TOL)]
    return fn


case("dd_adam_step_multi[58 tensors]", "dd_adam_step_multi", capacity=24 << 20)(_adam_multi(False))
case("dd_adam_step_multi_dev[58 tensors]", "dd_adam_step_multi_dev", capacity=24 << 20)(_adam_multi(True))


def _adam_rankb(n, k, rows, with_bias, on_dev):
    def fn(arena, mode):
        p0, _, m0, v0 = _pgmv((n, k), f"rb{n}{k}")
        b0, _, bm0, bv0 = _pgmv((n,), f"rbb{n}")
        x0 = hu((rows, k), f"rbx{rows}{k}", 0.0, 1.0)                 # unsigned factors: every gradient element well conditioned
        dy0 = hu((rows, n), f"rbdy{rows}{n}", 0.0, 0.1)
        p, m, v = arena.inout(p0, 16, "p"), arena.inout(m0, 16, "m"), arena.inout(v0, 16, "v")
        dy, x = arena.put(dy0, 16, "dy"), arena.put(x0, 16, "x")
        b = bm = bv = None
        if with_bias:
            b, bm, bv = arena.inout(b0, 16, "bias_p"), arena.inout(bm0, 16, "bias_m"), arena.inout(bv0, 16, "bias_v")
        if on_dev:
            sc = arena.put(torch.tensor([0.5]), 4, "grad_scale_dev")
            call("dd_adam_step_rankb_dev", p, m, v, dy, x, rows, n, k, b, bm, bv, 1e-3, 0.9, 0.999, 1e-8, 2, sc)
        else:
            call("dd_adam_step_rankb", p, m, v, dy, x, rows, n, k, b, bm, bv, 1e-3, 0.9, 0.999, 1e-8, 2, 0.5)
        outs = arena.verify()
        pr, mr, vr = adam64(p0.double(), m0.double(), v0.double(), dy0.double().t() @ x0.double() * 0.5, 1e-3, 1e-8, 2)
        checks = [Check("p", outs["p"], pr, ADAM_P_TOL), Check("m", outs["m"], mr, ADAM_MV_TOL), Check("v", outs["v"], vr, ADAM_MV_TOL)]
        if with_bias:
            br, bmr, bvr = adam64(b0.double(), bm0.double(), bv0.double(), dy0.double().sum(0) * 0.5, 1e-3, 1e-8, 2)
            checks += [Check("bias_p", outs["bias_p"], br, ADAM_P_TOL), Check("bias_m", outs["bias_m"], bmr, ADAM_MV_TOL),
                       Check("bias_v", outs["bias_v"], bvr, ADAM_MV_TOL)]
        return checks
    return fn


for _n, _k in ((20, 4), (52, 132)):      # the smallest of tests/test_gpu_round5.py::RANKB_SHAPES: less than one tile; ragged n- and k-tiles
    for _rows, _bias in ((1, True), (7, False), (64, True)):
        case(f"dd_adam_step_rankb[{_n}x{_k},rows={_rows},bias={_bias}]", "dd_adam_step_rankb")(_adam_rankb(_n, _k, _rows, _bias, False))
case("dd_adam_step_rankb_dev[52x132,rows=7,bias=True]", "dd_adam_step_rankb_dev")(_adam_rankb(52, 132, 7, True, True))
# rows past M that the kernels fetch through the wave-uniform offset of the load (x rows 16 .. 31 of a 32-row chunk), not through the
# lane's own: 20 rows (lds<1,2>), 40 (lds<2,1>, 8 rows in its second chunk), 48 on one k-tile (lds<2,1>; by device scale at the head's
# K = 64).  The arena has NaN behind x: a row that came back as memory instead of zeros makes every element of its tile NaN.
for _rows, _bias in ((20, True), (40, False)):
    case(f"dd_adam_step_rankb[52x132,rows={_rows},bias={_bias}]", "dd_adam_step_rankb")(_adam_rankb(52, 132, _rows, _bias, False))
case("dd_adam_step_rankb[20x4,rows=48,bias=True]", "dd_adam_step_rankb")(_adam_rankb(20, 4, 48, True, False))
case("dd_adam_step_rankb_dev[640x64,rows=48,bias=True]", "dd_adam_step_rankb_dev")(_adam_rankb(640, 64, 48, True, True))


# ------------------------------------------------------------------------------------------------ gradnorm.hip
def _sqnorm(n):
    def fn(arena, mode):
        g0 = hu((n,), f"sq{n}")
        g = arena.put(g0, 16, "g")
        out = arena.out((1,), f64, 8, "out")
        nbytes = size("dd_sqnorm_workspace_bytes", n)
        ws = arena.workspace(nbytes, 16)
        call("dd_sqnorm", g, n, out, ws, nbytes)
        ref = g0.double().pow(2).sum()
        return [Check("sqnorm", arena.verify()["out"], ref.reshape(1), n * EPS52 * float(ref), "abs")]      # test_sqnorm_matches_fp64's bound
    return fn


for _n in (3, 1027):
    case(f"dd_sqnorm[n={_n}]", "dd_sqnorm")(_sqnorm(_n))


def _sqnorm_multi(count):
    def fn(arena, mode):
        sizes = [(1, 3, 4, 1027, 255)[i % 5] for i in range(count)]
        host = [hu((n,), f"sqm{i}") for i, n in enumerate(sizes)]
        gs = [arena.put(g, 4, f"g{i}") for i, g in enumerate(host)]      # "any alignment": the type's
        table = adam_table([(g, g, g, g) for g in gs])                   # only the g / n fields are read
        out = arena.out((1,), f64, 8, "out")
        nbytes = size("dd_sqnorm_multi_workspace_bytes", table, count)
        ws = arena.workspace(nbytes, 16)
        call("dd_sqnorm_multi", table, count, out, ws, nbytes)
        ref = sum(g.double().pow(2).sum() for g in host)
        return [Check("sqnorm", arena.verify()["out"], ref.reshape(1), sum(sizes) * EPS52 * float(ref), "abs")]
    return fn


case("dd_sqnorm_multi[5]", "dd_sqnorm_multi")(_sqnorm_multi(5))
case("dd_sqnorm_multi[49]", "dd_sqnorm_multi", capacity=16 << 20)(_sqnorm_multi(49))      # one more than a table holds


def _rankb_sqnorm(rows, n, k, with_bias):
    def fn(arena, mode):
        x0 = hu((rows, k), f"rsx{rows}{k}", 0.0, 1.0)
        dy0 = hu((rows, n), f"rsy{rows}{n}", -1e-3, 1e-3)
        dy, x = arena.put(dy0, 16, "dy"), arena.put(x0, 16, "x")
        out = arena.out((1,), f64, 8, "out")
        nbytes = size("dd_rankb_sqnorm_workspace_bytes", rows, n, k)
        ws = arena.workspace(nbytes, 16)
        call("dd_rankb_sqnorm", dy, x, rows, n, k, with_bias, out, ws, nbytes)
        xd, yd = x0.double(), dy0.double()
        ref = float(((yd.T @ xd) ** 2).sum() + (yd.sum(0).pow(2).sum() if with_bias else 0.0))
        # the bound tests/test_gpu_grad_clip.py::_check_rankb_sqnorm derives: half-ulps of the sum of the absolute terms
        mag = float(((xd.abs() @ xd.abs().T) * (yd.abs() @ yd.abs().T)).sum())
        tol = (max(n, k) + rows * rows) * EPS52 * mag
        assert tol / ref < 1e-3
        return [Check("sqnorm", arena.verify()["out"], torch.tensor([ref], dtype=f64), tol, "abs")]
    return fn


for _rows in (1, 7, 64):
    for _n, _k in ((4, 4), (64, 260)):
        case(f"dd_rankb_sqnorm[rows={_rows},{_n}x{_k}]", "dd_rankb_sqnorm")(_rankb_sqnorm(_rows, _n, _k, _rows != 7))
for _n, _k in ((4, 4), (64, 260)):      # 40 rows: three 16-row blocks, the last one half full
    case(f"dd_rankb_sqnorm[rows=40,{_n}x{_k}]", "dd_rankb_sqnorm")(_rankb_sqnorm(40, _n, _k, True))


def _clip_scale(max_norm, grad_scale):
    def fn(arena, mode):
        slots = [4.0, 0.25, 1e-12]
        sq = arena.put(torch.tensor(slots, dtype=f64), 8, "sq")
        out3 = arena.out((3,), f32, 4, "out3")
        call("dd_clip_scale", sq, 3, max_norm, grad_scale, out3)
        norm = grad_scale * math.sqrt(sum(slots))
        coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
        got = arena.verify()["out3"]
        want = torch.tensor([grad_scale * coef, norm, coef], dtype=f64)
        assert bool(((got.double() - want).abs() <= EPS23 * want.abs()).all()), (got, want)      # test_clip_scale_is_clip_grad_norm_s_formula
        return [Check("out3", got, want, EPS23 * float(want.max()), "abs")]
    return fn


case("dd_clip_scale[1.0,1.0]", "dd_clip_scale")(_clip_scale(1.0, 1.0))
case("dd_clip_scale[0.0,0.25]", "dd_clip_scale")(_clip_scale(0.0, 0.25))


# ------------------------------------------------------------------------------------------------ linear.hip
def linear_nsplit(m, n, k, dgrad):
    """pick_split of csrc/linear.hip:428 for the forward (K tiles of 64 over ceil(N/128) workgroups) or the data gradient (N tiles of 32
    over ceil(K/128))."""
    other, ntiles = ((k + 127) // 128, (n + 31) // 32) if dgrad else ((n + 127) // 128, (k + 63) // 64)
    if ntiles <= 8:
        return 1
    split = min(max(1, min((512 + other - 1) // other, ntiles)), 512)
    tps = (ntiles + split - 1) // split
    return (ntiles + tps - 1) // tps


def _linear(entry, m, n, k, bias=True, nsplit=None):
    def fn(arena, mode):
        x64, w64 = hu((m, k), f"lx{m}{k}").double(), hu((n, k), f"lw{n}{k}", -0.2, 0.2).double()
        b64, gy64 = hu((n,), f"lb{n}").double(), hu((m, n), f"lg{m}{n}").double()
        nbytes = size("dd_linear_workspace_bytes", m, n, k)
        if nsplit is not None:      # the shape reaches the split / no-split side the case is named for (and the reduce kernel chosen by nsplit >= 16)
            assert linear_nsplit(m, n, k, entry == "dd_linear_dgrad") == nsplit
        if entry == "dd_linear_fwd":
            x, w = arena.put(x64.float(), 16, "x"), arena.put(w64.float(), 16, "w")
            b = arena.put(b64.float(), 16, "bias") if bias else None
            y = arena.out((m, n), f32, 16, "y")
            ws = arena.workspace(nbytes, 16)
            call(entry, x, w, b, y, m, n, k, ws, nbytes)
            return [Check("y", arena.verify()["y"], F.linear(x64, w64, b64 if bias else None), KERNEL_TOL)]
        dy, w = arena.put(gy64.float(), 16, "dy"), arena.put(w64.float(), 16, "w")
        dx = arena.out((m, k), f32, 16, "dx")
        ws = arena.workspace(nbytes, 16)
        call(entry, dy, w, dx, m, n, k, ws, nbytes)
        return [Check("dx", arena.verify()["dx"], gy64 @ w64, KERNEL_TOL)]
    return fn


for _m, _n, _k, _ns in ((3, 16, 704, 11), (5, 20, 8, 1), (65, 8, 8, 1), (3, 16, 1088, 17)):      # 11 splits: splits_reduce_few_kernel; 17: splits_reduce_kernel
    case(f"dd_linear_fwd[{_m},{_n},{_k}]", "dd_linear_fwd", capacity=16 << 20)(_linear("dd_linear_fwd", _m, _n, _k, True, _ns))
case("dd_linear_fwd[3,16,704,no bias]", "dd_linear_fwd", capacity=16 << 20)(_linear("dd_linear_fwd", 3, 16, 704, False, 11))
for _m, _n, _k, _ns in ((3, 16, 704, 1), (5, 20, 8, 1), (65, 8, 8, 1), (3, 292, 8, 10), (3, 548, 8, 18)):
    case(f"dd_linear_dgrad[{_m},{_n},{_k}]", "dd_linear_dgrad", capacity=16 << 20)(_linear("dd_linear_dgrad", _m, _n, _k, True, _ns))


def _linear_wgrad(m, n, k, with_bias):
    def fn(arena, mode):
        x64, gy64 = hu((m, k), f"lx{m}{k}").double(), hu((m, n), f"lg{m}{n}").double()
        # csrc/linear.hip:554: the 16-byte kernel wants x and dw on 16 bytes; the launcher's else branch takes anything a float can have
        loose = 4 if (k >= 512 and mode == "minimal") else 16
        dy, x = arena.put(gy64.float(), 16, "dy"), arena.put(x64.float(), loose, "x")
        dw = arena.out((n, k), f32, loose, "dw")
        db = arena.out((n,), f32, 16, "dbias") if with_bias else None
        wide = k >= 512 and k % 4 == 0 and x.data_ptr() % 16 == 0 and dw.data_ptr() % 16 == 0      # the launcher's predicate
        assert wide == (k >= 512 and mode == "natural"), "the two modes must reach linear_wgrad_wide_kernel and the scalar tiles"
        call("dd_linear_wgrad", dy, x, dw, db, m, n, k)
        outs = arena.verify()
        checks = [Check("dw", outs["dw"], gy64.t() @ x64, KERNEL_TOL)]
        if with_bias:
            checks.append(Check("dbias", outs["dbias"], gy64.sum(0), KERNEL_TOL))
        return checks
    return fn


for _m, _n, _k in ((3, 16, 704), (5, 20, 8), (65, 8, 8), (2, 1000, 64)):      # wide | scalar; scalar <4,1>; the same past 64 rows; scalar <1,2>
    case(f"dd_linear_wgrad[{_m},{_n},{_k}]", "dd_linear_wgrad", picks_kernel_by_alignment=_k >= 512)(_linear_wgrad(_m, _n, _k, True))
case("dd_linear_wgrad[3,16,704,no dbias]", "dd_linear_wgrad", picks_kernel_by_alignment=True)(_linear_wgrad(3, 16, 704, False))


def _column_sum(m, n):
    def fn(arena, mode):
        dy0 = hu((m, n), f"cs{m}{n}", -0.5, 0.5)
        al = 16 if n % 4 == 0 else 4      # csrc/linear.hip:543
        dy, db = arena.put(dy0, al, "dy"), arena.out((n,), f32, al, "dbias")
        call("dd_column_sum", dy, db, m, n)
        return [Check("dbias", arena.verify()["dbias"], dy0.double().sum(0), COLSUM_ATOL, "abs")]
    return fn


for _m, _n in ((32, 640), (7, 50), (3, 1027)):      # tests/test_gpu_round5.py::test_column_sum_matches_fp64
    case(f"dd_column_sum[{_m},{_n}]", "dd_column_sum")(_column_sum(_m, _n))


# ------------------------------------------------------------------------------------------------ dense.hip: BatchNorm1d + ReLU + dropout
def _bn_relu_drop(rows, feat, training, wide_pick=False):
    """Forward and backward in one arena (the backward reads what the forward wrote).  Dropout 0 (keep = NULL) so that fp64 applies.
    wide_pick: feat >= 65536, where the launchers take the multi-feature kernels for aligned operands (ALIGNMENT_PICKS) -- the
    minimal mode then puts x and dy on 4 bytes, which sends both launchers to the one-feature kernels."""
    def fn(arena, mode):
        eps, mom = 1e-5, 0.1
        x64 = hu((rows, feat), f"bnx{rows}{feat}", -2.0, 2.0).double().requires_grad_(True)
        g64 = hu((feat,), f"bng{feat}", 0.5, 1.5).double().requires_grad_(True)
        b64 = hu((feat,), f"bnb{feat}", -0.5, 0.5).double().requires_grad_(True)
        rm0, rv0 = hu((feat,), f"bnrm{feat}", -0.3, 0.3), hu((feat,), f"bnrv{feat}", 0.5, 1.5)
        gy64 = hu((rows, feat), f"bngy{rows}{feat}").double()
        rm64, rv64 = rm0.double().clone(), rv0.double().clone()
        y64 = F.relu(F.batch_norm(x64, rm64, rv64, g64, b64, training, mom, eps))
        y64.backward(gy64)
        loose = 4 if (wide_pick and mode == "minimal") else 16
        x = arena.put(x64.detach().float(), loose, "x")
        gamma, beta = arena.put(g64.detach().float(), 16, "gamma"), arena.put(b64.detach().float(), 16, "beta")
        rm, rv = arena.inout(rm0, 16, "running_mean"), arena.inout(rv0, 16, "running_var")
        nbt = arena.inout(torch.tensor([41], dtype=i64), 8, "num_batches_tracked")
        y = arena.out((rows, feat), f32, 16, "y")
        sm = arena.out((feat,), f32, 16, "save_mean", check_finite=training)      # written in training mode only
        si = arena.out((feat,), f32, 16, "save_invstd", check_finite=training)
        dy = arena.put(gy64.float(), loose, "dy")
        dx, dg, db = arena.out((rows, feat), f32, 16, "dx"), arena.out((feat,), f32, 16, "dgamma"), arena.out((feat,), f32, 16, "dbeta")
        if wide_pick:
            al = lambda t, a: t.data_ptr() % a == 0
            assert rows <= 32 and feat >= (1 << 16) and feat % 4 == 0
            assert al(x, 16) == (mode == "natural") and al(dy, 8) == (mode == "natural"), "one mode per kernel of dd_bn_relu_drop_fwd / dd_bn_relu_drop_bwd (csrc/dense.hip)"
        call("dd_bn_relu_drop_fwd", x, gamma, beta, rm, rv, None, y, sm, si, rows, feat, eps, mom, 1.0, int(training), nbt)
        call("dd_bn_relu_drop_bwd", dy, x, y, gamma, None, sm, si, rm, rv, dx, dg, db, rows, feat, eps, 1.0, int(training))
        outs = arena.verify()
        # tolerances: tests/test_gpu_parity.py::test_bn_relu_dropout
        checks = [Check("y", outs["y"], y64, KERNEL_TOL), Check("dx", outs["dx"], x64.grad, 10 * KERNEL_TOL),
                  Check("dgamma", outs["dgamma"], g64.grad, 10 * KERNEL_TOL), Check("dbeta", outs["dbeta"], b64.grad, 10 * KERNEL_TOL),
                  Check("running_mean", outs["running_mean"], rm64, KERNEL_TOL), Check("running_var", outs["running_var"], rv64, KERNEL_TOL),
                  Check("num_batches_tracked", outs["num_batches_tracked"], torch.tensor([42 if training else 41]), how="exact")]
        if training:
            xd = x64.detach()
            checks += [Check("save_mean", outs["save_mean"], xd.mean(0), KERNEL_TOL),
                       Check("save_invstd", outs["save_invstd"], 1 / (xd.var(0, unbiased=False) + eps).sqrt(), KERNEL_TOL)]
        return checks
    return fn


for _rows, _feat in ((3, 16), (5, 300), (65, 128)):      # <32>, <32> with a ragged block, the generic <0> kernel
    for _tr in (True, False):
        case(f"dd_bn_relu_drop[{_rows}x{_feat},training={_tr}]", ("dd_bn_relu_drop_fwd", "dd_bn_relu_drop_bwd"))(_bn_relu_drop(_rows, _feat, _tr))
for _tr in (True, False):
    case(f"dd_bn_relu_drop[3x65536,training={_tr},vec4/vec2 | one feature per thread]", ("dd_bn_relu_drop_fwd", "dd_bn_relu_drop_bwd"),
         picks_kernel_by_alignment=True, capacity=16 << 20)(_bn_relu_drop(3, 65536, _tr, wide_pick=True))


# ------------------------------------------------------------------------------------------------ mlp_tail.hip
def _mlp_tail(m, h1, h2, l, training):
    """dd_mlp_tail_fwd then dd_mlp_tail_bwd in one arena, dropout 0 (keep = NULL).  Against fp64 the existing test
    (tests/test_gpu_parity.py::test_fused_encoder_tail_matches_the_separate_kernels) holds z to 1e-4 and dlin1 to 1e-3 of the peak
    (floor 1e-6); the other outputs it compares with the separate kernels only, so here they are checked for being written, finite
    and the same bits at both alignments, and the running statistics at KERNEL_TOL like dd_bn_relu_drop_fwd's."""
    def fn(arena, mode):
        from driving_dirty_amd import _lib
        assert _lib.lib().dd_mlp_tail_supported(m, h1, h2, l)
        eps, mom = 1e-5, 0.1
        p64 = {k: hu(s, f"mt{k}{m}{h1}", lo, hi).double().requires_grad_(True) for k, s, lo, hi in (
            ("lin1", (m, h1), -2.0, 2.0), ("gamma1", (h1,), 0.5, 1.5), ("beta1", (h1,), -0.5, 0.5), ("w2", (h2, h1), -0.3, 0.3),
            ("bias2", (h2,), -0.2, 0.2), ("gamma2", (h2,), 0.5, 1.5), ("beta2", (h2,), -0.5, 0.5), ("wz", (l, h2), -0.3, 0.3), ("bz", (l,), -0.2, 0.2))}
        stat0 = {"rm1": hu((h1,), "mtrm1", -0.3, 0.3), "rv1": hu((h1,), "mtrv1", 0.5, 1.5), "rm2": hu((h2,), "mtrm2", -0.3, 0.3), "rv2": hu((h2,), "mtrv2", 0.5, 1.5)}
        stat64 = {k: v.double().clone() for k, v in stat0.items()}
        y1 = F.relu(F.batch_norm(p64["lin1"], stat64["rm1"], stat64["rv1"], p64["gamma1"], p64["beta1"], training, mom, eps))
        lin2 = F.linear(y1, p64["w2"], p64["bias2"])
        y2 = F.relu(F.batch_norm(lin2, stat64["rm2"], stat64["rv2"], p64["gamma2"], p64["beta2"], training, mom, eps))
        z64 = F.linear(y2, p64["wz"], p64["bz"])
        gz64 = hu((m, l), "mtgz").double()
        z64.backward(gz64)
        d = {k: arena.put(v.detach().float(), 16, k) for k, v in p64.items()}
        s = {k: arena.inout(v, 16, k) for k, v in stat0.items()}
        nbt1, nbt2 = arena.inout(torch.tensor([5], dtype=i64), 8, "nbt1"), arena.inout(torch.tensor([9], dtype=i64), 8, "nbt2")
        o = {k: arena.out(shape, f32, 16, k, check_finite=(training or not k.startswith(("mean", "inv")))) for k, shape in (
            ("y1", (m, h1)), ("lin2", (m, h2)), ("y2", (m, h2)), ("z", (m, l)), ("mean1", (h1,)), ("inv1", (h1,)), ("mean2", (h2,)), ("inv2", (h2,)))}
        call("dd_mlp_tail_fwd", d["lin1"], d["gamma1"], d["beta1"], s["rm1"], s["rv1"], nbt1 if training else None, None, d["w2"], d["bias2"],
             d["gamma2"], d["beta2"], s["rm2"], s["rv2"], nbt2 if training else None, None, d["wz"], d["bz"], o["y1"], o["lin2"], o["y2"], o["z"],
             o["mean1"], o["inv1"], o["mean2"], o["inv2"], m, h1, h2, l, eps, eps, mom, mom, 1.0, 1.0, int(training))
        dz = arena.put(gz64.float(), 16, "dz")
        g = {k: arena.out(tuple(p64[k].shape), f32, 16, "d" + k) for k in ("lin1", "gamma1", "beta1", "w2", "bias2", "gamma2", "beta2", "wz", "bz")}
        call("dd_mlp_tail_bwd", dz, d["lin1"], o["y1"], o["lin2"], o["y2"], d["gamma1"], d["gamma2"], None, None, d["w2"], d["wz"], o["mean1"],
             o["inv1"], o["mean2"], o["inv2"], s["rm1"], s["rv1"], s["rm2"], s["rv2"], g["lin1"], g["gamma1"], g["beta1"], g["w2"], g["bias2"],
             g["gamma2"], g["beta2"], g["wz"], g["bz"], m, h1, h2, l, eps, eps, 1.0, 1.0, int(training))
        outs = arena.verify()
        checks = [Check("z", outs["z"], z64, 1e-4), Check("dlin1", outs["dlin1"], p64["lin1"].grad, 1e-3, floor=1e-6)]
        checks += [Check(k, outs[k], stat64[k], KERNEL_TOL) for k in stat0]
        checks += [Check("nbt1", outs["nbt1"], torch.tensor([6 if training else 5]), how="exact"), Check("nbt2", outs["nbt2"], torch.tensor([10 if training else 9]), how="exact")]
        # the forward's intermediates at z's bound, every gradient at dlin1's (the two fp64 bounds the existing test sets); a Linear bias
        # in front of a train-mode BatchNorm has a mathematically zero gradient: its floor is the weight gradient's scale, as there
        inter = {"y1": y1, "lin2": lin2, "y2": y2}
        checks += [Check(k, outs[k], v.detach(), 1e-4) for k, v in inter.items()]
        w2_peak = float(p64["w2"].grad.abs().max())
        checks += [Check("d" + k, outs["d" + k], p64[k].grad, 1e-3, floor=(w2_peak if (k == "bias2" and training) else 1e-6))
                   for k in ("gamma1", "beta1", "w2", "bias2", "gamma2", "beta2", "wz", "bz")]
        return checks
    return fn


for _m, _h1, _h2, _l, _tr in ((3, 16, 16, 8, True), (5, 24, 16, 8, False), (32, 128, 128, 64, True)):
    case(f"dd_mlp_tail[{_m},{_h1},{_h2},{_l},training={_tr}]", ("dd_mlp_tail_fwd", "dd_mlp_tail_bwd"))(_mlp_tail(_m, _h1, _h2, _l, _tr))


# ------------------------------------------------------------------------------------------------ box_loss.hip
def _box_loss(batch, per, byte_target):
    def fn(arena, mode):
        import _box_loss_ref as ref
        p0, t0 = ref.inputs(batch, per, salt=batch + per, empty=(1,))
        probs = arena.put(p0, 16, "probs")
        target = arena.put(t0.to(u8) if byte_target else t0, 4 if byte_target else 16, "target")
        loss = arena.out((3,), f32, 4, "loss_out")
        stats = arena.out((batch, 5), f64, 8, "stats")
        coef = arena.out((batch, 4), f32, 16, "coef")
        ws = arena.workspace(size("dd_box_loss_workspace_bytes", batch), 8)
        dprobs = arena.out((batch, per), f32, 16, "dprobs")
        kind = 1 if byte_target else 0
        call("dd_box_loss_fwd", probs, target, kind, batch, per, -1.0, 0.7, 1.3, 1.0, loss, stats, coef, ws)      # DD_POS_WEIGHT_AUTO
        call("dd_box_loss_bwd", probs, target, kind, batch, per, coef, 2.0, dprobs)
        outs = arena.verify()
        total, l_bce, l_ts, g = ref.loss_and_grad(p0, t0, ref.AUTO, 0.7, 1.3, 1.0)
        want_stats = ref.stats(p0, t0)
        assert bool(((outs["stats"] - want_stats).abs() <= STATS_RTOL * want_stats.abs()).all())      # test_loss_gradient_and_statistics_against_fp64
        # coef as the header defines it, from the fp64 sums: {c0, c1, c2, c3} with w = (P - T) / max(T, 1), eps = 1
        T, S, I = want_stats[:, 0], want_stats[:, 1], want_stats[:, 2]
        U, wb, bp = S + T - I, (per - T) / T.clamp(min=1.0), float(batch * per)
        want_coef = torch.stack([0.7 * wb / bp, torch.full_like(T, 0.7 / bp), 1.3 / (batch * (U + 1.0)), 1.3 * (I + 1.0) / (batch * (U + 1.0) ** 2)], dim=1)
        got, want = outs["dprobs"].double(), 2.0 * g
        excess = float(((got - want).abs().amax(1) / want.abs().amax(1)).max())      # grad_excess: per sample, of its peak
        assert excess <= GRAD_OF_PEAK, excess
        return [Check("L", outs["loss_out"][0:1], total.reshape(1), LOSS_RTOL, "scalar"), Check("L_bce", outs["loss_out"][1:2], l_bce.reshape(1), LOSS_RTOL, "scalar"),
                Check("L_ts", outs["loss_out"][2:3], l_ts.reshape(1), LOSS_RTOL, "scalar"), Check("stats", outs["stats"], want_stats, STATS_RTOL),
                Check("dprobs", outs["dprobs"], want, GRAD_OF_PEAK)] + [
                    Check(f"coef c{j}", outs["coef"][:, j], want_coef[:, j], LOSS_RTOL, floor=1e-300) for j in range(4)]
    return fn


for _per in (8, 4100):
    for _bt in (False, True):
        case(f"dd_box_loss[3x{_per},u8={_bt}]", ("dd_box_loss_fwd", "dd_box_loss_bwd"))(_box_loss(3, _per, _bt))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)

