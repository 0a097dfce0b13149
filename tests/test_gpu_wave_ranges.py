"""The persistent conv kernels where one wave owns SEVERAL consecutive row tiles.

csrc/conv3x3_bf16.hip (bf_strip_fwd forward / stride-1 data gradient, bf_s2_dgrad, bf_wgrad + reduce) and the components_v2
instantiations of csrc/conv3x3.hip (conv_strip_fwd<EPI_BIAS_STATS, AFF>, EPI_RELU_MASK_AFF, conv_s2_dgrad<.., 3>, conv_wgrad<.., true>)
give every wave one contiguous range of row tiles idx = column * rows + row (column = image * nstrips + strip), walk it column segment
by column segment, carry input rows from one output row to the next in a 3-slot LDS ring, (bf16 forward) process rows in pairs with a
dummy second row behind an odd segment, and re-prime the ring at every segment start.  At the default resident grid (>= 256 workgroups)
the small shapes of the other test files give a wave at most ONE tile, so none of that runs there.

Here dd_set_cu_budget shrinks the grids instead.  The shapes are sized from a bound on the waves that can exist, not from a count read
off the code under test: a CU holds at most 32 waves (8 per SIMD), so at budget k there are at most 32k; with >= 3 * 32k row tiles
every wave that has work owns >= 3 consecutive ones (all but possibly the last).  For the fp32 kernels the bound is exact in the code:
resident_grid() with per_cu <= 2 and WPB <= 8 gives at most 16k waves.  The row counts are odd primes, so for every wave count the
launchers can choose a strip or image seam falls strictly inside some wave's range.  `_ranges` asserts all of it per shape.

Every bound below is one an existing test already uses (test_gpu_bf16.py: one bf16 ulp / 5e-3 flipped elements / 2e-5 of peak / 4e-3 of
peak for the stack; test_gpu_parity.py: 1e-5 of peak between budgets; test_gpu_heads.py: CHAIN_TOL), or exact equality.  Each test
prints its figures before it asserts (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from torch.nn import functional as F
from torch.nn import grad as nngrad

from driving_dirty_amd import synth

from test_gpu_bf16 import assert_bf16_close, bf16r, hu, nchw, nhwc, pad4, unpack_bits
from test_gpu_heads import CHAIN_TOL, rel_err

pytestmark = pytest.mark.gpu

WAVES_PER_CU = 32            # 8 waves on each of the 4 SIMDs: the most any kernel can keep resident on one CU
FP32_WAVES_PER_CU = 16       # dd_conv_strip.h resident_grid(): per_cu <= 2 workgroups of WPB <= 8 waves
FULL = 256                   # dd_set_cu_budget's default: the whole chip


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class cu_budget:
    """with cu_budget(k): the resident grids cover k compute units; the whole chip again afterwards, whatever happened inside."""

    def __init__(self, k):
        self.k = k

    def __enter__(self):
        from driving_dirty_amd import _lib
        _lib.check(_lib.lib().dd_set_cu_budget(self.k), "dd_set_cu_budget")

    def __exit__(self, *exc):
        from driving_dirty_amd import _lib
        _lib.lib().dd_set_cu_budget(FULL)
        return False


def _ranges(tiles, rows, budget, waves_per_cu=WAVES_PER_CU, prime=True, seams=True):
    """The preconditions on a shape of `tiles` row tiles in columns of `rows` at CU budget `budget`, for EVERY wave count the launcher
    may pick (whole workgroups of 4 or 8 waves, at most waves_per_cu * budget): a range is >= 3 tiles long, and (seams) no range length
    makes all column seams coincide with range ends -- at least one seam lies strictly inside a range."""
    assert tiles % rows == 0 and tiles // rows >= 2, (tiles, rows)
    assert tiles >= 3 * waves_per_cu * budget, (tiles, budget)
    if prime:
        assert rows % 2 == 1 and all(rows % p for p in range(3, rows, 2)), rows
    for nw in range(4, waves_per_cu * budget + 1, 4):
        per = -(-tiles // nw)                            # wave_range(): per = ceil(tiles / waves)
        assert per >= 3, (tiles, nw, per)
        if seams:
            assert any((k * rows) % per for k in range(1, tiles // rows)), (tiles, rows, nw, per)


def _tiles(b, h, w, stride):
    """(row tiles of the forward / weight gradient / stride-1 data gradient, row tiles of the data gradient, rows per column)."""
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    nstrips = (wo + 31) // 32
    rows_d = ho if stride == 1 else (h + 1) // 2       # bf_s2_dgrad walks class rows: two input rows each
    return b * nstrips * ho, b * nstrips * rows_d, ho, rows_d


def _flips(got, ref):
    """(largest |got - ref| in bf16 ulps of ref, fraction of elements that differ): the two figures assert_bf16_close bounds."""
    got, ref = got.detach().float().cpu().double(), ref.detach().double().cpu()
    diff = (got - ref).abs()
    spacing = torch.pow(2.0, torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7).clamp_min(2.0 ** -133)
    return float((diff / spacing).max()), float((diff > 0).double().mean())


# ------------------------------------------------------------------------------------------------ part 1: the bf16 kernels, each alone
#   (b, h, w, cin, stride, budget, seed)         strips x rows x images = row tiles   (>= 3 * 32 * budget)
# The seed of each shape was picked on the CPU, before any run on the device, from a scan of the operands alone: the one of seeds 0-9 whose
# fp64 results keep the smallest non-zero forward / data-gradient value furthest from zero (>= 1e-5 forward, >= 3e-6 data gradient), and at
# which a plain fp32-accumulated torch convolution, rounded to bf16, passes assert_bf16_close (at most 1 ulp, flips <= 1e-4 against the
# 5e-3 cap).  A value within fp32 summation noise of zero has a bf16 ulp below that noise, and "one ulp" then says nothing about a kernel.
RANGE_CASES = [
    (2, 19, 70, 32, 1, 1, 1),      # 3 x 19 x 2 = 114: stride 1, Cin 32 (forward, stride-1 data gradient, weight gradient)
    (2, 19, 70, 3, 1, 1, 1),       # 3 x 19 x 2 = 114: stride 1, Cin 3 (8-byte pixels; no data gradient)
    (2, 37, 130, 32, 2, 1, 5),     # 3 x 19 x 2 = 114 output rows; the data gradient walks (37 + 1) / 2 = 19 class rows: 114
    (3, 37, 20, 32, 1, 1, 3),      # 1 x 37 x 3 = 111: one strip, so every seam is an image seam
    (3, 37, 20, 3, 1, 1, 2),       # the same for the 3-channel layer
    (2, 37, 70, 32, 1, 2, 2),      # 3 x 37 x 2 = 222 >= 192: budget 2, stride 1
    (2, 73, 130, 32, 2, 2, 9),     # 3 x 37 x 2 = 222 >= 192: budget 2, stride 2 (data gradient: (73 + 1) / 2 = 37 class rows)
]


@functools.lru_cache(maxsize=None)
def _operands(b, h, w, cin, stride, seed):
    """Operands as in test_gpu_bf16.py::test_conv_fwd_dgrad_wgrad and the fp64 oracle of the mixed-precision contract, computed once per
    shape and shared (read-only) by the tests below."""
    x = bf16r(hu((b, cin, h, w), "wr_x", 0.0, 1.0, seed))
    wt = hu((32, cin, 3, 3), "wr_w", -0.2, 0.2, seed)
    bias = hu((32,), "wr_b", -0.1, 0.1, seed)
    wr = bf16r(wt).double()
    y_ref = bf16r(F.relu(F.conv2d(x.double(), wr, bias.double(), stride=stride, padding=1)).float()).double()
    ho, wo = y_ref.shape[2:]
    g = bf16r(hu((b, 32, ho, wo), "wr_g", seed=seed))
    o = dict(x=x, wt=wt, bias=bias, g=g, y_ref=y_ref,
             dw_ref=nngrad.conv2d_weight(x.double(), wr.shape, g.double(), stride=stride, padding=1),
             db_ref=g.double().sum(dim=(0, 2, 3)))
    if cin == 32:
        mask = (hu((b, h, w, 32), "wr_m", seed=seed) > 0).numpy()
        o["words"] = torch.from_numpy((mask.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=3).astype(np.uint32).view(np.int32))
        dx = nngrad.conv2d_input((b, 32, h, w), wr, g.double(), stride=stride, padding=1) * torch.from_numpy(mask).permute(0, 3, 1, 2)
        o["dx_ref"] = bf16r(dx.float()).double()
    return o


def _device_operands(o, cin, dev):
    xd = (pad4(nhwc(o["x"])) if cin == 3 else nhwc(o["x"])).to(dev).to(torch.bfloat16)
    return xd, nhwc(o["g"]).to(dev).to(torch.bfloat16)


@pytest.mark.parametrize("b,h,w,cin,stride,budget,seed", RANGE_CASES)
def test_bf16_forward_and_data_gradient_over_multi_row_ranges(dev, b, h, w, cin, stride, budget, seed):
    """bf_strip_fwd (forward, stride-1 data gradient) and bf_s2_dgrad with every wave on >= 3 consecutive row tiles: one bf16 ulp / 5e-3
    flips against the fp64 oracle, sign words == (y > 0), and bit for bit what the whole chip (one tile per wave) computes -- a row's
    arithmetic does not depend on which wave has it, so that last check tells a scheduling error from a rounding flip."""
    from driving_dirty_amd import ops, ops_bf16 as ob
    t_fwd, t_dgrad, rows, rows_d = _tiles(b, h, w, stride)
    _ranges(t_fwd, rows, budget)
    _ranges(t_dgrad, rows_d, budget)
    o = _operands(b, h, w, cin, stride, seed)
    d = ops.conv_desc(b, h, w, cin, stride)
    xd, gd = _device_operands(o, cin, dev)
    wd = o["wt"].to(dev)
    pf = ob.conv_pack(wd, d, ops.PACK_FWD)
    if cin == 32:
        pd = ob.conv_pack(wd, d, ops.PACK_DGRAD_S1 if stride == 1 else ops.PACK_DGRAD_S2)
        words = o["words"].to(dev)
    out = {}
    for k in (budget, FULL):
        with cu_budget(k):
            y, bits = ob.conv_fwd(xd, pf, o["bias"].to(dev), d)
            dx = ob.conv_dgrad(gd, pd, words, d) if cin == 32 else None
            torch.cuda.synchronize()
        out[k] = (y, bits, dx)
    y, bits, dx = out[budget]
    print(f"\nforward {(b, h, w, cin, stride)} budget {budget}: max ulp %.3f, flipped %.2e" % _flips(nchw(y.float().cpu()), o["y_ref"]))
    assert torch.equal(y, out[FULL][0]), "forward: budget changes the result"
    assert torch.equal(bits, out[FULL][1]), "sign words: budget changes the result"
    assert_bf16_close(nchw(y.float().cpu()), o["y_ref"], "forward")
    assert torch.equal(unpack_bits(bits), (y.float().cpu() > 0).double())
    if cin == 32:
        print(f"dgrad   {(b, h, w, cin, stride)} budget {budget}: max ulp %.3f, flipped %.2e" % _flips(nchw(dx.float().cpu()), o["dx_ref"]))
        assert torch.equal(dx, out[FULL][2]), "data gradient: budget changes the result"
        assert_bf16_close(nchw(dx.float().cpu()), o["dx_ref"], "dgrad")


def _wgrad_with(xd, gd, d, nbytes):
    """dd_conv_bf16_wgrad on a workspace of exactly `nbytes` (ops_bf16.conv_wgrad sizes it itself: here the size is the test's)."""
    from driving_dirty_amd import _lib
    from driving_dirty_amd.ops import _p, _stream
    ws = torch.empty(nbytes, device=xd.device, dtype=torch.uint8)
    dw = torch.empty((32, d.cin_real, 3, 3), device=xd.device, dtype=torch.float32)
    db = torch.empty(32, device=xd.device, dtype=torch.float32)
    _lib.check(_lib.lib().dd_conv_bf16_wgrad(_p(xd), _p(gd), _p(dw), _p(db), C.byref(d), _p(ws), nbytes, _stream()), "dd_conv_bf16_wgrad")
    return dw, db


@pytest.mark.parametrize("b,h,w,cin,stride,budget,seed", RANGE_CASES)
def test_bf16_weight_gradient_over_multi_row_ranges(dev, b, h, w, cin, stride, budget, seed):
    """bf_wgrad + bf_wgrad_reduce with every wave on >= 3 consecutive row tiles, and on the whole chip: 2e-5 of peak against fp64,
    two launches at one budget bit-identical (fixed summation order), the workspace size independent of the budget (as
    dd_conv_bf16_wgrad_workspace_bytes promises) and enough for the launch at the reduced budget."""
    from driving_dirty_amd import _lib, ops
    t_fwd, _, rows, _ = _tiles(b, h, w, stride)
    _ranges(t_fwd, rows, budget)
    o = _operands(b, h, w, cin, stride, seed)
    d = ops.conv_desc(b, h, w, cin, stride)
    xd, gd = _device_operands(o, cin, dev)
    nbytes = {}
    for k in (FULL, budget):
        with cu_budget(k):
            nbytes[k] = _lib.lib().dd_conv_bf16_wgrad_workspace_bytes(C.byref(d))
    assert nbytes[FULL] > 0 and nbytes[budget] == nbytes[FULL], nbytes
    for k in (budget, FULL):
        with cu_budget(k):
            dw, db = _wgrad_with(xd, gd, d, nbytes[FULL])
            dw2, db2 = _wgrad_with(xd, gd, d, nbytes[FULL])
            torch.cuda.synchronize()
        ew = float((dw.cpu().double() - o["dw_ref"]).abs().max() / o["dw_ref"].abs().max())
        eb = float((db.cpu().double() - o["db_ref"]).abs().max() / o["db_ref"].abs().max().clamp_min(1e-3))
        print(f"\nwgrad   {(b, h, w, cin, stride)} budget {k}: dw {ew:.2e}, db {eb:.2e} of peak")
        assert torch.equal(dw, dw2) and torch.equal(db, db2), ("two launches differ", k)
        assert ew < 2e-5, ("dw", k, ew)
        assert eb < 2e-5, ("db", k, eb)


STACK = (2, 37, 136)      # c1, c2: 5 strips x 37 rows x 2 = 370 tiles; c3 (and its data gradient's class rows): 3 x 19 x 2 = 114; 19 * 68 % 4 == 0


@functools.lru_cache(maxsize=None)
def _stack_reference():
    from oracle import bf16_parts
    b, h, w = STACK
    mods = [torch.nn.Conv2d(3, 32, 3, padding=1), torch.nn.Conv2d(32, 32, 3, padding=1), torch.nn.Conv2d(32, 32, 3, stride=2, padding=1)]
    for i, m in enumerate(mods):
        synth.fill_module(m, seed=60 + i)
    x = bf16r(hu((b, 3, h, w), "wr_img", 0.0, 1.0))
    pooled, _ = bf16_parts.conv_stack_pooled(x, *mods)
    gp = hu(tuple(pooled.shape), "wr_gpool")
    pooled.backward(gp.double())
    grads = [p.grad.clone() for m in mods for p in (m.weight, m.bias)]
    state = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in mods]
    return x, gp, pooled.detach(), grads, state


def test_bf16_conv_stack_over_multi_row_ranges(dev):
    """ops_bf16.encoder_conv_stack forward + backward with every layer's waves on >= 3 consecutive row tiles: the pooled vector bit for
    bit the whole chip's, the fp32 weight / bias gradients within 1e-5 of peak of the whole chip's (their partial sums are grouped by
    wave; test_cu_budget_never_changes_results's bound), and both runs within test_conv_stack_against_oracle's 4e-3 of the oracle."""
    from driving_dirty_amd import ops_bf16 as ob
    b, h, w = STACK
    for stride in (1, 2):
        t_fwd, t_dgrad, rows, rows_d = _tiles(b, h, w, stride)
        _ranges(t_fwd, rows, 1)
        _ranges(t_dgrad, rows_d, 1)
    assert (((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)) % 4 == 0       # the pool's windows of 4
    x, gp, pooled_ref, ref_grads, state = _stack_reference()
    mods = [torch.nn.Conv2d(3, 32, 3, padding=1), torch.nn.Conv2d(32, 32, 3, padding=1), torch.nn.Conv2d(32, 32, 3, stride=2, padding=1)]
    for m, s in zip(mods, state):
        m.load_state_dict(s)
        m.to(dev)
    xd = pad4(nhwc(x)).to(dev).to(torch.bfloat16)
    names = ["c1.w", "c1.b", "c2.w", "c2.b", "c3.w", "c3.b"]
    out = {}
    for k in (1, FULL):
        for m in mods:
            m.zero_grad(set_to_none=True)
        with cu_budget(k):
            pooled = ob.encoder_conv_stack(xd, *mods)
            pooled.backward(gp.to(dev))
            torch.cuda.synchronize()
        out[k] = (pooled.detach(), [p.grad.clone() for m in mods for p in (m.weight, m.bias)])
    assert torch.equal(out[1][0], out[FULL][0]), "pooled vector: budget changes the result"
    for name, g1, gf in zip(names, out[1][1], out[FULL][1]):
        e = rel_err(g1, gf)
        print(f"\nstack {name}: budget 1 vs whole chip {e:.2e} of peak")
        assert e < 1e-5, (name, e)
    for k in (1, FULL):
        pooled, grads = out[k]
        e = float((pooled.cpu().double() - pooled_ref).abs().max() / pooled_ref.abs().max())
        print(f"stack pooled, budget {k}: {e:.2e} of peak against the oracle")
        assert e < 4e-3, ("pooled", k, e)
        for name, g, r in zip(names, grads, ref_grads):
            e = float((g.cpu().double() - r.double()).abs().max() / r.double().abs().max())
            print(f"stack {name}, budget {k}: {e:.2e} of peak against the oracle")
            assert e < 4e-3, (name, k, e)


# ------------------------------------------------------------------------------------------------ part 2: components_v2's affine kernels
# Input 26 x 72: c1, c2 have 3 strips x 26 rows per image, c3 and its data gradient 2 strips x 13 (class) rows; 13 * 36 pixels feed the pool.
# Batch 4: 312 and 104 row tiles.  With 104 = 8 x 13 (and 312 = 12 x 26) a launch of exactly 8 (12) waves gives each wave one whole column
# -- 13 (26) consecutive rows, but no seam inside a range -- so batch 3 (234 and 78 tiles, both >= 3 * 16) runs beside it: there no wave
# count lines up with the columns.
V2_H, V2_W = 26, 72
V2_BATCHES = (4, 3)
V2_FEATURE_KEYS = ("c1.weight", "bn1.weight", "bn1.bias", "c2.weight", "bn2.weight", "bn2.bias", "c3.weight", "bn3.weight", "bn3.bias")


@functools.lru_cache(maxsize=None)
def _v2_reference(b):
    """oracle.ae_parts.EncoderNetV2 in fp64, well-conditioned seeded fills as in test_encoder_v2_conv_bn_relu_against_oracle: latent exit
    with all gradients and the running statistics, c3_only exit with the conv / BN gradients, eval-mode latent.  Computed once."""
    from driving_dirty_amd.components_v2 import Encoder
    from oracle import ae_parts
    h, w = V2_H, V2_W
    state = {k: v.clone() for k, v in synth.fill_module(Encoder(16, 8, 3, h, w), seed=41).state_dict().items()}
    ref = ae_parts.EncoderNetV2(16, 8, 3, h, w).double()
    ref.load_state_dict(state)
    ref.fc1.drop_p = ref.fc2.drop_p = 0.0
    x = synth.hash_uniform((b, 3, h, w), synth.key_salt("wr_v2x"), 0.0, 1.0)
    wz = synth.hash_uniform((b, 8), synth.key_salt("wr_v2w"))
    ref.train()
    z = ref(x.double())
    (z * wz.double()).sum().backward()
    r = dict(state=state, x=x, wz=wz, z=z.detach().clone(), grads={k: p.grad.clone() for k, p in ref.named_parameters()},
             bufs={k: v.double().clone() for k, v in ref.named_buffers()})
    ref.zero_grad()
    ref.c3_only = True
    f = ref(x.double())
    r["wf"] = synth.hash_uniform(tuple(f.shape), synth.key_salt("wr_v2f"))
    (f * r["wf"].double()).sum().backward()
    r["f"] = f.detach().clone()
    r["fgrads"] = {k: dict(ref.named_parameters())[k].grad.clone() for k in V2_FEATURE_KEYS}
    ref.c3_only = False
    ref.eval()
    with torch.no_grad():
        r["z_eval"] = ref(x.double()).clone()
    return r


@pytest.mark.parametrize("budget", [1, FULL])
@pytest.mark.parametrize("b", V2_BATCHES)
def test_encoder_v2_affine_kernels_over_multi_row_ranges(dev, b, budget):
    """components_v2.Encoder (relu(u * scale + shift) applied to input rows as they enter the ring: conv_strip_fwd<EPI_BIAS_STATS, AFF>,
    EPI_RELU_MASK_AFF, conv_s2_dgrad<.., 3>, conv_wgrad<.., true>) against the fp64 oracle at budget 1, where every wave has >= 3
    consecutive row tiles, under test_encoder_v2_conv_bn_relu_against_oracle's bounds; the feature map is judged per element, so one
    wrong row fails it.  The same checks on the whole chip, so that a failure names the schedule and not the shape."""
    from driving_dirty_amd.components_v2 import Encoder
    h, w = V2_H, V2_W
    t1, _, rows1, _ = _tiles(b, h, w, 1)
    t3, t3d, rows3, rows3d = _tiles(b, h, w, 2)
    assert (t1, t3, t3d) == ((312, 104, 104) if b == 4 else (234, 78, 78))
    _ranges(t1, rows1, 1, FP32_WAVES_PER_CU, prime=False, seams=(b != 4))
    _ranges(t3, rows3, 1, FP32_WAVES_PER_CU, seams=(b != 4))
    _ranges(t3d, rows3d, 1, FP32_WAVES_PER_CU, seams=(b != 4))
    assert (rows3 * ((w - 1) // 2 + 1)) % 4 == 0                   # the pool's windows of 4
    r = _v2_reference(b)
    enc = Encoder(16, 8, 3, h, w)
    enc.load_state_dict(r["state"])
    enc = enc.to(dev)
    enc.fc1.drop_p = enc.fc2.drop_p = 0.0
    xd = r["x"].to(dev)
    with cu_budget(budget):
        enc.train()
        z = enc(xd)
        (z * r["wz"].to(dev)).sum().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in enc.named_parameters()}
        bufs = {k: v.double().clone() for k, v in enc.named_buffers()}
        enc.zero_grad()
        enc.c3_only = True
        f = enc(xd)
        (f * r["wf"].to(dev)).sum().backward()
        torch.cuda.synchronize()
        fgrads = {k: dict(enc.named_parameters())[k].grad.clone() for k in V2_FEATURE_KEYS}
        enc.c3_only = False
        enc.eval()
        z_eval = enc(xd)
        torch.cuda.synchronize()
    worst = {"latent": rel_err(z, r["z"]), "feature": rel_err(f, r["f"]), "eval": rel_err(z_eval, r["z_eval"])}
    for k, g in grads.items():
        floor = 1e-30
        if k.endswith("bias") and (k.startswith("c") or k.endswith(".fc1.bias")):      # a bias in front of a BatchNorm: zero gradient
            floor = float(r["grads"][k[:-4] + "weight"].abs().max())
        worst["grad " + k] = rel_err(g, r["grads"][k], floor=floor)
    for k, v in bufs.items():
        worst["buffer " + k] = rel_err(v, r["bufs"][k])
    for k, g in fgrads.items():
        worst["feature grad " + k] = rel_err(g, r["fgrads"][k])
    print(f"\nencoder v2, batch {b}, budget {budget}: worst " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]))
    for k, v in worst.items():
        assert v < CHAIN_TOL, (k, b, budget, v)
