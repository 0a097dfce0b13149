"""The references, models, grids and bounds of tests/_element_ref.py, checked on the CPU: the fp64 references are torch's own fp64
operations; the fp32 models of ``dd_sigmoid_softplus`` and ``adam_elem2`` (correctly rounded primitives) stay inside the model part of every
bound on every grid, so a kernel whose hardware primitives are good to their 1 ulp can meet the whole bound; the grids hold the edge values
they claim; and the bounded comparison leaves out at most 1 % of an Adam grid.  tests/test_gpu_element_range.py holds the kernels to the
same bounds."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _element_ref as R  # noqa: E402

D = np.float64
BANDS = (0, 2, 4, 8, 12, 16, 24, 40, 80)


def _all_logits():
    return np.concatenate([R.logit_grid(), R.softplus_points()] + [R.band_logits(k) for k in BANDS])


def test_fp64_sigmoid_and_bce_terms_are_torchs():
    z = _all_logits()
    zt = torch.from_numpy(z).double()
    ref = torch.sigmoid(zt).numpy()
    assert np.all(np.abs(R.sigmoid64(z) - ref) <= 1e-14 * ref)
    # softplus: -logsigmoid(|z|) is log1p(exp(-|z|)) with no cancellation
    sp = -TF.logsigmoid(zt.abs()).numpy()
    assert np.all(np.abs(R.softplus64(z) - sp) <= 1e-14 * sp)
    rs = np.random.RandomState(3)
    for t in (np.zeros_like(z), np.ones_like(z), (rs.uniform(size=z.size) < 0.5).astype(np.float32)):
        ref = TF.binary_cross_entropy_with_logits(zt, torch.from_numpy(t).double(), reduction="none").numpy()
        # torch forms (1 - t) z - logsigmoid(z): for a confident correct pixel that is a difference of two numbers of size |z|, so its own
        # rounding is 1e-16 (|z| + 1) absolute; relative agreement is what the softplus line above shows
        assert np.all(np.abs(R.bce_logits_terms64(z, t) - ref) <= 1e-14 * (np.abs(D(z)) + 1.0))


def _torch_adam64(p, g_steps, m, v, lr, b1, b2, eps, first_step, scale):
    q = R.adam_params(lr, b1, b2, eps, first_step, scale)
    pt = torch.from_numpy(D(p)).clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=float(q["lr"]), betas=(float(q["b1"]), float(q["b2"])), eps=float(q["eps"]), foreach=False)
    opt.state[pt] = {"step": torch.tensor(float(first_step - 1)), "exp_avg": torch.from_numpy(D(m)).clone(),
                     "exp_avg_sq": torch.from_numpy(D(v)).clone()}
    for g in g_steps:
        pt.grad = torch.from_numpy(D(g) * D(q["gs"]))
        opt.step()
    st = opt.state[pt]
    return pt.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("steps,first_step,cfg", [(1, 1, (1e-3, 0.9, 0.999, 1e-8, 1.0)), (1, 1000, (1.0, 0.5, 0.9, 1e-3, 0.37)),
                                                 (3, 1, (1e-3, 0.9, 0.999, 1e-8, 1.0)), (3, 10, (1e-3, 0.5, 0.9, 1e-8, 0.37))])
def test_fp64_adam_is_torchs(steps, first_step, cfg):
    """One and three steps of torch.optim.Adam (fp64, foreach=False) from a grid state.  torch forms m as a lerp, so the two agree to fp64
    rounding of m's TERMS; the update inherits that through U / M."""
    lr, b1, b2, eps, scale = cfg
    p, g, m, v = (t[:4099] for t in R.adam_grid())
    gs = [g * np.float32(1 + 0.5 * i) for i in range(steps)]
    pr, mr, vr = _torch_adam64(p, gs, m, v, lr, b1, b2, eps, first_step, scale)
    P, M, V = D(p), D(m), D(v)
    tol_p = 1e-14 * np.abs(P)
    for i, gi in enumerate(gs):
        M, V, U, mag = R.adam64(P, gi, M, V, lr, b1, b2, eps, first_step + i, scale)
        P = P + U
        tol_p = tol_p + 1e-14 * (mag / np.abs(M) + 1.0) * np.abs(U) + 1e-14 * np.abs(P)
    assert np.all(np.abs(M - mr) <= 1e-14 * steps * mag)
    assert np.all(np.abs(V - vr) <= 1e-14 * V)
    assert np.all(np.abs(P - pr) <= tol_p)


def test_fma32_rounds_once():
    """The model's fused multiply-add against exact rational arithmetic, on cases built to sit on an fp32 tie of the fp64 sum."""
    from fractions import Fraction
    rs = np.random.RandomState(5)
    a = rs.uniform(1, 2, 2000).astype(np.float32)
    b = rs.uniform(1, 2, 2000).astype(np.float32)
    exact = D(a) * D(b)
    tie = np.float32(exact).astype(D) + 0.5 * D(np.spacing(np.float32(exact)))      # an fp32 midpoint near a b
    c = (tie - exact).astype(np.float32)                                             # a b + c lands within an ulp of c of the midpoint
    c = np.concatenate([c, c * np.float32(1 + 2 ** -20), rs.uniform(-1e-9, 1e-9, 2000).astype(np.float32)])
    a, b = np.tile(a, 3), np.tile(b, 3)
    got = R.fma32(a, b, c)
    for x, y, w, o in zip(a, b, c, got):
        f = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(w))
        lo = np.float32(float(f))                                                    # float(Fraction) is correctly rounded to fp64
        cands = sorted({float(np.nextafter(lo, np.float32(-np.inf))), float(lo), float(np.nextafter(lo, np.float32(np.inf)))})
        dist = [abs(Fraction(cv) - f) for cv in cands]
        best = min(dist)
        winners = [cv for cv, dv in zip(cands, dist) if dv == best]
        assert float(o) in winners and (len(winners) == 1 or (np.float32(o).view(np.uint32) & 1) == 0)


def test_sigmoid_model_is_inside_the_model_part_of_the_bounds(capsys):
    z = _all_logits()
    sig, l1p = R.model_sigmoid_softplus(z)
    s64, sp64 = R.sigmoid64(z), R.softplus64(z)
    es, el = np.abs(D(sig) - s64), np.abs(D(l1p) - sp64)
    pos = z >= 0
    need_sig = (np.maximum(es - R.TINY, 0) / (R.U24 * s64) - np.abs(D(z)))[~pos].max()
    need_sp = (np.maximum(el - R.TINY, 0) / (R.U24 * sp64) - np.abs(D(z))).max()
    with capsys.disabled():
        print(f"\n[element model] sig z>=0: {es[pos].max() / R.U24:.2f} x 2^-24 absolute (model part {R.SIG_POS_MODEL / R.U24:.0f}, bound "
              f"{R.SIG_POS_BOUND / R.U24:.0f}); sig z<0 needs |z| + {need_sig:.2f} (model part {R.SIG_MODEL_K}, bound {R.SIG_BOUND_K}); "
              f"softplus needs |z| + {need_sp:.2f} (model part {R.SP_MODEL_K}, bound {R.SP_BOUND_K})")
    assert np.all(es <= R.sig_bound(z, s64, R.SIG_MODEL_K, R.SIG_POS_MODEL))
    assert np.all(el <= R.softplus_bound(z, sp64, R.SP_MODEL_K))
    assert R.SIG_MODEL_K < R.SIG_BOUND_K and R.SP_MODEL_K < R.SP_BOUND_K and R.SIG_POS_MODEL < R.SIG_POS_BOUND
    # the non-finite logits
    s, _ = R.model_sigmoid_softplus(np.array([np.nan, np.inf, -np.inf], dtype=np.float32))
    assert np.isnan(s[0]) and s[1] == 1.0 and s[2] == 0.0


def test_exact_sigmoid_is_the_models_and_known_for_most_positive_logits():
    """Where _element_ref.exact_sigmoid calls the probability known, the fp32 model gives those bits; and it is known for most of the
    logits the GPU test draws (a condition on the reference alone)."""
    z = R.exact_sigmoid_logits()
    known, bits = R.exact_sigmoid(z)
    sig, _ = R.model_sigmoid_softplus(z)
    assert known.mean() >= 0.85 and np.array_equal(sig[known].view(np.uint32), bits[known].view(np.uint32))
    for lo, hi, share in ((4, 6, 0.5), (6, 10, 0.9), (10, 17.4, 0.99)):
        assert known[(z >= lo) & (z < hi)].mean() >= share
    # a raw reciprocal one ulp off is NOT these bits: the check can tell a missing refinement
    off = np.nextafter(bits, np.float32(0))
    assert not np.any(off[known].view(np.uint32) == bits[known].view(np.uint32))
    # nor is anything known where it should not be: negative logits, and z = 0 (u = 2: the spacing changes)
    k2, _ = R.exact_sigmoid(np.array([-1.0, 0.0], dtype=np.float32))
    assert not k2.any()


def test_band_means_of_the_model_are_inside_the_loss_bounds():
    """The mean loss of a band from the model's terms (summed in fp64: the kernel's own fp32 partial sums are four terms long) against the
    fp64 mean, at the bounds tests/test_gpu_element_range.py uses: targets all right, all wrong, and half and half."""
    for k in BANDS:
        z = R.band_logits(k)
        _, l1p = R.model_sigmoid_softplus(z)
        right = (z > 0).astype(np.float32)
        rs = np.random.RandomState(k)
        mix = np.where(rs.uniform(size=z.size) < 0.5, right, 1 - right).astype(np.float32)
        for t in (right, 1 - right, mix):
            terms = (np.maximum(z, 0) - z * t).astype(np.float32).astype(D) + D(l1p)
            ref = R.bce_logits_terms64(z, t)
            assert abs(terms.mean() - ref.mean()) <= R.band_mean_bound(k, z, t) * ref.mean()


def test_adam_model_is_inside_the_model_part_of_the_bounds_and_the_filter_keeps_99_percent(capsys):
    p, g, m, v = R.adam_grid()
    worst = dict(v=0.0, m=0.0, u=0.0, excluded=0.0)
    for cfg in R.adam_configs():
        M, V, U, mag = R.adam64(p, g, m, v, *cfg)
        ok = R.adam_bounded(M, V, U)
        worst["excluded"] = max(worst["excluded"], 1.0 - ok.mean())
        pn, mn, vn = R.model_adam(p, g, m, v, *cfg)
        em, ev, eu = R.adam_errors(p, pn, mn, vn, M, V, U)
        tm, tv, tu = R.adam_bounds(p, M, V, U, mag, R.ADAM_MODEL_KV, R.ADAM_MODEL_KM, R.ADAM_MODEL_KU)
        assert np.all(em[ok] <= tm[ok]) and np.all(ev[ok] <= tv[ok]) and np.all(eu[ok] <= tu[ok]), cfg
        _, _, base = R.adam_bounds(p, M, V, U, mag, 0, R.ADAM_MODEL_KM, 0)          # m's share and the final half ulp alone
        worst["v"] = max(worst["v"], (ev / (R.U24 * np.abs(V)))[ok].max())
        worst["m"] = max(worst["m"], (em / (R.U24 * mag))[ok].max())
        worst["u"] = max(worst["u"], (np.maximum(eu - base, 0) / (R.U24 * np.abs(U)))[ok].max())
    with capsys.disabled():
        print(f"\n[adam model] worst over {len(R.adam_configs())} configurations, x 2^-24: v {worst['v']:.2f} (model part {R.ADAM_MODEL_KV}), "
              f"m {worst['m']:.2f} ({R.ADAM_MODEL_KM}), update {worst['u']:.2f} ({R.ADAM_MODEL_KU}); excluded share {worst['excluded']:.4%}")
    assert worst["excluded"] <= 0.01
    # the constants are the model's worst case rounded up, no more
    assert np.ceil(worst["v"]) == R.ADAM_MODEL_KV and np.ceil(worst["m"]) == R.ADAM_MODEL_KM and np.ceil(worst["u"]) == R.ADAM_MODEL_KU
    assert (R.ADAM_KV, R.ADAM_KM, R.ADAM_KU) == (R.ADAM_MODEL_KV + 2, R.ADAM_MODEL_KM + 2, R.ADAM_MODEL_KU + 2)


def test_a_nan_or_infinite_output_is_never_inside_a_bound():
    """error_fraction keeps NaN and turns an error against a zero tolerance into inf: an Adam pass that returns NaN for p, m or v on an
    element whose reference is finite cannot come out as 'error 0'."""
    p, g, m, v = (t[:1024] for t in R.adam_grid())
    cfg = R.adam_configs(step=10)[0]
    M, V, U, mag = R.adam64(p, g, m, v, *cfg)
    ok = R.adam_bounded(M, V, U)
    tols = R.adam_bounds(p, M, V, U, mag)
    good = R.model_adam(p, g, m, v, *cfg)
    for bad_value in (np.nan, np.inf):
        for which in range(3):
            out = [t.copy() for t in good]
            out[which][5] = bad_value
            errs = R.adam_errors(p, *out, M, V, U)
            worst = [float(R.error_fraction(e, t)[ok].max()) for e, t in zip(errs, tols)]
            assert ok[5] and not np.max(worst) <= 1.0
    worst = [float(R.error_fraction(e, t)[ok].max()) for e, t in zip(R.adam_errors(p, *good, M, V, U), tols)]
    assert np.max(worst) <= 1.0
    assert np.array_equal(R.error_fraction([0.0, 1.0, np.nan, 1.0], [0.0, 0.0, 0.0, 2.0]), [0.0, np.inf, np.nan, 0.5], equal_nan=True)


def test_logit_grid_holds_its_edges():
    z = R.logit_grid()
    assert z.dtype == np.float32 and z.size == R.N_GRID == 4 * 256 * 64 + 3
    bits = set(z.view(np.uint32).tolist())
    lattice = (np.arange(-208, 209) * 0.5).astype(np.float32)
    for want in (lattice, R.logit_edges()):
        assert set(want.view(np.uint32).tolist()) <= bits
    assert np.float32(0.0).view(np.uint32) in bits and np.float32(-0.0).view(np.uint32) in bits
    assert R.logit_edges().size == 2 * 9 + 2
    # the thresholds are where they are said to be: e = 2^-126, 2^-25, 2^-24
    for zk, ek in ((R.Z_FLUSH, 2.0 ** -126), (R.Z_ONE, 2.0 ** -25), (R.Z_ONE_ULP, 2.0 ** -24)):
        assert abs(np.exp(-D(zk)) / ek - 1) < 1e-5
    sig, l1p = R.model_sigmoid_softplus(np.array([-87.0, -88.0, 16.5, 17.5, -17.5], dtype=np.float32))
    assert sig[0] > 0 and sig[1] == 0 and sig[2] < 1 and sig[3] == 1 and 0 < sig[4] == l1p[4]      # flushed; 1 + e == 1: l1p = e = sig
    mag = np.abs(z[z != 0])
    assert mag.min() < 1e-29 and mag.max() == 104 and np.sum(z < 0) > 30000 and np.sum(z > 0) > 30000
    assert np.all(np.abs(z[-3:]) > 16)                       # the scalar tail works on the large-|z| paths too
    for k in BANDS:
        b = R.band_logits(k)
        assert b.size == R.N_GRID and np.all((np.abs(b) >= k) & (np.abs(b) <= k + 1)) and 0.4 < np.mean(b > 0) < 0.6


def test_adam_grids_hold_their_ranges_and_special_values():
    p, g, m, v = R.adam_grid()
    for name, t in (("g", g), ("m", m), ("v", v), ("p", p)):
        lo, hi = R.ADAM_RANGES[name]
        a = np.abs(D(t))
        assert t.size == R.N_GRID and a.min() >= lo * (1 - 1e-6) and a.max() <= hi * (1 + 1e-6)
        assert a.min() < lo * 1.01 and a.max() > hi / 1.01                       # the ends are reached
        decades = np.floor(np.log10(a)).astype(int)
        assert len(set(decades.tolist())) >= int(round(np.log10(hi / lo)))        # and every decade between
    assert np.all(v > 0) and all(0.45 < np.mean(t < 0) < 0.55 for t in (p, g, m))
    assert len(R.adam_configs()) == 96 and len(R.adam_configs(step=10)) == 16
    sp, sg, sm, sv = R.adam_special_grid()
    assert sp.size % 4 == 3                                                       # float4 body and scalar tail
    assert sp[0] == 0 and sg[0] == 0 and not np.signbit(sg[0]) and sm[0] == 0 and sv[0] == 0        # the all-zero state
    tiny = float(np.finfo(np.float32).tiny)
    with np.errstate(over="ignore", under="ignore"):
        assert 0 < np.float32(1e-42) < tiny and 0 < np.float32(3e-23) ** 2 < tiny and np.isinf(np.float32(2e19) ** 2)
    assert 0 < np.float32(R.SUBNORMAL) < tiny
    assert np.any((sg == 0) & np.signbit(sg)) and np.any(np.isposinf(sg)) and np.any(np.isneginf(sg)) and np.any(np.isnan(sg))
    for val in (1e-42, 3e-23, 2e19):
        for mm in (0.0, R.SUBNORMAL):
            for vv in (0.0, R.SUBNORMAL):
                assert np.any((sg == np.float32(val)) & (sm == np.float32(mm)) & (sv == np.float32(vv)))
    assert np.array_equal(R.value_class(np.array([0.0, -0.0, 1e-40, -3.0, np.inf, -np.inf, np.nan], dtype=np.float32)), [0, 0, 1, 1, 2, 3, 4])
