"""fp64 references, fp32 models, input grids and error bounds for the two element functions every dense loss and every optimizer pass
is made of: ``dd_sigmoid_softplus`` (csrc/dd_device.h) and ``adam_elem2`` / ``adam_elem`` (csrc/dd_adam.h).  CPU only (numpy): imported by
tests/test_element_ref.py, which proves that the bounds can be met, and by tests/test_gpu_element_range.py, which holds the kernels to them.

Three layers:

* the fp64 REFERENCE of each operation (``sigmoid64``, ``softplus64``, ``bce_logits_terms64``, ``adam64``);
* an fp32 MODEL of each element: the header's operation sequence in numpy float32, every fused multiply-add rounded once, and
  exp2 / log2 / sqrt / 1/x CORRECTLY ROUNDED where the hardware instructions (v_exp_f32, v_log_f32, v_sqrt_f32, v_rcp_f32) are good to
  1 ulp.  What the model loses against the reference is the cost of the FORMULA in fp32; a bound is that, rounded up, plus an allowance
  of 1 ulp per hardware primitive on the path.  No constant here was taken from a kernel's output;
* the GRIDS both are judged on, with the edge values of each domain placed in them by construction.
"""
import numpy as np

F = np.float32
D = np.float64
U24 = 2.0 ** -24                 # half an ulp of a number in [1, 2): the unit of every bound below
TINY = 2.0 ** -126               # smallest normal fp32; results below it are flushed by the hardware transcendentals
FMAX = float(np.finfo(np.float32).max)
N_GRID = 4 * 256 * 64 + 3        # 65 539: the float4 body, more than one 256-thread block, and a 3-element scalar tail

LOG2E = F(1.4426950408889634)    # the constants as dd_sigmoid_softplus spells them, rounded to fp32 as the compiler does
LN2 = F(0.6931471805599453)


# ------------------------------------------------------------------------------------------------ fp64 references
def sigmoid64(z):
    z = np.asarray(z, dtype=D)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(-np.abs(z))
        return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus64(z):
    """log1p(exp(-|z|)): the transcendental term of BCE-with-logits."""
    with np.errstate(under="ignore"):
        return np.log1p(np.exp(-np.abs(np.asarray(z, dtype=D))))


def bce_logits_terms64(z, t):
    """Per-element BCE-with-logits max(z, 0) - z t + log1p(exp(-|z|))."""
    z, t = np.asarray(z, dtype=D), np.asarray(t, dtype=D)
    return np.maximum(z, 0.0) - z * t + softplus64(z)


def adam_params(lr, b1, b2, eps, step, grad_scale):
    """The parameter values the kernels work with: lr, betas, eps and the scale are fp32 arguments, 1 - beta is an fp32 subtraction, and
    the bias corrections are fp64 on the host from the fp32 betas (tests/test_gpu_round5.py::_adam64 argues the betas)."""
    lr, b1, b2, eps, gs = F(lr), F(b1), F(b2), F(eps), F(grad_scale)
    bc1 = 1.0 - D(b1) ** D(step)
    bc2 = 1.0 - D(b2) ** D(step)
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, gs=gs, omb1=F(F(1) - b1), omb2=F(F(1) - b2), bc1=bc1, bc2=bc2)


def adam64(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0):
    """One step of torch.optim.Adam in fp64 on fp32 state.  Returns M, V, the update U = p_new - p, and the conditioning magnitude
    |b1 m| + |(1 - b1) g scale| of M (a sum of two signed terms: its rounding is relative to that, not to |M|)."""
    q = adam_params(lr, b1, b2, eps, step, grad_scale)
    g, m, v = np.asarray(g, dtype=D), np.asarray(m, dtype=D), np.asarray(v, dtype=D)
    with np.errstate(all="ignore"):
        G = g * D(q["gs"])
        t0, t1 = D(q["b1"]) * m, D(q["omb1"]) * G
        M = t0 + t1
        V = D(q["b2"]) * v + D(q["omb2"]) * G * G
        U = -(D(q["lr"]) / q["bc1"]) * M / (np.sqrt(V) / np.sqrt(q["bc2"]) + D(q["eps"]))
        return M, V, U, np.abs(t0) + np.abs(t1)


def adam_bounded(M, V, U):
    """Elements whose reference is finite and, where not exactly zero, normal in fp32: the only ones held to the relative bounds (below
    2^-126 fp32 has no relative precision to hold anything to, and the hardware square root and reciprocal flush)."""
    ok = np.ones(np.shape(M), dtype=bool)
    with np.errstate(invalid="ignore"):
        for r in (M, V, U):
            a = np.abs(r)
            ok &= np.isfinite(r) & ((a == 0) | ((a >= TINY) & (a <= FMAX)))
    return ok


# ------------------------------------------------------------------------------------------------ fp32 models
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding.  The product of two fp32 is exact in fp64; the fp64 sum is rounded to odd when it is inexact and
    sits on an fp32 tie, so that the second rounding (to fp32) cannot differ from a single one."""
    with np.errstate(all="ignore"):
        prod = D(a) * D(b)
        c = np.broadcast_to(D(c), np.shape(prod)).astype(D)
        s = prod + c
        bb = s - prod
        err = (prod - (s - bb)) + (c - bb)                      # two-sum: prod + c == s + err exactly (finite operands)
        tie = np.isfinite(s) & (err != 0) & ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000))
        s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)      # the exact sum lies on err's side of s
        return s.astype(F)


def _flush(x):
    return np.where(np.abs(x) < F(TINY), F(0) * x, x).astype(F)


def model_sigmoid_softplus(z):
    """dd_sigmoid_softplus in numpy float32, operation for operation -> (sig, l1p)."""
    z = np.asarray(z, dtype=F)
    with np.errstate(all="ignore"):
        a = (-np.abs(z) * LOG2E).astype(F)
        e = _flush(np.exp2(a.astype(D)).astype(F))              # v_exp_f32 flushes results below 2^-126
        u = (F(1) + e).astype(F)
        d = (u - F(1)).astype(F)                                # exact
        r = (1.0 / u.astype(D)).astype(F)
        r = fma32(r, fma32(-u, r, F(1)), r)                     # one Newton step
        sig = np.where(z >= 0, r, (e * r).astype(F)).astype(F)
        lg = (np.log2(u.astype(D)).astype(F) * LN2).astype(F)
        rd = (1.0 / d.astype(D)).astype(F)
        l1p = np.where(d == 0, e, (lg * (e * rd).astype(F)).astype(F)).astype(F)
    return sig, l1p


def model_adam(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0):
    """adam_elem2 in numpy float32 with the host's parameter preparation (dd_adam.h adam_bias / adam_kernel) -> (p, m, v).  m and v use
    multiplies and fused multiply-adds only, which are IEEE on the device: they are what the kernels must give bit for bit."""
    q = adam_params(lr, b1, b2, eps, step, grad_scale)
    p, g, m, v = (np.asarray(t, dtype=F) for t in (p, g, m, v))
    bc1, bc2_sqrt = F(q["bc1"]), F(np.sqrt(q["bc2"]))
    step_size = F(q["lr"] / bc1)
    inv_bc2 = F(F(1) / bc2_sqrt)
    with np.errstate(all="ignore"):
        gg = (g * q["gs"]).astype(F)
        mm = fma32(q["b1"], m, (gg * q["omb1"]).astype(F))
        vv = fma32(q["b2"], v, ((gg * q["omb2"]).astype(F) * gg).astype(F))
        # v_sqrt_f32 and v_rcp_f32 flush arguments and results below 2^-126; the model does not need to: the denominator lies between eps
        # and 1e21, so the reciprocal never gets there, and the square root does only for a subnormal v, whose reference V is subnormal
        # too -- adam_bounded() leaves such elements out of every bound
        s = np.sqrt(vv.astype(D)).astype(F)
        denom = fma32(s, inv_bc2, q["eps"])
        r = (1.0 / denom.astype(D)).astype(F)
        pn = fma32(-step_size, (mm * r).astype(F), p)
    return pn, mm, vv


# ------------------------------------------------------------------------------------------------ grids
def _ulp_neighbours(x):
    x = np.asarray(x, dtype=F)
    return np.concatenate([np.nextafter(x, F(0)), x, np.nextafter(x, F(np.inf))])


# |z| at which e = exp(-|z|) drops below 2^-126 and is flushed; at which e = 2^-24, the tie of 1 + e (round to even: from there on
# 1 + e == 1, u - 1 == 0 and the softplus is e itself); and at which e = 2^-25, one binade further into that branch
Z_FLUSH = F(126 * np.log(2.0))                 # 87.34
Z_ONE = F(25 * np.log(2.0))                    # 17.33: e = 2^-25
Z_ONE_ULP = F(24 * np.log(2.0))                # 16.64: e = 2^-24, above it 1 + e == 1


def logit_edges():
    """The edge logits, both signs: +-0, and k, k +- 1 ulp for the three thresholds."""
    k = _ulp_neighbours([Z_FLUSH, Z_ONE, Z_ONE_ULP])
    return np.concatenate([k, -k, np.array([0.0, -0.0], dtype=F)]).astype(F)


def logit_grid():
    """N_GRID logits: every integer and half-integer in [-104, 104], the edges, and log-uniform magnitudes 1e-30 .. 100 of both signs."""
    rs = np.random.RandomState(20240)
    lattice = (np.arange(-208, 209) * 0.5).astype(F)
    fixed = np.concatenate([lattice, logit_edges()])
    k = N_GRID - fixed.size
    mag = np.exp(rs.uniform(np.log(1e-30), np.log(100.0), k))
    z = np.concatenate([fixed, (mag * rs.choice([-1.0, 1.0], k)).astype(F)]).astype(F)
    rs.shuffle(z)                                             # the edges land in the vector body and, by the next line, in the tail
    z[-3:] = np.array([Z_ONE, -Z_FLUSH, -16.5], dtype=F)
    z[:2] = np.array([0.0, -0.0], dtype=F)
    return z


def band_logits(k, n=N_GRID, seed=0):
    """n logits with |z| uniform in [k, k + 1] and random signs: one band of a confident head."""
    rs = np.random.RandomState(1000 + 17 * k + seed)
    return (rs.uniform(k, k + 1.0, n) * rs.choice([-1.0, 1.0], n)).astype(F)


def softplus_points():
    """Logits for single-element launches, signs alternating: |z| every integer and half-integer up to 104 (209 points), then the |z| at
    which exp(-|z|) is k ulps of 1 (k 2^-23) for k = 1 .. 64, and the same a little further out (e just under k ulps)."""
    near_one = -np.log(np.arange(1, 65) * 2.0 ** -23)
    z = np.concatenate([np.arange(0, 209) * 0.5, near_one, near_one * (1 + 2.0 ** -12)]).astype(F)
    z[1::2] *= -1
    return z


def exact_sigmoid_logits(n=4 * 256 * 64):
    """z uniform in [3, 17.4]: positive logits whose u = fl(1 + e) is not yet 1 and whose e is small enough for u to be determined (below
    z = 3 the exponential's allowed error is wider than the gap between two ties of 1 + e)."""
    return np.random.RandomState(99).uniform(3.0, 17.4, n).astype(F)


def exact_sigmoid(z):
    """(known, bits): for z >= 0 the sigmoid is the refined reciprocal of u = fl(1 + e) alone, and one Newton step from ANY start good
    to an ulp or two lands on fl((1 / u)(1 - eps^2)), eps^2 <= 2^-44: the correctly rounded reciprocal of u unless 1 / u is within that
    of a rounding tie.  u itself is known wherever 1 + exp(-z) is further from a tie of fp32 than twice the error the exponential is
    allowed ((|z| + 11) 2^-24 relative, the sigmoid bound for z < 0, which holds the kernel's e).  ``known`` marks the logits where both
    hold; there the probability is determined to the BIT by the formula, whatever the hardware instructions round."""
    z = np.asarray(z, dtype=F)
    with np.errstate(all="ignore"):
        e = np.exp(-D(z))
        x = 1.0 + e
        frac = e * 2.0 ** 23
        from_tie = np.abs(frac - np.floor(frac) - 0.5) * 2.0 ** -23
        u = x.astype(F)
        rr = 1.0 / D(u)
        r = rr.astype(F)
        tie_r = 0.5 * D(np.spacing(r)) - np.abs(rr - D(r))
        known = (z >= 0) & (e < 0.9) & (from_tie > 2 * (np.abs(D(z)) + SIG_BOUND_K) * U24 * e) & (tie_r > 2.0 ** -40 * rr)
    return known, r


ADAM_RANGES = dict(g=(1e-15, 1e15), m=(1e-15, 1e15), v=(1e-30, 1e30), p=(1e-6, 1e2))


def adam_grid(n=N_GRID, seed=7):
    """(p, g, m, v) fp32, log-uniform over ADAM_RANGES; p, g, m with random signs."""
    rs = np.random.RandomState(seed)

    def logu(lo, hi, signed):
        x = np.exp(rs.uniform(np.log(lo), np.log(hi), n))
        return (x * rs.choice([-1.0, 1.0], n) if signed else x).astype(F)
    g = logu(*ADAM_RANGES["g"], True)
    m = logu(*ADAM_RANGES["m"], True)
    v = logu(*ADAM_RANGES["v"], False)
    p = logu(*ADAM_RANGES["p"], True)
    return p, g, m, v


ADAM_STEPS = (1, 2, 10, 1000, 100000, 2 ** 31 - 1)
ADAM_BETAS = ((0.9, 0.999), (0.5, 0.9))
ADAM_EPS = (1e-8, 1e-3)
ADAM_LR = (1e-3, 1.0)
ADAM_SCALES = (1.0, 0.37)


def adam_configs(step=None):
    """(lr, b1, b2, eps, step, grad_scale) over the whole product, or over one step's 16."""
    return [(lr, b1, b2, eps, s, gs) for s in (ADAM_STEPS if step is None else (step,)) for b1, b2 in ADAM_BETAS for eps in ADAM_EPS
            for lr in ADAM_LR for gs in ADAM_SCALES]


SUBNORMAL = 1e-40
G_SPECIAL = (0.0, -0.0, 1e-42, 3e-23, 2e19, np.inf, -np.inf, np.nan)      # 1e-42: subnormal; 3e-23: g^2 subnormal; 2e19: g^2 overflows


def adam_special_grid():
    """(p, g, m, v): every special gradient against m, v in {0, subnormal} and p in {0, 1}; the all-zero state is element 0 (g = 0,
    m = v = p = 0).  67 elements: 16 float4 groups and a 3-element tail, the last three repeating the infinities and the NaN there."""
    rows = [(p, g, m, v) for g in G_SPECIAL for m in (0.0, SUBNORMAL) for v in (0.0, SUBNORMAL) for p in (0.0, 1.0)]
    rows += [(1.0, np.inf, 0.0, 0.0), (1.0, -np.inf, SUBNORMAL, 0.0), (0.0, np.nan, 0.0, SUBNORMAL)]
    a = np.array(rows, dtype=F)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy()


def value_class(x):
    """0 zero, 1 finite non-zero, 2 +inf, 3 -inf, 4 NaN."""
    x = np.asarray(x)
    c = np.ones(x.shape, dtype=np.int8)
    c[x == 0] = 0
    c[np.isposinf(x)] = 2
    c[np.isneginf(x)] = 3
    c[np.isnan(x)] = 4
    return c


# ------------------------------------------------------------------------------------------------ bounds
# sigmoid, z >= 0: r = 1 / fl(1 + e).  The rounding of 1 + e is up to 2^-24 of u in [1, 2], which 1/u passes on scaled by 1/u^2 <= 1; the
# refined reciprocal rounds once more (half an ulp of [0.5, 1]: 2^-25); e's own error is e (0.72 |z| + 1) 2^-24 / u^2 < 0.4 * 2^-24.
# CPU model, worst on logit_grid() and the nine bands: 1.55 x 2^-24 (tests/test_element_ref.py prints it).  The hardware allowance is one:
# v_exp_f32's ulp of e reaches sig as e / u^2 <= 1/4 ulp, and v_rcp_f32's ulp is squared by the Newton step.
SIG_POS_MODEL = 2 * U24
SIG_POS_BOUND = 3 * U24
# sigmoid, z < 0, and the softplus: relative error (|z| + k) 2^-24.  The |z| is the rounding of the exponent a = -|z| log2(e): half an ulp
# of a is up to 2^-24 |a| (reached when |a| is just above a power of two), and exp2 turns an absolute error of the exponent into a relative
# one of ln2 * 2^-24 |a| = 2^-24 |z|.  The rounded constant log2(e) (1.3e-8 low) adds 0.22 |z| 2^-24 more, which the "+ k" has to carry:
# the bounds (|z| + 11, |z| + 12) are the ones the element was given, and hold ON THESE GRIDS, not for every fp32 logit -- past
# |z| = 40 a logit whose exponent rounds the wrong way from just above 64 would need 1.22 |z| + 3.
# CPU model, worst on logit_grid() and the nine bands: sig and softplus both |z| + 8.20, at z = -+45 (a = 64.92, the constant's share
# is 9.9 there); below |z| = 44 the model needs |z| + 4.6.  So of the bound's 11 (12) the formula takes 9 at that point and the hardware
# primitives -- v_exp_f32, the refined reciprocal, one multiply; for the softplus v_log_f32 and the plain v_rcp_f32 -- have 2 (3) left.
SIG_MODEL_K, SIG_BOUND_K = 9, 11
SP_MODEL_K, SP_BOUND_K = 9, 12
LOSS_WRONG_BOUND = 4 * U24       # mean loss with every target wrong: terms |z| + softplus, relative


def sig_bound(z, ref, k=SIG_BOUND_K, pos=SIG_POS_BOUND):
    z = np.asarray(z, dtype=D)
    return np.where(z >= 0, pos, (np.abs(z) + k) * U24 * ref + TINY)


def softplus_bound(z, ref, k=SP_BOUND_K):
    return (np.abs(np.asarray(z, dtype=D)) + k) * U24 * ref + TINY


def band_mean_bound(k, z, t):
    """Relative bound on the mean BCE-with-logits of a band |z| in [k, k + 1].  Terms whose target agrees with the sign of z are the
    softplus alone and get its bound at |z| = k + 1; terms whose target is wrong are |z| + softplus and get LOSS_WRONG_BOUND; every term is
    positive, so the mean's error is at most the two weighted by their share of the sum."""
    terms = bce_logits_terms64(z, t)
    right = np.asarray(t) == (np.asarray(z) > 0)
    s_right, s_wrong = terms[right].sum(), terms[~right].sum()
    return ((k + 1 + SP_BOUND_K) * U24 * s_right + LOSS_WRONG_BOUND * s_wrong) / (s_right + s_wrong)


# Adam.  The CPU model's worst case over adam_configs() (all 96) on adam_grid(), in units of 2^-24 (tests/test_element_ref.py asserts
# them and prints the figures):
#   v            3.94 relative                 -> ceil 4      (five roundings of at most 2^-24 each: g scale twice, two multiplies, the fma)
#   m            2.44 of the magnitude         -> ceil 3      (three: g scale, one multiply, the fma)
#   the update   2.38 of |U| beyond m's share  -> ceil 3      (m's share taken at its rounded-up 3)
# plus 2 for v_sqrt_f32 and v_rcp_f32 at 1 ulp each.  (m and v meet neither instruction; tests/test_gpu_element_range.py also holds them
# to the model's bits.)
ADAM_MODEL_KV, ADAM_MODEL_KM, ADAM_MODEL_KU = 4, 3, 3
ADAM_HW = 2
ADAM_KV, ADAM_KM, ADAM_KU = ADAM_MODEL_KV + ADAM_HW, ADAM_MODEL_KM + ADAM_HW, ADAM_MODEL_KU + ADAM_HW


def adam_bounds(p, M, V, U, mag, kv=ADAM_KV, km=ADAM_KM, ku=ADAM_KU):
    """Absolute tolerances (tol_m, tol_v, tol_u) for m, v and p_new - p (differences taken in fp64 from the fp32 tensors).  The update
    carries m's error scaled by U / M, its own ku, and half an ulp of the larger of p and p + U for the final rounding of p."""
    with np.errstate(all="ignore"):
        tol_m = km * U24 * mag
        tol_v = kv * U24 * np.abs(V)
        share = np.where(M != 0, mag / np.abs(M), 0.0)
        big = np.maximum(np.abs(D(p)), np.abs(D(p) + U))
        half_ulp = 0.5 * D(np.spacing(np.minimum(big, FMAX).astype(F)))
        tol_u = (km * share + ku) * U24 * np.abs(U) + half_ulp
    return tol_m, tol_v, tol_u


def error_fraction(err, tol):
    """err / tol per element, for a worst-case ``.max()``: 0 only for the true 0 / 0 (no error against a zero tolerance), inf for any error
    against a zero tolerance, and NaN wherever the output was NaN -- numpy's max keeps it, and ``NaN <= 1`` is false."""
    err, tol = np.asarray(err, dtype=D), np.asarray(tol, dtype=D)
    with np.errstate(all="ignore"):
        return np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.where(np.isnan(err), np.nan, np.inf)))


def adam_errors(p_old, p_new, m_new, v_new, M, V, U):
    """|error| of m, v and the update, fp64 differences of fp32 tensors."""
    with np.errstate(all="ignore"):
        return np.abs(D(m_new) - M), np.abs(D(v_new) - V), np.abs((D(p_new) - D(p_old)) - U)
