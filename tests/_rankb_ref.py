"""What the tests of the rank-B optimizer pass (``dd_adam_step_rankb``, csrc/adam_rankb.hip) share, without the package: the cases and
the class each belongs to, the host arithmetic of the launcher restated (``plan``), the fp64 gradient (``grad64``) and the per-element
checker of one step from zero moments (``check_first_step``).  CPU only (torch).

The checker's bounds are derived, not measured.  From ``m0 = v0 = 0``, ``step = 1``, ``grad_scale = 1`` the element (``adam_elem2`` of
csrc/dd_adam.h, contraction off) is ``m = fl(g omb1)``, ``v = fl(fl(g omb2) g)`` with ``omb = 1.f - fp32(beta)`` and g the kernel's fp32
gradient, so with ``gt = m / omb1`` taken in fp64:

* ``|gt - g64| <= (rows + 3) 2^-24 S + 2^-120``, ``S = |dy|^T |x|``: an fp32 sum of ``rows`` products in any order and any mixture of
  fused and rounded multiply-adds is within ``rows u S`` of the exact one to first order (u = 2^-24), the multiply by omb1 adds one
  rounding of at most ``u |g| <= u S``; the two spare units hold the second-order terms (``rows <= 64``).
* ``|v - omb2 gt^2| <= 5 2^-24 omb2 gt^2 + 2^-120``: v carries two roundings, gt^2 twice the one of m: four units to first order.
* the same two for ``bias_m`` and ``bias_v`` with ``S = sum_b |dy_b|`` (a sequential fp32 sum of ``rows`` terms).

2^-120 is the absolute floor under which fp32 results may be subnormal.  A NaN or an infinity anywhere fails.
"""
import torch

NUM_CU = 256                       # DD_NUM_CU of csrc/dd_common.h
U24, FLOOR = 2.0 ** -24, 2.0 ** -120
F32, F64 = torch.float32, torch.float64

# rows, n, k, blocks per CU, spare CUs -> form, total, grid, per, straddles, has_empty_piece (plan() below; tests/test_rankb_ref.py asserts
# every line, so that a change of the dispatch breaks the table and does not silently move a case to another kernel)
CASES = []


def _case(rows, n, k, blocks, spare, form, total, grid, per, straddles, empty):
    for r in rows:
        CASES.append(((r, n, k, blocks, spare), (form, total, grid, per, straddles, empty)))


# the head's form on 301 n-groups (the last one of 2 n-tiles, its last n-tile of 4 rows): 3 and 2 groups per workgroup, the dY prefetch of
# the next group, workgroups past the end of the list
_case((9, 32), 19220, 64, 1, 128, "short", 301, 128, 3, True, True)
_case((9, 32), 19220, 64, 1, 0, "short", 301, 256, 2, True, True)
# the 48-row head: two chunks, one k-tile per n-group -- new dY behind the barrier for every tile
_case((48,), 19220, 64, 1, 128, "lds<2,1>", 301, 128, 3, True, True)
# 5 n-groups x 33 k-tiles in pieces of 2: every other piece straddles an n-group (dY reloaded in the middle of a piece)
_case((25,), 260, 2052, 1, 128, "lds<1,2>", 165, 128, 2, True, True)
# the same with 1, 8, 16, 25 and 31 rows in the second 32-row chunk
_case((33, 40, 48, 57, 63), 260, 2052, 1, 128, "lds<2,1>", 165, 128, 2, True, True)
# rows past M inside the second half of the chunk (x rows 16 .. 31: fetched through the wave-uniform offset of the load)
_case((17, 20, 25), 52, 132, 1, 0, "lds<1,2>", 3, 3, 1, False, False)
# 31 n-tiles x 19 slabs of 256 columns = 589 > 512 workgroups: the wrap to the next n-tile and its dY reload in the middle of a piece
_case((17, 32), 484, 4620, 4, 128, "wide", 589, 512, 2, True, True)


def plan(rows, n, k, blocks_per_cu=1, spare_cus=0):
    """rankb_launch's host arithmetic (csrc/adam_rankb.hip) -> (form, total, grid, per, straddles, has_empty_piece).  ``straddles``: some
    workgroup's piece of the work list holds items of two n-groups (``wide``: two n-tiles; ``short``: an item IS an n-group) -- the dY
    tile changes inside the piece; ``has_empty_piece``: some workgroup's piece starts past the end of the list."""
    ntile_n, ntile_k = (n + 15) // 16, (k + 63) // 64
    short = rows <= 32 and ntile_k == 1
    wide = rows <= 32 and not short and ntile_k >= 64 and blocks_per_cu > 1
    if wide:
        form, group = "wide", (k + 255) // 256
        total = ntile_n * group
    else:
        form = "short" if short else ("lds<1,2>" if rows <= 32 else "lds<2,1>")
        group = 1 if short else ntile_k
        total = (ntile_n + 3) // 4 * group
    grid = min(total, max(NUM_CU - spare_cus, 1) * blocks_per_cu)
    per = (total + grid - 1) // grid
    pieces = [(b * per, min((b + 1) * per, total)) for b in range(grid)]
    straddles = any(lo < hi and lo // group != (hi - 1) // group for lo, hi in pieces)
    empty = any(lo >= hi for lo, hi in pieces)
    return form, total, grid, per, straddles, empty


def omb(beta):
    """1.f - fp32(beta) as the launcher computes it, as a double."""
    return float(torch.tensor(1.0, dtype=F32) - torch.tensor(beta, dtype=F32))


def factors(rows, n, k, signed, step, gen):
    """x [rows, k], dy [rows, n] of one step, drawn as tests/test_gpu_round5.py::test_adam_rankb_matches_fp64 draws them."""
    x = torch.rand(rows, k, generator=gen) - (0.5 if signed else 0.0)
    dy = (torch.rand(rows, n, generator=gen) - (0.5 if signed else 0.0)) * 0.1 * step
    return x, dy


def grad64(dy, x, scale=1.0):
    """(dW, db) = (dy^T x, column sums of dy) x scale, in fp64."""
    yd, xd = dy.double().cpu(), x.double().cpu()
    return yd.t() @ xd * scale, yd.sum(0) * scale


def _worst(err, bound):
    frac = err / bound
    frac = torch.where(torch.isfinite(frac), frac, torch.full_like(frac, float("inf")))      # a NaN or an infinity anywhere fails
    return float(frac.max())


def first_step_fractions(dy, x, m, v, bias_m=None, bias_v=None, beta1=0.9, beta2=0.999):
    """The worst fraction of each derived bound (module docstring) that ``m``, ``v`` (and the bias moments) use after ONE step from zero
    moments with ``grad_scale = 1`` on the factors ``dy``, ``x``: {"m": .., "v": .., "bias_m": .., "bias_v": ..}; above 1 is a failure."""
    rows = dy.shape[0]
    o1, o2 = omb(beta1), omb(beta2)
    g64, b64 = grad64(dy, x)
    s_w = dy.double().cpu().abs().t() @ x.double().cpu().abs()
    s_b = dy.double().cpu().abs().sum(0)
    out = {}
    for name, mm, vv, ref, s in (("m", m, v, g64, s_w), ("bias_m", bias_m, bias_v, b64, s_b)):
        if mm is None:
            continue
        gt = mm.detach().double().cpu() / o1
        out[name] = _worst((gt - ref).abs(), (rows + 3) * U24 * s + FLOOR)
        want_v = o2 * gt * gt
        out[name.replace("m", "v")] = _worst((vv.detach().double().cpu() - want_v).abs(), 5 * U24 * want_v + FLOOR)
    return out


def check_first_step(dy, x, m, v, bias_m=None, bias_v=None, beta1=0.9, beta2=0.999):
    """Assert that every element is inside its bound; returns the fractions."""
    frac = first_step_fractions(dy, x, m, v, bias_m, bias_v, beta1, beta2)
    bad = {k: f for k, f in frac.items() if not f <= 1.0}
    assert not bad, f"outside the derived bound (fraction of it used): {bad}; all: {frac}"
    return frac


def model_first_step(dy, x, sequential=False, beta1=0.9, beta2=0.999):
    """An fp32 candidate of the first step on the CPU -> (m, v, bias_m, bias_v): the gradient as ``dy.T @ x`` in fp32, or summed row by
    row; then the element's three rounded multiplies."""
    dy, x = dy.to(F32), x.to(F32)
    if sequential:
        g, b = torch.zeros(dy.shape[1], x.shape[1]), torch.zeros(dy.shape[1])
        for r in range(dy.shape[0]):
            g = g + dy[r][:, None] * x[r][None, :]
            b = b + dy[r]
    else:
        g, b = dy.t() @ x, dy.sum(0)
    o1, o2 = torch.tensor(omb(beta1), dtype=F32), torch.tensor(omb(beta2), dtype=F32)
    return g * o1, (g * o2) * g, b * o1, (b * o2) * b
