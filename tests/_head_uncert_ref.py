"""Reference of include/dd_head_uncert.h's semantics, for the CPU and the GPU tests of the sampled head's uncertainty.  CPU only
(numpy); the GPU tests hand it CPU copies.

Three layers, as tests/_element_ref.py and tests/_head_mean_ref.py:

* ``stats_from_logits(z32, S)``: everything in fp64 from the PRODUCT'S OWN fp32 logits (``ops.linear`` delivers them with the kernel's
  bits), with the TIGHT bounds: what the header's formulas may lose in fp32, and nothing of the GEMM;
* ``stats64(x, w, bias, S)``: pure fp64 from the operands, with the LOOSE bounds: the tight ones plus the logits' ``KERNEL_BOUND * peak``
  carried through each statistic's slope;
* ``model32(z32, S)``: the header's operation sequence in numpy float32 with correctly rounded primitives
  (``_element_ref.model_sigmoid_softplus``; ln as fp64 rounded once).  tests/test_head_uncert_ref.py shows with it that the tight bounds
  are met by the formulas alone.  No constant here was taken from a kernel's output.

THE BOUNDS, all absolute, per element, in units of U = 2^-24 (half an ulp of [1, 2): the relative error of one rounded fp32
operation).  csrc/dd_device.h states the element's error model: ``sig`` within 3 U absolute for z >= 0 and within (|z| + 11) U
relative for z < 0; ``l1p`` within (|z| + 12) U relative (``_element_ref.sig_bound`` / ``softplus_bound``, TINY for the flush to zero).

  p       e_p = sig_bound(z, p)
  mean    S - 1 adds of partial sums that stay below S, each within U of the partial: (S - 1) U of the mean; one multiply and the
          rounded constant (float)(1 / S): 2 U.                                   e_m = mean_s e_p + (S + 1) U
  var     d = p - m carries e_d = e_p + e_m + U |d| (the subtract); d^2 carries 2 |d| e_d + e_d^2 and its multiply's U d^2; S - 1 adds,
          the multiply and the constant: (S + 1) U of the sum.    e_v = t + (S + 2) U (var + t),  t = mean_s (2 |d| e_d + e_d^2)
  h       l1p and q = sigmoid(-|z|) relative (|z| + 12) U and (|z| + 11) U, the multiply |z| q and the add one U each (|z| is exact:
          the reference starts from the same fp32 logit).                          e_h = (|z| + 13) U h + 2 TINY (1 + |z|)
  expected                                                                          e_x = mean_s e_h + (S + 1) U ln 2     (h <= ln 2)
  entropy H(m_hat) against H(m), |m_hat - m| <= e_m.  The transfer: the slope |ln(m / (1 - m))| times e_m, the slope taken at the end
          of [m - e_m, m + e_m] that is further from 1/2 (the slope grows towards 0 and 1: at the element's own m it is a first-order
          statement only); where that interval reaches 0 or 1 the slope is unbounded and the identity |H(a) - H(b)| <= H(|a - b|)
          bounds it instead; the smaller of the two.  The formula: 1 - m is exact for m >= 1/2 and within U / 2 below, where the
          term's slope |ln(1 - m) + 1| is at most 1; logf within 1 ulp = 2 U relative, each product U, the final subtract U: 4 U H + U.
                                                                                    e_H = transfer + 4 U (H + transfer) + U
  mi      the subtract of two numbers below ln 2, and |max(a, 0) - max(b, 0)| <= |a - b|.       e_i = e_H + e_x + U ln 2
  scores  means over n pixels in fp64 of fp32 values: the mean of the elements' bounds, plus n 2^-52 of the mean for the fp64 adds.

A few 10^-6 at S = 64, a few 10^-7 at S = 2.  The loose bounds replace e_p by e_p + dz / 4 (the sigmoid's slope is at most 1/4) and e_h by
e_h + dz / 4 (|dh/dz| = |z| p (1 - p) <= 0.2239), dz = KERNEL_BOUND * max |z|, take |z| + dz in the relative terms, and use the
identity alone for the entropy's transfer.
"""
from collections import namedtuple

import numpy as np

import _element_ref as er
from _head_mean_ref import KERNEL_BOUND

F, D, U, TINY = er.F, er.D, er.U24, er.TINY
LN2 = float(np.log(2.0))
STATS = ("entropy", "mi", "var")      # the columns of ``scores``

Stats = namedtuple("Stats", "mean entropy expected mi var scores")


def xlogx(f):
    """-(f ln f) in fp64, 0 at 0."""
    f = np.asarray(f, dtype=D)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(f == 0, 0.0, -f * np.log(np.where(f == 0, 1.0, f)))


def entropy64(m):
    """Binary entropy in nats."""
    m = np.asarray(m, dtype=D)
    return xlogx(m) + xlogx(1.0 - m)


def draw_entropy64(z):
    """The entropy of one draw from its logit: softplus(-|z|) + |z| sigmoid(-|z|)."""
    a = np.abs(np.asarray(z, dtype=D))
    with np.errstate(under="ignore"):
        e = np.exp(-a)
        return np.log1p(e) + a * (e / (1.0 + e))


def _scores(entropy, mi, var):
    return np.stack([entropy.mean(-1), mi.mean(-1), var.mean(-1)], axis=-1)


def _reference(z, samples):
    """fp64 logits [scenes * S, n] -> Stats (fp64), and the per-draw pieces the bounds need."""
    z = np.asarray(z, dtype=D)
    n = z.shape[1]
    z = z.reshape(-1, samples, n)
    p = er.sigmoid64(z)
    h = draw_entropy64(z)
    mean = p.mean(1)
    entropy, expected = entropy64(mean), h.mean(1)
    mi = np.maximum(entropy - expected, 0.0)
    d = p - mean[:, None]
    var = (d * d).mean(1)
    return Stats(mean, entropy, expected, mi, var, _scores(entropy, mi, var)), z, p, h, d


def _bounds(ref, z, p, h, d, samples, dz=0.0, identity_only=None):
    """Stats of absolute bounds for ``ref`` (see the module docstring); ``dz``: how far the logits themselves may be off;
    ``identity_only``: the entropy's transfer from the identity alone (the default under ``dz``)."""
    az = np.abs(z) + dz
    e_p = np.where(z >= 0, er.SIG_POS_BOUND, (az + er.SIG_BOUND_K) * U * p + TINY) + 0.25 * dz
    e_m = e_p.mean(1) + (samples + 1) * U
    e_d = e_p + e_m[:, None] + U * np.abs(d)
    t = (2 * np.abs(d) * e_d + e_d * e_d).mean(1)
    e_v = t + (samples + 2) * U * (ref.var + t)
    e_h = (az + 13) * U * h + 2 * TINY * (1 + az) + 0.25 * dz
    e_x = e_h.mean(1) + (samples + 1) * U * LN2
    identity = np.where(e_m < 0.5, entropy64(np.minimum(e_m, 0.5)), LN2)      # H is increasing on [0, 1/2]
    if dz if identity_only is None else identity_only:
        transfer = identity
    else:
        lo, hi = ref.mean - e_m, ref.mean + e_m
        inside = (lo > 0) & (hi < 1)
        far = np.where(np.abs(lo - 0.5) > np.abs(hi - 0.5), lo, hi)
        with np.errstate(divide="ignore", invalid="ignore"):
            slope = np.abs(np.log(far / (1.0 - far)))
        transfer = np.where(inside, np.minimum(slope * e_m, identity), identity)
    e_H = transfer + 4 * U * (ref.entropy + transfer) + U
    e_i = e_H + e_x + U * LN2
    n = z.shape[-1]
    e_s = _scores(e_H, e_i, e_v) + n * 2.0 ** -52 * ref.scores
    return Stats(e_m, e_H, e_x, e_i, e_v, e_s)


def stats_from_logits(z32, samples):
    """fp32 logits [scenes * S, n] (numpy, scene-major) -> (Stats in fp64, Stats of the TIGHT bounds)."""
    z32 = np.asarray(z32)
    assert z32.dtype == F and z32.ndim == 2 and z32.shape[0] % samples == 0
    ref, z, p, h, d = _reference(z32, samples)
    return ref, _bounds(ref, z, p, h, d, samples)


def stats64(x, w, bias, samples):
    """x [scenes * S, k], w [n, k], bias [n] or None (numpy) -> (Stats in fp64 from the operands, Stats of the LOOSE bounds)."""
    z = np.asarray(x, dtype=D) @ np.asarray(w, dtype=D).T
    if bias is not None:
        z = z + np.asarray(bias, dtype=D)
    ref, zz, p, h, d = _reference(z, samples)
    return ref, _bounds(ref, zz, p, h, d, samples, dz=KERNEL_BOUND * float(np.abs(z).max()))


def stats_of_logits64(z, samples, dz):
    """fp64 logits [scenes * S, n] of a reference whose logits the product may miss by ``dz`` (a model against its fp64 oracle:
    MODEL_BOUND of the peak) -> (Stats, Stats of bounds): the loose bounds at that ``dz``, the entropy's transfer the smaller of the
    end-point slope and the identity, both of which hold."""
    ref, zz, p, h, d = _reference(z, samples)
    return ref, _bounds(ref, zz, p, h, d, samples, dz=dz, identity_only=False)


# ---- the fp32 model -----------------------------------------------------------------------------------------------------------
def _ln32(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(x.astype(D)).astype(F)      # logf, correctly rounded


def _term32(f):
    with np.errstate(invalid="ignore"):
        return np.where(f == 0, F(0), -(f * _ln32(np.where(f == 0, F(1), f))).astype(F)).astype(F)


def model32(z32, samples):
    """The header's formulas in numpy float32, operation for operation -> Stats (fp32 maps, fp64 scores)."""
    z32 = np.asarray(z32, dtype=F)
    n = z32.shape[1]
    z = z32.reshape(-1, samples, n)
    inv = F(1.0 / samples)
    with np.errstate(all="ignore"):
        p, _ = er.model_sigmoid_softplus(z)
        az = np.abs(z)
        q, l1p = er.model_sigmoid_softplus(-az)
        h = (l1p + (az * q).astype(F)).astype(F)
        total, htotal = p[:, 0].copy(), h[:, 0].copy()
        for s in range(1, samples):
            total = (total + p[:, s]).astype(F)
            htotal = (htotal + h[:, s]).astype(F)
        mean, expected = (total * inv).astype(F), (htotal * inv).astype(F)
        d = (p[:, 0] - mean).astype(F)
        sq = (d * d).astype(F)
        for s in range(1, samples):
            d = (p[:, s] - mean).astype(F)
            sq = (sq + (d * d).astype(F)).astype(F)
        var = (sq * inv).astype(F)
        om = (F(1) - mean).astype(F)
        entropy = (_term32(mean) - np.where(om == 0, F(0), (om * _ln32(np.where(om == 0, F(1), om))).astype(F))).astype(F)
        gap = (entropy - expected).astype(F)
        mi = (F(0) * entropy).astype(F) if samples == 1 else np.where(gap < 0, F(0), gap).astype(F)
    return Stats(mean, entropy, expected, mi, var, _scores(entropy.astype(D), mi.astype(D), var.astype(D)))


def fraction(got, ref, bound):
    """max |got - ref| / bound: the largest fraction of the bound an output uses (NaN where the output is NaN)."""
    return float(np.max(er.error_fraction(np.abs(np.asarray(got, dtype=D) - ref), bound)))
