"""fp64 reference, seeded inputs, an fp32 model and DERIVED error bounds for the road-map loss on logits (csrc/rm_loss.hip): plain torch
and numpy, following the definition in include/dd_rm_loss.h.

Per sample b over its P elements, with p = sigmoid(z): T = sum t, S = sum p, I = sum p t, U = S + T - I, A = sum t softplus(-z),
C = sum (1 - t) softplus(z),
  L_bce = 1 / (B P) sum_b (w_b A_b + C_b),  w_b = pos_weight or (P - T_b) / max(T_b, 1),
  L_ts  = 1 / B sum_b [1 - (I_b + eps) / (U_b + eps)],  L = alpha L_bce + beta L_ts.
The gradient comes from autograd with w_b detached; ``closed_form_grad`` is the formula of the header, for the test that holds the two
together.  alpha, beta, eps and a numeric pos_weight cross the ABI as fp32: the reference takes them rounded to fp32 (``abi``), which
is the function the kernels are asked to compute.

THE BOUNDS.  Nothing here was taken from a kernel's output.  A statistic is a sum of non-negative terms; the kernel's value differs
from the fp64 one by
  * the element function's error: ``_element_ref.sig_bound`` per probability, ``_element_ref.softplus_bound`` per log1p(exp(-|z|));
  * fp32 rounding on the way to fp64: a thread adds at most ACC = CHUNK / 256 terms in fp32, ACC - 1 adds, and the term itself is one
    more add (max(+-z, 0) + l1p; the products with a 0 / 1 target are exact): ACC roundings of at most 2^-24 of a partial sum, which is
    at most the sum: ACC 2^-24 of the sum;
  * fp64 adds after that: fewer than P of them on any path, P 2^-53 of the sum.
The losses follow by propagation: L_bce is linear in A and C; a sample's soft threat score is monotone in I and in S, so its bound is
its value at the corners of the box [I +- dI] x [S +- dS]; and each of the three is rounded to fp32 once.
"""
import os
import re

import numpy as np
import torch
from torch.nn import functional as F

import _element_ref as E

AUTO = "auto"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "dd_rm_loss.h")) as _f:
    CHUNK = int(re.search(r"^#define DD_RM_LOSS_CHUNK (\d+)", _f.read(), re.M).group(1))
THREADS = 256
ACC = CHUNK // THREADS            # terms a thread adds in fp32 before it goes to fp64
GRAD_OF_PEAK = 2e-5               # a gradient against that sample's peak |dL/dz|: the box-loss test's figure, the project's
MODEL_GRAD_OF_PEAK = 2e-4         # a parameter gradient of a model against that tensor's peak


def abi(x):
    """A scalar as the fp32 ABI argument it is handed over as."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ the fp64 reference
def weights(t, pos_weight):
    """w_b as fp64 [B, 1]: a constant of the step."""
    b, per = t.shape
    if pos_weight is None:
        pos_weight = 1.0
    if pos_weight == AUTO:
        tb = t.sum(dim=1, keepdim=True)
        return ((per - tb) / tb.clamp(min=1.0)).detach()
    return torch.full((b, 1), abi(pos_weight), dtype=torch.float64)


def softplus(z):
    """log(1 + exp(z)) in fp64, relative accuracy on both sides (|z| < 700)."""
    return F.softplus(z, beta=1.0, threshold=1000.0)


def stats(z, t):
    """fp64 [B, 5] = {T, S, I, A, C}."""
    z, t = z.detach().double().cpu(), t.detach().double().cpu()
    p = torch.sigmoid(z)
    return torch.stack([t.sum(1), p.sum(1), (p * t).sum(1), (t * softplus(-z)).sum(1), ((1 - t) * softplus(z)).sum(1)], dim=1)


def terms(z, t, pos_weight=None, eps=1.0):
    """(L_bce, L_ts) as fp64 0-dim tensors, differentiable in z (fp64 [B, P]; t fp64)."""
    b, per = z.shape
    w = weights(t, pos_weight)
    p = torch.sigmoid(z)
    l_bce = (w * t * softplus(-z) + (1 - t) * softplus(z)).sum() / (b * per)
    tb, sb, ib = t.sum(1), p.sum(1), (p * t).sum(1)
    l_ts = (1 - (ib + eps) / (sb + tb - ib + eps)).sum() / b
    return l_bce, l_ts


def loss_and_grad(z, t, pos_weight=None, alpha=1.0, beta=0.0, eps=1.0):
    """-> (L, L_bce, L_ts, dL/dz), all fp64 on the CPU, from fp32 / uint8 / bool inputs taken exactly; the gradient by autograd."""
    z = z.detach().double().cpu().requires_grad_(True)
    t = t.detach().double().cpu()
    alpha, beta, eps = abi(alpha), abi(beta), abi(eps)
    l_bce, l_ts = terms(z, t, pos_weight, eps)
    total = alpha * l_bce + beta * l_ts
    (g,) = torch.autograd.grad(total, z)
    return total.detach(), l_bce.detach(), l_ts.detach(), g


def closed_form_grad(z, t, pos_weight=None, alpha=1.0, beta=0.0, eps=1.0):
    """The header's formula, fp64: c1 (1 - t) p - c0 t (1 - p) + p (1 - p) [c3 (1 - t) - c2 t].  1 - p is taken as sigmoid(-z)."""
    z, t = z.detach().double().cpu(), t.detach().double().cpu()
    alpha, beta, eps = abi(alpha), abi(beta), abi(eps)
    b, per = z.shape
    w = weights(t, pos_weight)
    p, q = torch.sigmoid(z), torch.sigmoid(-z)
    tb, sb, ib = t.sum(1, keepdim=True), p.sum(1, keepdim=True), (p * t).sum(1, keepdim=True)
    den, num = sb + tb - ib + eps, ib + eps
    c0, c1, c2, c3 = alpha * w / (b * per), alpha / (b * per), beta / (b * den), beta * num / (b * den ** 2)
    return c1 * (1 - t) * p - c0 * t * q + p * q * (c3 * (1 - t) - c2 * t)


# ------------------------------------------------------------------------------------------------ inputs
def inputs(b, per, salt=0, density=0.35, empty=(), full=()):
    """(z fp32 [b, per] uniform in [-8, 8], t fp32 0 / 1 Bernoulli(density)); the samples in ``empty`` get t = 0, in ``full`` t = 1."""
    from driving_dirty_amd import synth
    z = synth.hash_uniform((b, per), synth.key_salt("rm_loss_z", salt), -8.0, 8.0)
    t = (synth.hash_uniform((b, per), synth.key_salt("rm_loss_t", salt), 0.0, 1.0) < density).float()
    for i in empty:
        t[i] = 0.0
    for i in full:
        t[i] = 1.0
    return z, t


def edge_inputs():
    """(z fp32 [2, n], t), n a multiple of 4: the edge logits of ``_element_ref.logit_edges()`` (the flush, 1 + e == 1 and one-ulp thresholds and their
    neighbours, both signs, +-0) and +-60 -- |z| reaches 87.4 -- once against each target value: sample 1 has the targets of sample 0
    inverted, so every logit meets t = 0 and t = 1."""
    edges = np.concatenate([E.logit_edges(), np.array([60.0, -60.0], dtype=np.float32)])
    pad = (-edges.size) % 4
    edges = np.concatenate([edges, np.zeros(pad, dtype=np.float32)])
    z = torch.from_numpy(np.stack([edges, edges]))
    t0 = (torch.arange(edges.size) % 2).float()
    return z, torch.stack([t0, 1 - t0])


SHAPES = [(1, 4), (3, CHUNK + 4), (65, 260), (2, 640000)]


def case(shape):
    """(z, t fp32 0 / 1) on the CPU for one of SHAPES."""
    b, per = shape
    if shape == (3, CHUNK + 4):       # a ragged last piece; sample 1 has an empty target, sample 2 is all ones
        return inputs(b, per, salt=1, empty=(1,), full=(2,))
    if shape == (2, 640000):          # the product shape: the road masks the models train on
        from driving_dirty_amd import synth
        z, _ = inputs(b, per, salt=4)
        return z, synth.road_maps(b, seed=31).reshape(b, per).float()
    return inputs(b, per, salt=b)


# ------------------------------------------------------------------------------------------------ the fp32 model of the kernels
def model_terms(z, t):
    """The five fp32 terms of every element as ``stat_quad`` forms them -> fp32 [5, B, P] (numpy), and the probabilities."""
    z = np.asarray(z, dtype=E.F)
    t = np.asarray(t, dtype=E.F)
    sig, l1p = E.model_sigmoid_softplus(z)
    sp_pos = (np.maximum(z, E.F(0)) + l1p).astype(E.F)
    sp_neg = (np.maximum(-z, E.F(0)) + l1p).astype(E.F)
    return np.stack([t, sig, (sig * t).astype(E.F), (t * sp_neg).astype(E.F), ((E.F(1) - t) * sp_pos).astype(E.F)]), sig


def model_stats(z, t):
    """fp64 [B, 5]: the statistics as the kernels add them up -- thread ``i`` of a piece owns the vectors i, i + 256, ... of it, ACC fp32
    adds in that order (a term past the sample's end is a +0), then fp64."""
    five, _ = model_terms(z, t)
    _, b, per = five.shape
    pps = -(-per // CHUNK)
    padded = np.zeros((5, b, pps * CHUNK), dtype=E.F)
    padded[:, :, :per] = five
    # [5, b, piece, vector u, thread, k] -> per thread the sequence (u, k)
    seq = padded.reshape(5, b, pps, ACC // 4, THREADS, 4).transpose(0, 1, 2, 4, 3, 5).reshape(5, b, pps * THREADS, ACC)
    acc = np.zeros(seq.shape[:-1], dtype=E.F)
    for j in range(ACC):
        acc = (acc + seq[..., j]).astype(E.F)
    return acc.astype(E.D).sum(axis=2).T.copy()


# ------------------------------------------------------------------------------------------------ the bounds
def stat_bounds(z, t):
    """fp64 numpy [B, 5]: |kernel - fp64| allowed for {T, S, I, A, C} (the module docstring derives it).  T's is 0: sums of at most ACC
    ones are exact in fp32 and integers below 2^53 in fp64."""
    z = np.asarray(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, dtype=E.D)
    t = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=E.D)
    per = z.shape[1]
    sig, sp = E.sigmoid64(z), E.softplus64(z)
    e_sig, e_sp = E.sig_bound(z, sig), E.softplus_bound(z, sp)
    sums = np.stack([t.sum(1), sig.sum(1), (sig * t).sum(1), (t * (np.maximum(-z, 0) + sp)).sum(1), ((1 - t) * (np.maximum(z, 0) + sp)).sum(1)], axis=1)
    elem = np.stack([np.zeros(z.shape[0]), e_sig.sum(1), (t * e_sig).sum(1), (t * e_sp).sum(1), ((1 - t) * e_sp).sum(1)], axis=1)
    out = elem + (ACC * E.U24 + per * 2.0 ** -53) * sums
    out[:, 0] = 0.0
    return out


def soft_ts(i, s, t, eps):
    return 1.0 - (i + eps) / (s + t - i + eps)


def loss_bounds(z, t, pos_weight, alpha, beta, eps, st=None, sb=None):
    """(bound of L, of L_bce, of L_ts) as floats: the statistics' bounds carried through the header's formulas, and one fp32 rounding
    of each result.  ``st`` / ``sb``: ``stats(z, t).numpy()`` and ``stat_bounds(z, t)`` where the caller has them already."""
    st = stats(z, t).numpy() if st is None else st
    sb = stat_bounds(z, t) if sb is None else sb
    b, per = z.shape
    alpha, beta, eps = abi(alpha), abi(beta), abi(eps)
    w = weights(t.detach().double().cpu(), pos_weight).numpy()[:, 0]
    T, S, I, A, C = st.T
    dS, dI, dA, dC = sb[:, 1], sb[:, 2], sb[:, 3], sb[:, 4]
    l_bce, e_bce = float((w * A + C).sum() / (b * per)), float((w * dA + dC).sum() / (b * per))
    f = soft_ts(I, S, T, eps)
    with np.errstate(all="ignore"):
        corners = np.stack([soft_ts(np.maximum(I + a * dI, 0.0), S + c * dS, T, eps) for a in (-1, 1) for c in (-1, 1)])
    e_f = np.abs(corners - f).max(axis=0)
    l_ts, e_ts = float(f.sum() / b), float(e_f.sum() / b)
    total = alpha * l_bce + beta * l_ts
    return (alpha * e_bce + beta * e_ts + E.U24 * abs(total), e_bce + E.U24 * abs(l_bce), e_ts + E.U24 * abs(l_ts))


def grad_excess(got, want):
    """max over the samples of |got - want| / that sample's peak |want| (fp64, on the CPU).  A sample whose gradient is identically zero
    (an empty target under the soft threat score alone with eps = 0: I = 0 and t = 0 everywhere) must come out as exact zeros."""
    got, want = got.detach().double().cpu(), want.double().cpu()
    err, peak = (got - want).abs().amax(dim=1), want.abs().amax(dim=1)
    assert bool((err[peak == 0] == 0).all()), "a zero gradient must be exact"
    return float((err / peak.clamp(min=1e-300)).max())
