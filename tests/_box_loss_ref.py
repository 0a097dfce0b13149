"""fp64 reference for the class-balanced box-map loss (csrc/box_loss.hip): plain torch, following the definition in include/dd_hotpath.h.

Per sample b over its P elements: T = sum t, S = sum p, I = sum p t, U = S + T - I,
  L_bce = 1 / (B P) sum_b sum_i -[w_b t max(log p, -100) + (1 - t) max(log(1 - p), -100)],  w_b = pos_weight or (P - T_b) / max(T_b, 1),
  L_ts  = 1 / B sum_b [1 - (I_b + eps) / (U_b + eps)],  L = alpha L_bce + beta L_ts.
The gradient comes from autograd with w_b detached, and is set to zero explicitly for the clamped term at p = 0 / p = 1 (the convention of
bce_probs_kernel); ``closed_form_grad`` is the formula of the header, for the test that holds the two together.  Also the seeded inputs the
tests draw from.  Nothing here imports the package under test beyond ``synth``'s closed-form generators.
"""
import torch

AUTO = "auto"


def weights(t, pos_weight):
    """w_b as fp64 [B, 1]: a constant of the step."""
    b, per = t.shape
    if pos_weight is None:
        pos_weight = 1.0
    if pos_weight == AUTO:
        tb = t.sum(dim=1, keepdim=True)
        return ((per - tb) / tb.clamp(min=1.0)).detach()
    return torch.full((b, 1), float(pos_weight), dtype=torch.float64)


def stats(p, t):
    """fp64 [B, 5] = {T, S, I, A, C}."""
    p, t = p.double(), t.double()
    lp, lq = clamped_logs(p)
    nlp, nlq = -lp, -lq
    return torch.stack([t.sum(1), p.sum(1), (p * t).sum(1), (t * nlp).sum(1), ((1 - t) * nlq).sum(1)], dim=1)


def clamped_logs(p):
    """(max(log p, -100), max(log(1 - p), -100)).  Where a clamp is active (p = 0 for the first, p = 1 for the second) the value is the
    constant -100, written as one: its slope is zero by the convention, where autograd through log would give inf or nan."""
    pd, half, floor = p.detach(), torch.full_like(p, 0.5), torch.full_like(p, -100.0)
    lp = torch.where(pd > 0, torch.log(torch.where(pd > 0, p, half)), floor).clamp(min=-100.0)
    lq = torch.where(pd < 1, torch.log1p(-torch.where(pd < 1, p, half)), floor).clamp(min=-100.0)
    return lp, lq


def terms(p, t, pos_weight=None, eps=1.0):
    """(L_bce, L_ts) as fp64 0-dim tensors, differentiable in p (fp64 [B, P]; t fp64)."""
    b, per = p.shape
    w = weights(t, pos_weight)
    lp, lq = clamped_logs(p)
    l_bce = -(w * t * lp + (1 - t) * lq).sum() / (b * per)
    tb, sb, ib = t.sum(1), p.sum(1), (p * t).sum(1)
    l_ts = (1 - (ib + eps) / (sb + tb - ib + eps)).sum() / b
    return l_bce, l_ts


def loss_and_grad(p, t, pos_weight=None, alpha=1.0, beta=0.0, eps=1.0):
    """-> (L, L_bce, L_ts, dL/dp), all fp64 on the CPU, from fp32 / uint8 / bool inputs taken exactly; the gradient by autograd."""
    p = p.detach().double().cpu().requires_grad_(True)
    t = t.detach().double().cpu()
    l_bce, l_ts = terms(p, t, pos_weight, eps)
    total = alpha * l_bce + beta * l_ts
    (g,) = torch.autograd.grad(total, p)
    return total.detach(), l_bce.detach(), l_ts.detach(), g


def closed_form_grad(p, t, pos_weight=None, alpha=1.0, beta=0.0, eps=1.0):
    """The header's formula, fp64: alpha / (B P) [-w t / p + (1 - t) / (1 - p)] - beta / B [t (U + eps) - (I + eps)(1 - t)] / (U + eps)^2,
    the first bracket's terms 0 where p = 0 / p = 1."""
    p, t = p.detach().double().cpu(), t.detach().double().cpu()
    b, per = p.shape
    w = weights(t, pos_weight)
    gp = torch.where(p > 0, 1 / torch.where(p > 0, p, torch.ones_like(p)), torch.zeros_like(p))
    gq = torch.where(p < 1, 1 / torch.where(p < 1, 1 - p, torch.ones_like(p)), torch.zeros_like(p))
    tb, sb, ib = t.sum(1, keepdim=True), p.sum(1, keepdim=True), (p * t).sum(1, keepdim=True)
    den, num = sb + tb - ib + eps, ib + eps
    return alpha / (b * per) * (-w * t * gp + (1 - t) * gq) - beta / b * (t * den - num * (1 - t)) / den ** 2


def inputs(b, per, salt=0, density=0.03, empty=(), full=()):
    """(p fp32 [b, per] uniform in [0.02, 0.98], t fp32 0 / 1 Bernoulli(density)); the samples in ``empty`` get t = 0, in ``full`` t = 1."""
    from driving_dirty_amd import synth
    p = synth.hash_uniform((b, per), synth.key_salt("box_loss_p", salt), 0.02, 0.98)
    t = (synth.hash_uniform((b, per), synth.key_salt("box_loss_t", salt), 0.0, 1.0) < density).float()
    for i in empty:
        t[i] = 0.0
    for i in full:
        t[i] = 1.0
    return p, t
