"""fp64 reference and seeded inputs for the mirror consistency loss (csrc/consistency.hip): plain torch, following the definition in
include/dd_consistency.h.

``a`` [B,h,w] the logits of the scenes, ``m`` [B,h,w] those of the mirrored scenes, ``m' = flip(m, rows)``, N = B h w:
  L = sum (sigmoid(a) - sigmoid(m'))^2 / N,   Q_b the same sum per pair,   D_b = #{(a > 0) != (m' > 0)} on the fp32 logits.
The gradients come from autograd.

THE BOUNDS are the project's kernel bounds, stated before any kernel ran: a gradient within 2e-5 of its tensor's peak, the loss (and a
pair's Q_b) within 2e-5 of itself, D_b exact."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "dd_consistency.h")) as _f:
    CHUNK = int(re.search(r"^#define DD_CONS_CHUNK (\d+)", _f.read(), re.M).group(1))
GRAD_OF_PEAK = 2e-5               # a gradient against its tensor's peak
LOSS_REL = 2e-5                   # the loss, and a pair's sum, against itself
MODEL_GRAD_OF_PEAK = 2e-4         # a parameter gradient of a model against that tensor's peak

# (B, h, w): the smallest shapes at which the kernels can still go wrong
SHAPES = [(1, 1, 4),                        # one vector
          (2, 3, 8),                        # odd h: the middle row pairs with itself
          (3, 5, 6), (1, 7, 5),             # w % 4 != 0: the 4-byte path
          (2, 4, 1028),                     # a row longer than one sweep of a workgroup
          (2, 1, CHUNK + 4),                # a piece boundary inside a row
          (2, 2, CHUNK // 2 + 4),           # ... and across rows
          (33, 2, 8),                       # more pairs than the finishing launch has waves
          (2, 800, 800)]                    # the road map
EDGE_LOGITS = (0.0, 1e-3, 1.0, 17.0, 40.0, 88.0, 104.0)      # both signs of each: past 1 - p == 1 (17), the flush of exp (88), exp2's range (104)


def disagreement(a, m):
    """fp64 [B]: the elements where the fp32 logits fall on different sides of 0, the mirrored map's rows reversed."""
    return ((a > 0) != (torch.flip(m, dims=(1,)) > 0)).reshape(a.shape[0], -1).sum(1).double()


def loss_and_grad(a, m, grad_scale=1.0):
    """-> (L, stats [B,2] = {Q_b, D_b}, dL/da * grad_scale, dL/dm * grad_scale), all fp64 on the CPU, from fp32 inputs taken exactly."""
    a32, m32 = a.detach().cpu(), m.detach().cpu()
    ad, md = a32.double().requires_grad_(True), m32.double().requires_grad_(True)
    d = torch.sigmoid(ad) - torch.sigmoid(torch.flip(md, dims=(1,)))
    q = (d * d).reshape(ad.shape[0], -1).sum(1)
    loss = q.sum() / ad.numel()
    da, dm = torch.autograd.grad(loss * grad_scale, (ad, md))
    return loss.detach(), torch.stack([q.detach(), disagreement(a32, m32)], dim=1), da, dm


def inputs(shape, salt=0):
    """(a, m) fp32 on the CPU, uniform in [-8, 8]."""
    from driving_dirty_amd import synth
    return (synth.hash_uniform(shape, synth.key_salt("cons_a", salt), -8.0, 8.0),
            synth.hash_uniform(shape, synth.key_salt("cons_m", salt), -8.0, 8.0))


def edge_inputs(w=16):
    """(a, m) fp32 [1, 14, w]: every pair of +-EDGE_LOGITS meets once -- a[r, c] = V[r], and m such that its row-reversed map is V[c % 14]."""
    v = torch.tensor([s * x for x in EDGE_LOGITS for s in (1.0, -1.0)], dtype=torch.float32)
    n = v.numel()
    a = v.reshape(1, n, 1).expand(1, n, w).contiguous()
    m_rev = v[torch.arange(w) % n].reshape(1, 1, w).expand(1, n, w)
    return a, torch.flip(m_rev, dims=(1,)).contiguous()


def peak_error(got, want):
    """max |got - want| / max |want| (fp64, on the CPU); a reference that is identically zero must be met exactly."""
    got, want = got.detach().double().cpu(), want.double().cpu()
    err, peak = float((got - want).abs().max()), float(want.abs().max())
    if peak == 0.0:
        assert err == 0.0, "a zero gradient must be exact"
        return 0.0
    return err / peak
