"""Reference and inputs for the bootstrapped road-map loss (csrc/topk_loss.hip): plain torch on the CPU, following the definition in
include/dd_topk_loss.h.

``z`` [B,P] fp32 logits, ``t`` [B,P] 0/1.  The margins are taken in fp32 -- a sign flip, ``-0 -> +0`` -- so the selection is made on the
bits the kernel sees: ``tau = torch.topk(u, K).values[..., -1]``, the mask ``u >= tau`` (ties kept).  Loss, ``L_all``, the per-sample sums
and the gradient then come in fp64, by autograd through ``softplus``.

THE BOUNDS are the project's kernel bounds, stated before any kernel ran: ``n_b``, ``tau_b`` and the set of non-zero gradient positions
exact; the loss, ``L_all`` and the per-sample sums within 2e-5 of themselves; a gradient within 2e-5 of its tensor's peak."""
import os
import re

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "dd_topk_loss.h")) as _f:
    _text = _f.read()
CHUNK = int(re.search(r"^#define DD_TOPK_CHUNK (\d+)", _text, re.M).group(1))
BINS = int(re.search(r"^#define DD_TOPK_BINS (\d+)", _text, re.M).group(1))
PIECE_BYTES = int(re.search(r"^#define DD_TOPK_PIECE_BYTES (\d+)", _text, re.M).group(1))
STATE_BYTES = int(re.search(r"^#define DD_TOPK_STATE_BYTES (\d+)", _text, re.M).group(1))
DIGIT_BITS = (11, 11, 10)         # the digit plan of csrc/topk_loss.hip, from the top of the key
GRAD_OF_PEAK = 2e-5               # a gradient against its tensor's peak
LOSS_REL = 2e-5                   # the loss, L_all and a sample's sums, against themselves
MODEL_GRAD_OF_PEAK = 2e-4         # a parameter gradient of a model against that tensor's peak
EDGE_LOGITS = (0.0, 1e-3, 1.0, 17.0, 40.0, 88.0, 104.0)      # both signs of each: past 1 - p == 1 (17), the flush of exp (88), exp2's range (104)


def header_workspace_bytes(batch, per):
    """The header's formula, spelled here a second time."""
    return batch * (PIECE_BYTES * ((per + CHUNK - 1) // CHUNK) + 4 * BINS + STATE_BYTES)


def margins(z, t):
    """fp32 [B,P]: ``-z`` where the label is set, else ``z``; a ``-0`` margin is ``+0``."""
    z = z.detach().cpu().float()
    t = t.detach().cpu().to(torch.bool)
    u = torch.where(t, -z, z)
    return torch.where(u == 0, torch.zeros_like(u), u)


def selection(z, t, keep):
    """-> (tau fp32 [B], mask bool [B,P], n int64 [B]) on the fp32 margins: exact."""
    u = margins(z, t)
    tau = torch.topk(u, int(keep), dim=1).values[:, -1]
    mask = u >= tau[:, None]
    return tau, mask, mask.sum(1)


def loss_and_grad(z, t, keep, grad_scale=1.0):
    """-> (L, L_all, stats fp64 [B,4] = {n_b, sum_{S_b} sp, tau_b, sum_all sp}, dL/dz * grad_scale fp64 [B,P], mask), on the CPU, from
    fp32 logits taken exactly."""
    z32 = z.detach().cpu().float()
    tb = t.detach().cpu().to(torch.bool)
    tau, mask, n = selection(z32, tb, keep)
    zd = z32.double().requires_grad_(True)
    sp = F.softplus(torch.where(tb, -zd, zd))      # per-pixel BCE-with-logits: softplus of the margin
    sel = (sp * mask).sum(1)
    loss = (sel / n.double()).mean()
    (dz,) = torch.autograd.grad(loss * grad_scale, zd)
    total = sp.detach().sum(1)
    stats = torch.stack([n.double(), sel.detach(), tau.double(), total], dim=1)
    return loss.detach(), total.sum() / z32.numel(), stats, dz, mask


def logits_and_target(shape, salt=0, scale=2.0):
    """(z fp32 ~ N(0, scale^2), t uint8 with about a third set) on the CPU, seeded."""
    g = torch.Generator().manual_seed(1000 + salt)
    z = torch.randn(shape, generator=g) * scale
    t = (torch.rand(shape, generator=g) < 1.0 / 3.0).to(torch.uint8)
    return z, t


def floats_of_keys(keys):
    """int64 keys in [0, 2^32) -> the fp32 values whose order-preserving image they are (the inverse of the header's key map)."""
    k = np.asarray(keys, dtype=np.uint64).astype(np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k)
    return torch.from_numpy(bits.astype(np.uint32).view(np.float32).copy())


def key_of_float(x):
    bits = int(np.float32(x).view(np.uint32))
    return (~bits & 0xffffffff) if bits & 0x80000000 else bits | 0x80000000


def peak_error(got, want):
    """max |got - want| / max |want| (fp64, on the CPU); a reference that is identically zero must be met exactly."""
    got, want = got.detach().double().cpu(), want.double().cpu()
    err, peak = float((got - want).abs().max()), float(want.abs().max())
    if peak == 0.0:
        assert err == 0.0, "a zero gradient must be exact"
        return 0.0
    return err / peak
