"""The mirror consistency loss: train the road-map head on UNLABELLED scenes by pulling the map predicted from a scene and the map
predicted from its left/right mirror together.

The data set has four times as many unlabelled scenes as labelled ones, and the dense blocks' dropout is always on: two passes over one
scene are two stochastic views of it, the setting of the Pi-model (Laine & Aila, "Temporal Ensembling for Semi-Supervised Learning",
2017).  Here the second view is also the mirrored scene (``augment.augment_views``), whose map is the scene's map with its rows reversed
(``tta.py``'s convention), so the loss carries the reversal inside it.  Two parts.  The BINDER of
``csrc/libdd_consistency.so`` (``include/dd_consistency.h``), a ``_lib.Extension`` of its entry in ``build.TRAINING_EXTENSIONS``.  And what
``RoadMapBCE.training_step`` takes when ``hparams.cons_weight`` > 0: ``mirror_consistency``, ``ramp``, ``check_hparams``; with the weight 0
or absent the model never imports this module.

THE SEMANTICS are the header's.  ``a`` [B,h,w] the logits of the scenes, ``m`` [B,h,w] those of the mirrored scenes, ``m'[b,r,c] =
m[b,h-1-r,c]``, ``P`` the dense head's one sigmoid: ``L = mean (P(a) - P(m'))^2``; per pair ``Q_b = sum (P(a) - P(m'))^2`` and ``D_b`` the number
of elements where ``a > 0`` and ``m' > 0`` disagree, exact.  The gradient goes through ``p (1 - p)`` only: finite for every finite logit.

One GPU, fp32 logits.  The loss is a per-rank quantity: under data-parallel training every rank takes the mean over its own pairs and
``ddp.GradSync`` averages the gradients, as for every other loss of the package; it has not been run on more than one GPU.
"""
import math

import torch

from . import _lib, ops
from . import build as _build
from ._lib import HotpathError
from .lightning import hparam

# ---- the binder ------------------------------------------------------------------------------------------------------------------
_EXT = _lib.Extension(_build.TRAINING_EXTENSIONS["consistency"])
LIB, SIGNATURES, STREAMED, OPERANDS = _EXT.library, _EXT.signatures, _EXT.streamed, _EXT.operands
lib, launch, last_error = _EXT.lib, _EXT.launch, _EXT.last_error      # module-level names: the functions below reach ``launch`` through the module's globals at call time
CHUNK = _EXT.constant("DD_CONS_CHUNK")                     # elements per piece: a workgroup's share of one pair


def workspace_bytes(batch, per):
    """The bytes of fp64 partials a call on ``batch`` pairs of ``per`` elements needs: two per piece (the header: there is no size query)."""
    return 2 * 8 * int(batch) * (-(-int(per) // CHUNK))


# ---- the two launch functions as functions of tensors ------------------------------------------------------------------------------
def _operands(who, a, m):
    if not isinstance(a, torch.Tensor) or a.dim() != 3 or a.numel() == 0:
        raise HotpathError(f"{who}: expected fp32 [B,h,w] with no empty dimension, got {tuple(getattr(a, 'shape', ()))}")
    _lib.dev(a, f"{who}: a")
    _lib.dev(m, f"{who}: m", tuple(a.shape))
    return tuple(a.shape)


def _results(a, b, per):
    nbytes = workspace_bytes(b, per)
    return (torch.empty(1, device=a.device, dtype=torch.float32), torch.empty((b, 2), device=a.device, dtype=torch.float64),
            torch.empty(nbytes, device=a.device, dtype=torch.uint8), nbytes)


def fwd(a, m):
    """dd_cons_fwd outside autograd -> (loss fp32 [1], stats fp64 [B,2] = {Q_b, D_b})."""
    b, h, w = _operands("consistency.fwd", a, m)
    loss, stats, ws, nbytes = _results(a, b, h * w)
    launch("dd_cons_fwd", a.detach(), m.detach(), b, h, w, loss, stats, ws, nbytes)
    return loss, stats


def fwd_grad(a, m, grad_scale=1.0, out=None):
    """dd_cons_fwd_grad outside autograd -> (loss, stats, da, dm): the same pass, also writing ``dL/da * grad_scale`` and ``dL/dm *
    grad_scale``.  ``out``: (da, dm) to write into instead of two new tensors."""
    b, h, w = _operands("consistency.fwd_grad", a, m)
    da, dm = (torch.empty_like(a), torch.empty_like(m)) if out is None else out
    _lib.dev(da, "consistency.fwd_grad: da", (b, h, w))
    _lib.dev(dm, "consistency.fwd_grad: dm", (b, h, w))
    loss, stats, ws, nbytes = _results(a, b, h * w)
    launch("dd_cons_fwd_grad", a.detach(), m.detach(), b, h, w, float(grad_scale), da, dm, loss, stats, ws, nbytes)
    return loss, stats, da, dm


# ---- autograd --------------------------------------------------------------------------------------------------------------------
def _halves(z):
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.numel() == 0 or z.shape[0] % 2:
        raise HotpathError("mirror_consistency: expected logits [2B,h,w] with no empty dimension -- B scenes, then their B mirrors -- got "
                           f"{tuple(getattr(z, 'shape', ()))}")
    _lib.dev(z, "mirror_consistency: logits")
    b = z.shape[0] // 2
    return z[:b], z[b:]


class MirrorConsistency(torch.autograd.Function):
    """ONE logits tensor ``z`` [2B,h,w] -- rows [:B] from the scenes, rows [B:] from their mirrors -- -> (loss, stats); ``stats`` carries no
    gradient.  The gradient is written with the forward into one ``dz`` [2B,h,w], as the package's other losses do."""

    @staticmethod
    def forward(ctx, z):
        a, m = _halves(z)
        if ctx.needs_input_grad[0]:
            dz = torch.empty_like(z)
            loss, stats, _, _ = fwd_grad(a, m, 1.0, out=(dz[:a.shape[0]], dz[a.shape[0]:]))
        else:
            dz, (loss, stats) = None, fwd(a, m)
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return loss.reshape(()), stats

    @staticmethod
    def backward(ctx, g, _gs):
        (dz,) = ctx.saved_tensors
        if g is None or dz is None:
            return None
        return ops._scaled_loss_grad(ctx, dz, g)


def mirror_consistency(z, return_stats=False):
    """The mirror consistency loss of the road-map head's logits ``z`` [2B,h,w] (fp32, contiguous): rows [:B] predicted from B scenes, rows
    [B:] from their left/right mirrors -> the 0-dim loss ``mean (P(z[b]) - P(z[B + b]) rows reversed)^2``, differentiable in ``z``.
    ``return_stats=True``: ``(loss, stats)``, ``stats`` fp64 [B,2] = {Q_b, D_b} without a gradient."""
    loss, stats = MirrorConsistency.apply(z)
    return (loss, stats) if return_stats else loss


# ---- the weight ------------------------------------------------------------------------------------------------------------------
def ramp(step, rampup_steps):
    """The Pi-model's sigmoid-shaped ramp-up of the loss's weight: 1 when ``rampup_steps`` <= 0, else ``exp(-5 (1 - min(step /
    rampup_steps, 1))^2)``: exp(-5) at step 0, 1 from ``rampup_steps`` on."""
    if rampup_steps <= 0:
        return 1.0
    x = 1.0 - min(float(step) / float(rampup_steps), 1.0)
    return math.exp(-5.0 * x * x)


def check_hparams(hparams):
    """``(cons_weight, cons_rampup_steps)`` of ``hparams`` (absent: 0, 0).  A negative or non-finite weight or a negative ramp raises
    ValueError."""
    weight, steps = hparam(hparams, "cons_weight", 0.0), hparam(hparams, "cons_rampup_steps", 0)
    try:
        weight = float(0.0 if weight is None else weight)
    except (TypeError, ValueError):
        raise ValueError(f"cons_weight must be a number, got {weight!r}") from None
    if not 0.0 <= weight < float("inf"):
        raise ValueError(f"cons_weight must be a finite number >= 0, got {weight!r}")
    try:
        steps = int(0 if steps is None else steps)
    except (TypeError, ValueError):
        raise ValueError(f"cons_rampup_steps must be an integer, got {steps!r}") from None
    if steps < 0:
        raise ValueError(f"cons_rampup_steps must be >= 0, got {steps}")
    return weight, steps


def add_consistency_args(p):
    """``--cons_weight`` / ``--cons_rampup_steps``, for the parser of a script that trains ``RoadMapBCE`` on batches with an unlabelled part."""
    p.add_argument("--cons_weight", type=float, default=0.0,
                   help="weight of the mirror consistency loss on the unlabelled scenes of a (sample, target, road_image, unlabelled) batch: "
                        "the map of a scene and of its mirror pulled together; 0 = off")
    p.add_argument("--cons_rampup_steps", type=int, default=0,
                   help="steps over which the consistency weight rises from exp(-5) of itself to itself (exp(-5 (1 - t / T)^2)); 0 = no ramp")
    return p
