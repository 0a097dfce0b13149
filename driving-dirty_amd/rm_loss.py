"""The road-map loss on the head's logits: weighted BCE-with-logits plus the soft threat score, the metric the head is scored in.

The logit-domain counterpart of ``ops.box_loss``.  The box loss works on probabilities: it clamps the logs at -100
and divides by ``p`` and ``1 - p``, and a confident road-map head has logits past |z| = 17, where ``1 - p`` is 0 in fp32.  Here the
loss is ``softplus(+-z)`` and the gradient goes through ``p (1 - p)``: finite for every finite logit.  Two parts.  The BINDER of
``csrc/libdd_rm_loss.so`` (``include/dd_rm_loss.h``), a ``_lib.Extension`` of its entry in ``build.EXTENSIONS``.  And ``road_map_loss``, which ``RoadMapBCE`` and ``JointRoadMapBBox`` take when an
``rm_*`` hparam is set (``roadmap.rm_loss_config`` parses them, ``roadmap.add_rm_loss_args`` are the flags); with all of them at their
defaults neither imports this module.

THE SEMANTICS are the header's.  Per sample, ``T = sum t``, ``S = sum p``, ``I = sum p t``, ``U = S + T - I``;
``L_bce = F.binary_cross_entropy_with_logits(z, t, pos_weight=w)`` with ``w`` None (1), a positive number or "auto" = the sample's own
negatives / positives, a constant of the step; ``L_ts = mean_b 1 - (I + eps) / (U + eps)``; ``L = bce_weight L_bce + ts_weight L_ts``.

One GPU, fp32 logits.  The loss is a per-rank quantity: under data-parallel training every rank takes the mean over its own samples
and ``ddp.GradSync`` averages the gradients, as for every other loss of the package.
"""
import ctypes as C

import torch

from . import _lib, ops
from . import build as _build
from ._lib import HotpathError

# ---- the binder ------------------------------------------------------------------------------------------------------------------
_EXT = _lib.Extension(_build.EXTENSIONS["rm_loss"])
LIB, SIGNATURES, STREAMED, OPERANDS = _EXT.library, _EXT.signatures, _EXT.streamed, _EXT.operands
lib, launch, last_error = _EXT.lib, _EXT.launch, _EXT.last_error      # module-level names: the functions below reach ``launch`` through the module's globals at call time
CHUNK = _EXT.constant("DD_RM_LOSS_CHUNK")                  # elements per piece: a workgroup's share of one sample
TABLE_MAX = _EXT.constant("DD_RM_LOSS_TABLE_MAX")          # per-sample masks of a pointer table; a longer tuple is stacked
POS_WEIGHT_AUTO = _EXT.constant("DD_RM_POS_WEIGHT_AUTO", float)
TARGET_F32, TARGET_U8 = 0, 1                               # dd_hotpath.h: DD_TARGET_F32 / DD_TARGET_U8
ACC_TERMS = CHUNK // 256                                   # elements a thread adds in fp32 before it goes to fp64


def workspace_bytes(batch, per_sample):
    """The bytes of fp64 partials a forward call needs: five per piece (the header: there is no size query)."""
    return 5 * 8 * int(batch) * (-(-int(per_sample) // CHUNK))


# ---- operands --------------------------------------------------------------------------------------------------------------------
def _pos_weight(pos_weight):
    if pos_weight is None:
        return 1.0
    if isinstance(pos_weight, str):
        if pos_weight != "auto":
            raise HotpathError(f"road_map_loss: pos_weight must be None, a positive number or 'auto', got {pos_weight!r}")
        return POS_WEIGHT_AUTO
    if float(pos_weight) == POS_WEIGHT_AUTO:
        raise HotpathError("road_map_loss: pos_weight must be positive (the per-sample weight is asked for as 'auto')")
    return float(pos_weight)


def _operands(values, target, what="logits"):
    """Host-side check of the [B, P] fp32 ``values`` (logits or probabilities) and the target -> (target as the kernels read it,
    its entry point's suffix, the operands that describe it).  A tuple of at most TABLE_MAX masks goes as a HOST pointer table; a
    longer one is stacked and takes the byte kernel, the same arithmetic in the same order: the same bits."""
    if not isinstance(values, torch.Tensor) or values.dim() != 2:
        raise HotpathError(f"road_map_loss: {what} must be [B, P], got {tuple(getattr(values, 'shape', ()))}")
    if values.dtype != torch.float32:
        raise HotpathError(f"road_map_loss: {what} must be fp32, got {values.dtype}")
    _lib.dev(values, what)
    b, per = values.shape
    if isinstance(target, (tuple, list)):
        if len(target) != b:
            raise HotpathError(f"road_map_loss: {len(target)} masks for {b} samples")
        for t in target:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype in (torch.bool, torch.uint8) and t.numel() == per):
                raise HotpathError(f"road_map_loss: per-sample masks must be contiguous bool / uint8 device tensors of {per} elements")
        if b <= TABLE_MAX:
            return target, "_u8_ptrs", ((C.c_void_p * b)(*[t.data_ptr() for t in target]),)
        target = torch.stack(tuple(t.reshape(-1) for t in target), dim=0)
    if not (isinstance(target, torch.Tensor) and target.is_cuda and target.is_contiguous() and tuple(target.shape) == (b, per)
            and target.dtype in (torch.float32, torch.uint8, torch.bool)):
        raise HotpathError(f"road_map_loss: target must be a contiguous fp32 / uint8 / bool device tensor of shape {(b, per)} or a tuple of "
                           f"per-sample masks, got {getattr(target, 'dtype', type(target))} {tuple(getattr(target, 'shape', ()))}")
    return target, "", (target, TARGET_F32 if target.dtype == torch.float32 else TARGET_U8)


def fwd(logits, target, pos_weight=None, bce_weight=1.0, ts_weight=0.0, ts_eps=1.0, want_probs=True):
    """dd_rm_loss_fwd / dd_rm_loss_fwd_u8_ptrs outside autograd -> (losses fp32 [3] = {L, L_bce, L_ts}, stats fp64 [B, 5] = {T, S, I, A,
    C} per sample, coef fp32 [B, 4]: the gradient coefficients ``bwd`` takes, probs fp32 [B, P] or None).  One pass over the data for
    any weight; validation stops here."""
    pw = _pos_weight(pos_weight)
    target, suffix, described = _operands(logits, target)
    b, per = logits.shape
    dev = logits.device
    losses = torch.empty(3, device=dev, dtype=torch.float32)
    stats = torch.empty((b, 5), device=dev, dtype=torch.float64)
    coef = torch.empty((b, 4), device=dev, dtype=torch.float32)
    probs = torch.empty_like(logits) if want_probs else None
    nbytes = workspace_bytes(b, per)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    launch("dd_rm_loss_fwd" + suffix, logits, *described, b, per, pw, float(bce_weight), float(ts_weight), float(ts_eps), probs, losses, stats,
           coef, ws, nbytes)
    return losses, stats, coef, probs


def bwd(probs, target, coef, grad_scale=1.0):
    """dd_rm_loss_bwd / dd_rm_loss_bwd_u8_ptrs: d(loss)/d(logits) * grad_scale from the probabilities and the coefficients of ``fwd`` on
    the same target."""
    target, suffix, described = _operands(probs, target, "probs")
    b, per = probs.shape
    _lib.dev(coef, "coef", (b, 4))
    dlogits = torch.empty_like(probs)
    launch("dd_rm_loss_bwd" + suffix, probs, *described, b, per, coef, float(grad_scale), dlogits)
    return dlogits


# ---- autograd --------------------------------------------------------------------------------------------------------------------
class RoadMapLoss(torch.autograd.Function):
    """Weighted BCE-with-logits + soft threat score -> (loss, probs, L_bce, L_ts, stats); everything but the loss carries no gradient.
    The gradient is written with the forward (from the probabilities it has just stored), as the package's other losses do."""

    @staticmethod
    def forward(ctx, logits, target, pos_weight, bce_weight, ts_weight, ts_eps):
        losses, stats, coef, probs = fwd(logits, target, pos_weight, bce_weight, ts_weight, ts_eps)
        ctx.save_for_backward(bwd(probs, target, coef) if ctx.needs_input_grad[0] else None)
        loss, bce, ts = losses.unbind(0)
        ctx.mark_non_differentiable(probs, bce, ts, stats)
        ctx.set_materialize_grads(False)      # no 82 MB of zeros for the probabilities' (unused) gradient slot
        return loss, probs, bce, ts, stats

    @staticmethod
    def backward(ctx, g, _gp, _gb, _gt, _gs):
        (dz,) = ctx.saved_tensors
        if g is None or dz is None:
            return (None,) * 6
        return (ops._scaled_loss_grad(ctx, dz, g),) + (None,) * 5


def road_map_loss(logits, target, pos_weight=None, bce_weight=1.0, ts_weight=0.0, ts_eps=1.0, return_parts=False):
    """``bce_weight * L_bce + ts_weight * L_ts`` of the road-map head's ``logits`` [B, P] (fp32) against ``target``: a [B, P] tensor (fp32
    in [0, 1], uint8 or bool) or the collate's tuple of per-sample bool / uint8 masks -> ``(loss, probs)``: the 0-dim loss,
    differentiable in ``logits``, and sigmoid(logits) -- the bits of ``ops.sigmoid`` -- without a gradient.
      * L_bce: ``F.binary_cross_entropy_with_logits`` with the positive elements weighted by ``pos_weight``: None (1), a positive number,
        or "auto" = each sample's own (P - T_b) / max(T_b, 1), a constant of the step;
      * L_ts: mean over the samples of 1 - (I_b + ts_eps) / (U_b + ts_eps), the soft threat score.
    ``return_parts=True``: ``(loss, probs, L_bce, L_ts, stats)``, the components detached 0-dim tensors for logging and ``stats`` fp64
    [B, 5] = {T, S, I, A, C}."""
    loss, probs, bce, ts, stats = RoadMapLoss.apply(logits, target, pos_weight, bce_weight, ts_weight, ts_eps)
    return (loss, probs, bce, ts, stats) if return_parts else (loss, probs)

