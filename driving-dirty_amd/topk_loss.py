"""The bootstrapped road-map loss: BCE-with-logits averaged over each scene's K HARDEST pixels, K annealed down from "all".

Every other road-map loss of the package is a mean over a scene's 640 000 pixels, most of which are easy after the first epochs: the
thin band along the road edges, where the threat score is lost, gets a few percent of the gradient.  Bootstrapped cross-entropy (Wu et
al., "Bridging Category-level and Instance-level Semantic Image Segmentation", 2016) averages over the K pixels with the largest
loss instead.  That needs an exact per-sample selection -- the K-th largest of 640 000 -- inside a step without a host round trip:
``csrc/topk_loss.hip``.  Two parts.  The BINDER of ``csrc/libdd_topk_loss.so`` (``include/dd_topk_loss.h``), a
``_lib.Extension`` of its entry in ``build.BOOTSTRAP_EXTENSIONS``.  And what ``RoadMapBCE`` takes when ``hparams.rm_topk_frac`` < 1:
``TopKBce``, ``keep_now``, ``check_hparams``; with the fraction 1 or absent the model never imports this module.

THE SEMANTICS are the header's.  ``z`` [B,P] fp32 logits, ``t`` a 0/1 byte target; the margin ``u = -z if t else z`` (a sign flip; the
per-pixel loss ``softplus(u)`` is increasing in it); ``tau_b`` the K-th largest margin of sample b, ``S_b = {u >= tau_b}`` with ties
kept, ``n_b = |S_b| >= K``; ``L = mean_b mean_{S_b} softplus(u)``; the gradient ``(sigmoid(z) - t) / (B n_b)`` on ``S_b`` and exactly 0
elsewhere.  K = P is ``F.binary_cross_entropy_with_logits``.

One GPU, fp32 logits.  The loss is a per-rank quantity, as every other loss of the package.
"""
import ctypes as C
import math

import torch

from . import _lib, ops
from . import build as _build
from ._lib import HotpathError
from .lightning import hparam

# ---- the binder ------------------------------------------------------------------------------------------------------------------
_EXT = _lib.Extension(_build.BOOTSTRAP_EXTENSIONS["topk_loss"])
LIB, SIGNATURES, STREAMED, OPERANDS = _EXT.library, _EXT.signatures, _EXT.streamed, _EXT.operands
lib, launch, last_error = _EXT.lib, _EXT.launch, _EXT.last_error      # module-level names: the functions below reach ``launch`` through the module's globals at call time
CHUNK = _EXT.constant("DD_TOPK_CHUNK")                     # elements per piece: a workgroup's share of one sample
TABLE_MAX = _EXT.constant("DD_TOPK_TABLE_MAX")             # per-sample masks of a pointer table; a longer tuple is stacked
BINS = _EXT.constant("DD_TOPK_BINS")                       # histogram counters per sample
PIECE_BYTES = _EXT.constant("DD_TOPK_PIECE_BYTES")
STATE_BYTES = _EXT.constant("DD_TOPK_STATE_BYTES")


def workspace_bytes(batch, per):
    """The bytes a call on ``batch`` samples of ``per`` elements needs (the header: there is no size query)."""
    return int(batch) * (PIECE_BYTES * (-(-int(per) // CHUNK)) + 4 * BINS + STATE_BYTES)


# ---- the two launch functions as one function of tensors ---------------------------------------------------------------------------
def _operands(logits, target):
    """Host-side check of the [B, P] fp32 ``logits`` and the byte target -> (entry point, the operand that describes the target, what
    keeps it alive).  A tuple of at most TABLE_MAX masks goes as a HOST pointer table; a longer one is stacked: the same bits."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.numel() == 0:
        raise HotpathError(f"topk_loss: logits must be [B, P] with no empty dimension, got {tuple(getattr(logits, 'shape', ()))}")
    _lib.dev(logits, "topk_loss: logits")
    b, per = logits.shape
    if isinstance(target, (tuple, list)):
        if len(target) != b:
            raise HotpathError(f"topk_loss: {len(target)} masks for {b} samples")
        for t in target:
            if isinstance(t, torch.Tensor) and t.dtype.is_floating_point:
                raise HotpathError(f"topk_loss: a floating-point target ({t.dtype}) is refused: the selection is defined on 0 / 1 labels (bool / uint8)")
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype in (torch.bool, torch.uint8) and t.numel() == per):
                raise HotpathError(f"topk_loss: per-sample masks must be contiguous bool / uint8 device tensors of {per} elements")
        if b <= TABLE_MAX:
            return "dd_topk_bce_u8_ptrs", (C.c_void_p * b)(*[t.data_ptr() for t in target]), target
        target = torch.stack(tuple(t.reshape(-1) for t in target), dim=0)
    if isinstance(target, torch.Tensor) and target.dtype.is_floating_point:
        raise HotpathError(f"topk_loss: a floating-point target ({target.dtype}) is refused: the selection is defined on 0 / 1 labels (bool / uint8)")
    if not (isinstance(target, torch.Tensor) and target.is_cuda and target.is_contiguous() and tuple(target.shape) == (b, per)
            and target.dtype in (torch.uint8, torch.bool)):
        raise HotpathError(f"topk_loss: target must be a contiguous uint8 / bool device tensor of shape {(b, per)} or a tuple of per-sample "
                           f"masks, got {getattr(target, 'dtype', type(target))} {tuple(getattr(target, 'shape', ()))}")
    return "dd_topk_bce", target, target


def fwd(logits, target, keep, grad=True, grad_scale=1.0, want_probs=True):
    """dd_topk_bce / dd_topk_bce_u8_ptrs outside autograd -> (losses fp32 [2] = {L, L_all}, probs fp32 [B, P] or None, stats fp64 [B, 4] =
    {n_b, sum_{S_b} sp, tau_b, sum_all sp}, dlogits fp32 [B, P] = dL/dz * grad_scale or None with ``grad=False``)."""
    name, described, _alive = _operands(logits, target)
    b, per = logits.shape
    keep = int(keep)
    if not 1 <= keep <= per:
        raise HotpathError(f"topk_loss: keep = {keep} must be in 1 .. {per}")
    dev = logits.device
    losses = torch.empty(2, device=dev, dtype=torch.float32)
    stats = torch.empty((b, 4), device=dev, dtype=torch.float64)
    probs = torch.empty_like(logits) if want_probs else None
    dz = torch.empty_like(logits) if grad else None
    nbytes = workspace_bytes(b, per)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    launch(name, logits.detach(), described, b, per, keep, float(grad_scale), probs, dz, losses, stats, ws, nbytes)
    return losses, probs, stats, dz


# ---- autograd --------------------------------------------------------------------------------------------------------------------
class TopKBce(torch.autograd.Function):
    """(logits [B, P], target, keep) -> (loss, probs, stats); ``probs`` and ``stats`` carry no gradient.  ``target``: the stacked byte
    target or the tuple of per-sample masks.  The gradient is written with the forward, as the package's other losses do."""

    @staticmethod
    def forward(ctx, logits, target, keep):
        losses, probs, stats, dz = fwd(logits, target, keep, grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(probs, stats)
        ctx.set_materialize_grads(False)      # no 82 MB of zeros for the probabilities' (unused) gradient slot
        return losses[0], probs, stats

    @staticmethod
    def backward(ctx, g, _gp, _gs):
        (dz,) = ctx.saved_tensors
        if g is None or dz is None:
            return None, None, None
        return ops._scaled_loss_grad(ctx, dz, g), None, None


def topk_bce(logits, target, keep):
    """The bootstrapped BCE of ``logits`` [B, P] (fp32) against the 0/1 byte ``target`` over each sample's ``keep`` hardest pixels ->
    ``(loss, probs, stats)``: the 0-dim loss, differentiable in ``logits``; sigmoid(logits), the bits of ``ops.sigmoid``; ``stats`` fp64
    [B, 4] = {n_b, sum over the kept pixels, tau_b, sum over all pixels}."""
    return TopKBce.apply(logits, target, keep)


# ---- the anneal --------------------------------------------------------------------------------------------------------------------
def keep_now(frac, warmup_steps, t, per):
    """K at step ``t``: ``ceil(f per)`` clamped to 1 .. per, with ``f = 1 - (1 - frac) min(t / T, 1)`` -- 1 at step 0, ``frac`` from step
    ``T = warmup_steps`` on -- and ``f = frac`` when ``T <= 0``.  In Python doubles."""
    f = float(frac) if warmup_steps <= 0 else 1.0 - (1.0 - float(frac)) * min(float(t) / float(warmup_steps), 1.0)
    return max(1, min(int(per), int(math.ceil(f * int(per)))))


def check_hparams(hparams):
    """``(rm_topk_frac, rm_topk_warmup_steps)`` of ``hparams`` (absent: 1, 0).  A fraction outside (0, 1] or a negative warm-up raises
    ValueError."""
    frac, steps = hparam(hparams, "rm_topk_frac", 1.0), hparam(hparams, "rm_topk_warmup_steps", 0)
    try:
        frac = float(1.0 if frac is None else frac)
    except (TypeError, ValueError):
        raise ValueError(f"rm_topk_frac must be a number, got {frac!r}") from None
    if not 0.0 < frac <= 1.0:
        raise ValueError(f"rm_topk_frac must be in (0, 1], got {frac!r}")
    try:
        steps = int(0 if steps is None else steps)
    except (TypeError, ValueError):
        raise ValueError(f"rm_topk_warmup_steps must be an integer, got {steps!r}") from None
    if steps < 0:
        raise ValueError(f"rm_topk_warmup_steps must be >= 0, got {steps}")
    return frac, steps


def add_topk_args(p):
    """``--rm_topk_frac`` / ``--rm_topk_warmup_steps``, for the parser of a script that trains ``RoadMapBCE``."""
    p.add_argument("--rm_topk_frac", type=float, default=1.0,
                   help="road-map loss: average the BCE over this fraction of each scene's pixels, the hardest ones (0 < F <= 1); 1 = off, "
                        "the mean over all pixels")
    p.add_argument("--rm_topk_warmup_steps", type=int, default=0,
                   help="steps over which the kept fraction falls linearly from 1 to rm_topk_frac; 0 = rm_topk_frac from the first step")
    return p
