"""Mirror test-time averaging on the device: predict from the scene and from its left/right mirror, reflect the second answer back and
average the PROBABILITIES before the threshold.

The other half of ``augment.py``'s mirror: a model trained with ``--aug_mirror`` has seen both orientations of every
scene, and this is how a prediction uses both.  Two parts.  The BINDER of ``csrc/libdd_tta.so`` (``include/dd_tta.h``), a
``_lib.Extension`` of its entry in ``build.EXTENSIONS``.  And the pieces a model's ``predict_*`` / ``validation_step`` are composed of: ``mirror_views``,
``mirror_masks``, ``mean_prob``, ``mean_gt``, ``resolve``.

THE SEMANTICS are the header's: ``mean[b,r,c] = 0.5f * (P(a[b,r,c]) + P(m[b,h-1-r,c]))`` with ``a`` from the scene and ``m`` from the
mirrored scene -- the rows reverse because the bird's-eye frame has y to the left along the rows, the reversal ``augment_masks``
applies to a mirrored sample's road mask.  ``P`` is the identity, or the dense head's one sigmoid (csrc/dd_device.h).  A pixel is set
where ``mean > tau``, strictly, ``tau`` rounded to fp32: the rule of ``JointRoadMapBBox._own_road_masks``.

Off by default.  ``hparams.tta_mirror`` (``--tta_mirror``) lives in the hparams, as ``rm_threshold`` does: it travels in the
checkpoint, and a loaded model predicts in the mode its thresholds were calibrated in.  There is ONE ``rm_threshold`` and ONE
``box_threshold``: under the flag validation calibrates them on the averaged probabilities (which are less extreme than single ones),
and a ``tta=False`` prediction from such a checkpoint reuses them as they are.
"""
import torch

from . import _lib, augment
from . import build as _build
from ._lib import HotpathError
from .lightning import hparam

# ---- the binder ------------------------------------------------------------------------------------------------------------------
_EXT = _lib.Extension(_build.EXTENSIONS["tta"])
LIB, SIGNATURES, STREAMED, OPERANDS = _EXT.library, _EXT.signatures, _EXT.streamed, _EXT.operands
lib, launch, last_error = _EXT.lib, _EXT.launch, _EXT.last_error      # module-level names: the functions below reach ``launch`` through the module's globals at call time

MIRROR = "mirror"      # the one mode there is besides off (None)


# ---- the mirrored scene ------------------------------------------------------------------------------------------------------------
def _batch_size(x):
    return x.shape[0] if isinstance(x, torch.Tensor) else len(x)


def mirror_views(x):
    """Whatever ``forward`` takes (fp32 views [B,6,3,H,W] or uint8 frames [B,6,H,W,3], stacked or the collate's tuple) -> ONE stacked
    fp32 [B,6,3,H,W], every sample mirrored: ``augment.augment_views`` with flag 1 and the identity colour, which moves values bit for
    bit and, applied twice, is the identity."""
    b = _batch_size(x)
    color = torch.tensor([1.0, 0.0]).repeat(b, 6, 1)
    return augment.augment_views(x, [augment.FLAG_MIRROR] * b, color)


def mirror_masks(rm):
    """The road map of the mirrored scene, rows reversed.  bool / uint8 masks (a tuple of [h,w] or stacked [B,h,w]) ->
    ``augment.augment_masks`` with every flag 1: a tuple of B contiguous views of ONE stacked tensor, dtype kept, the form the box
    branch gathers from.  An fp32 map [B,1,h,w] (the other form ``forward(x, rm)`` takes) -> ``torch.flip`` along its rows: a copy
    with no arithmetic, and the one place torch moves data on the averaged path."""
    if isinstance(rm, torch.Tensor) and rm.is_floating_point():
        if rm.dim() != 4:
            raise HotpathError(f"mirror_masks: a floating-point road map is [B,1,h,w], got {tuple(rm.shape)}")
        return torch.flip(rm, dims=(2,))
    return augment.augment_masks(rm, [augment.FLAG_MIRROR] * _batch_size(rm))


# ---- the two kernels as functions of tensors ---------------------------------------------------------------------------------------
def _operands(who, a, m):
    _lib.dev(a, f"{who}: a")
    if a.dim() != 3 or a.numel() == 0:
        raise HotpathError(f"{who}: expected fp32 [B,h,w] with no empty dimension, got {tuple(a.shape)}")
    _lib.dev(m, f"{who}: m", tuple(a.shape))
    return tuple(a.shape)


def mean_prob(a, m, from_logits):
    """fp32 [B,h,w] ``a`` (from the scene) and ``m`` (from the mirrored scene) -> fp32 [B,h,w] ``0.5f * (P(a) + P(m) row-reversed)``
    (dd_tta_mean_prob).  ``from_logits``: P is the dense head's sigmoid, else the identity.  Outside autograd."""
    b, h, w = _operands("mean_prob", a, m)
    out = torch.empty((b, h, w), device=a.device, dtype=torch.float32)
    launch("dd_tta_mean_prob", a.detach(), m.detach(), out, b, h, w, int(bool(from_logits)))
    return out


def mean_gt(a, m, tau, from_logits):
    """The same mean ``> tau`` (strictly, ``tau`` rounded to fp32; a NaN mean is False) as torch.bool [B,h,w], one byte per element
    from one kernel (dd_tta_mean_gt): neither the probabilities nor the mean reach memory."""
    b, h, w = _operands("mean_gt", a, m)
    out = torch.empty((b, h, w), device=a.device, dtype=torch.uint8)
    launch("dd_tta_mean_gt", a.detach(), m.detach(), float(tau), out, b, h, w, int(bool(from_logits)))
    return out.view(torch.bool)


# ---- the mode --------------------------------------------------------------------------------------------------------------------
def resolve(module, tta):
    """The ``tta=`` argument of a prediction -> the mode, ``MIRROR`` or None (off).  None: ``module.hparams.tta_mirror`` (default
    False); False: off; True / "mirror": the mirror.  Anything else raises ValueError."""
    if tta is None:
        tta = bool(hparam(getattr(module, "hparams", None), "tta_mirror", False))
    if tta is False:
        return None
    if tta is True or (isinstance(tta, str) and tta == MIRROR):
        return MIRROR
    raise ValueError(f"tta must be None (hparams.tta_mirror), False, True or 'mirror', got {tta!r}")


def add_tta_args(p):
    """``--tta_mirror``, for the ``add_model_specific_args`` of the models that predict from the cameras."""
    p.add_argument("--tta_mirror", action="store_true",
                   help="predict (and validate / calibrate the thresholds) from the scene AND its left/right mirror: the mean of the two "
                        "probabilities, the mirrored one reflected back; kept in the checkpoint")
    return p
