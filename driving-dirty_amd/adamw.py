"""Decoupled weight decay (AdamW) on the device: the BINDER of ``csrc/libdd_adamw.so`` (``include/dd_adamw.h``), a ``_lib.Extension``
of its entry in ``build.OPTIMIZER_EXTENSIONS``, the factor the kernels take, the shims ``optim.HipAdam`` calls, and the command line.

THE SEMANTICS are the header's: per element of a decayed tensor ``p1 = p * keep`` -- one fp32 multiply, one rounding -- and then the
Adam element of ``csrc/dd_adam.h`` on ``(p1, g, m, v)``, unchanged; ``keep = float32(1 - lr * weight_decay)`` computed in double on
the host.  That is ``torch.optim.AdamW``: the moments never see the decay.  ``keep == 1`` is the parent's step, and ``HipAdam`` then
makes the parent's calls: nothing of this module is entered.
"""
import ctypes as C
import math

from . import _lib, ops
from . import build as _build
from ._lib import HotpathError

# ---- the binder ------------------------------------------------------------------------------------------------------------------
_EXT = _lib.Extension(_build.OPTIMIZER_EXTENSIONS["adamw"])
LIB, SIGNATURES, STREAMED, OPERANDS = _EXT.library, _EXT.signatures, _EXT.streamed, _EXT.operands
lib, launch, last_error = _EXT.lib, _EXT.launch, _EXT.last_error      # module-level names: the shims below reach ``launch`` through the module's globals at call time


def keep_of(lr, weight_decay):
    """The factor a decayed parameter is multiplied by in front of its Adam update, as the fp32 the kernels are handed:
    ``float32(1 - lr * weight_decay)``, the product and the difference in double (torch.optim.AdamW's ``param.mul_(1 - lr *
    weight_decay)``, whose Python double torch rounds to fp32 once).  ``lr * weight_decay > 1`` is refused: not a decay."""
    keep = 1.0 - float(lr) * float(weight_decay)
    if not 0.0 <= keep <= 1.0:      # a NaN fails both
        raise ValueError(f"keep = 1 - lr * weight_decay = {keep} is outside [0, 1] (lr = {lr}, weight_decay = {weight_decay})")
    return C.c_float(keep).value


def check_weight_decay(weight_decay, who):
    """``weight_decay`` as a float; negative or non-finite values are refused in ``who``'s name."""
    wd = float(weight_decay or 0.0)
    if not (math.isfinite(wd) and wd >= 0.0):
        raise ValueError(f"{who}: weight_decay = {weight_decay}: a finite number >= 0 is needed")
    return wd


# ---- the shims, operand checks as ops.adam_step_flat / ops.adam_step_multi ------------------------------------------------------------
def step_flat(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale, keep):
    """``dd_adamw_step`` on flat fp32 device tensors of equal length; ``grad_scale`` a number, or a one-element fp32 device tensor
    that the kernel reads when it starts (clipping)."""
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        ops._dev(t, name, p.shape)
    scale, scale_dev = ops._scale_arg(grad_scale)
    launch("dd_adamw_step", p, g, m, v, p.numel(), lr, beta1, beta2, eps, int(step), 0.0 if scale is None else scale, scale_dev, keep)


def step_multi(tensors, keeps, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """``dd_adamw_step_multi``: one launch for a list of small (p, g, m, v) quadruples that share ``step``, ``keeps[i]`` the factor of
    quadruple i (1.0: it does not decay)."""
    if not tensors:
        return
    if len(keeps) != len(tensors):
        raise HotpathError(f"step_multi: {len(keeps)} factors for {len(tensors)} tensors")
    table = ops._adam_table(tensors)
    scale, scale_dev = ops._scale_arg(grad_scale)
    launch("dd_adamw_step_multi", table, (C.c_float * len(keeps))(*keeps), len(tensors), lr, beta1, beta2, eps, int(step),
           0.0 if scale is None else scale, scale_dev)


def decay(p, keep):
    """``dd_decay``: ``p *= keep`` in place on the current stream (the pre-scale in front of a rank-B pass)."""
    ops._dev(p, "p")
    launch("dd_decay", p, p.numel(), keep)


# ---- the command line --------------------------------------------------------------------------------------------------------------
def add_weight_decay_args(p):
    """``--weight_decay`` / ``--weight_decay_all``, for the ``add_model_specific_args`` of the models ``train.TrainStep`` trains."""
    p.add_argument("--weight_decay", type=float, default=0.0,
                   help="decoupled weight decay (torch.optim.AdamW's) inside TrainStep's optimizer passes (0: off); biases and "
                        "BatchNorm vectors (parameters of at most one dimension) do not decay")
    p.add_argument("--weight_decay_all", action="store_true", help="decay every parameter, the one-dimensional ones too")
    return p
