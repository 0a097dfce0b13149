"""Road-map prediction averaged over S dropout draws, in one pass of the head.

The dense blocks' dropout is always on, as in the reference (components.py:108): a prediction is one random draw, and predicting the
same frames twice gives two maps.  Only the tail behind ``fc1``'s Linear is stochastic -- a few 128-wide layers -- and the head is one
stream over its 164 MB weight that up to 64 rows share.  So: the conv stack and ``fc1``'s Linear once, S draws of the tail per scene
(``Encoder.latent_samples``), and the head on the ``B * S`` latents with the mean of the S probabilities taken inside its kernel.
Neither logits nor probabilities of the single draws are written.

Two parts.  The BINDER of ``csrc/libdd_head_mean.so`` (``include/dd_head_mean.h``), a ``_lib.Extension`` of its entry in
``build.PREDICTION_EXTENSIONS``.  And the pieces a model's ``predict_*`` / ``validation_step`` are composed of: ``mean_prob``, ``mean_gt``,
``resolve``, ``generator``.

THE SEMANTICS are the header's: ``mean[b,j] = (p[b,0,j] + p[b,1,j] + ... + p[b,S-1,j]) * float32(1 / S)``, the sum taken left to right
in fp32, ``p`` the dense head's one sigmoid (csrc/dd_device.h) of ``dd_linear_fwd``'s logit for row ``b * S + s``.  A pixel is set
where ``mean > tau``, strictly, ``tau`` rounded to fp32: the rule of ``JointRoadMapBBox._own_road_masks``.

Off by default.  ``hparams.mc_samples`` (``--mc_samples``, 1) and ``hparams.mc_seed`` (``--mc_seed``, 0) live in the hparams, as
``tta_mirror`` does: they travel in the checkpoint, and a loaded model predicts in the mode its threshold was calibrated in.  Under
S > 1 the masks come from the module's OWN device generator, reseeded from ``mc_seed`` at every call: a prediction is a function of the
weights, the batch and the seed, and torch's global generators are not touched.  With S = 1 nothing here is reached: the parent's
calls, call for call, the global generator's single draw included.
"""
import torch

from . import _lib
from . import build as _build
from ._lib import HotpathError
from .lightning import hparam

# ---- the binder ------------------------------------------------------------------------------------------------------------------
_EXT = _lib.Extension(_build.PREDICTION_EXTENSIONS["head_mean"])
LIB, SIGNATURES, STREAMED, OPERANDS = _EXT.library, _EXT.signatures, _EXT.streamed, _EXT.operands
lib, launch, last_error = _EXT.lib, _EXT.launch, _EXT.last_error      # module-level names: the functions below reach ``launch`` through the module's globals at call time

MAX_SAMPLES = 64      # rows of one launch of the head (csrc/linear.hip runs 64 rows per launch)


# ---- the two kernels as functions of tensors ---------------------------------------------------------------------------------------
def _operands(who, x, weight, bias, samples):
    samples = _samples(samples, f"{who}: samples")
    x = _lib.dev(x.detach(), f"{who}: x")
    if x.dim() != 2 or x.shape[0] == 0 or x.shape[0] % samples:
        raise HotpathError(f"{who}: expected fp32 [scenes * {samples}, k] (scene-major), got {tuple(x.shape)}")
    n, k = weight.shape
    _lib.dev(weight.detach(), f"{who}: weight", (n, x.shape[1]))
    if bias is not None:
        _lib.dev(bias.detach(), f"{who}: bias", (n,))
    return x, x.shape[0] // samples, samples, n, k


def mean_prob(x, weight, bias, samples):
    """fp32 ``x`` [scenes * samples, k], row ``b * samples + s`` draw ``s`` of scene ``b``; ``weight`` [n, k] and ``bias`` [n] (or None) of
    an nn.Linear -> fp32 [scenes, n]: the mean over a scene's draws of ``sigmoid(x W^T + b)`` (dd_head_mean_prob).  Outside autograd."""
    x, scenes, samples, n, k = _operands("mean_prob", x, weight, bias, samples)
    out = torch.empty((scenes, n), device=x.device, dtype=torch.float32)
    launch("dd_head_mean_prob", x, weight.detach(), None if bias is None else bias.detach(), out, scenes, samples, n, k)
    return out


def mean_gt(x, weight, bias, tau, samples):
    """The same mean ``> tau`` (strictly, ``tau`` rounded to fp32; a NaN mean is False) as torch.bool [scenes, n], one byte per element
    from the head's kernel (dd_head_mean_gt): nothing but the map reaches memory."""
    x, scenes, samples, n, k = _operands("mean_gt", x, weight, bias, samples)
    out = torch.empty((scenes, n), device=x.device, dtype=torch.uint8)
    launch("dd_head_mean_gt", x, weight.detach(), None if bias is None else bias.detach(), float(tau), out, scenes, samples, n, k)
    return out.view(torch.bool)


# ---- the mode --------------------------------------------------------------------------------------------------------------------
def _samples(value, name="mc_samples"):
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= MAX_SAMPLES:
        raise ValueError(f"{name} must be an integer in 1 .. {MAX_SAMPLES}, got {value!r}")
    return value


def _seed(value, name="mc_seed"):
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value < 2 ** 63:
        raise ValueError(f"{name} must be a non-negative integer, got {value!r}")
    return value


def resolve(module, mc_samples):
    """The ``mc_samples=`` argument of a prediction -> S: the argument, else ``module.hparams.mc_samples``, else 1 (off).  Anything but
    an integer in 1 .. 64 raises ValueError."""
    if mc_samples is None:
        mc_samples = hparam(getattr(module, "hparams", None), "mc_samples", 1)
    return _samples(mc_samples)


def seed_of(module):
    """``module.hparams.mc_seed``, else 0; anything but a non-negative integer raises ValueError."""
    return _seed(hparam(getattr(module, "hparams", None), "mc_seed", 0))


def check_hparams(hparams):
    """What a model's constructor calls: both values as ``resolve`` / ``seed_of`` would refuse them later."""
    _samples(hparam(hparams, "mc_samples", 1))
    _seed(hparam(hparams, "mc_seed", 0))


def generator(module, device):
    """The module's own generator on ``device``, reseeded from ``hparams.mc_seed``: what every S > 1 call draws its masks from.  Made at
    the first call and kept as a plain attribute (never a state_dict key); torch's global generators are not touched."""
    device = torch.device(device)
    gen = getattr(module, "_mc_generator", None)
    if gen is None or gen.device != device:
        gen = torch.Generator(device=device)
        module._mc_generator = gen
    gen.manual_seed(seed_of(module))
    return gen


def head_mean_prob(module, encoder, pooled, samples, gen, keeps=None):
    """``module.fc1`` (the road-map head) on ``samples`` draws of ``encoder``'s tail per row of ``pooled`` -> fp32 [B,800,800], the mean
    probabilities."""
    z = encoder.latent_samples(pooled, samples, keeps, gen)
    return mean_prob(z, module.fc1.weight, module.fc1.bias, samples).reshape(-1, 800, 800)


def head_mean_gt(module, encoder, pooled, samples, gen, tau, keeps=None):
    """The same ``> tau`` -> torch.bool [B,800,800]."""
    z = encoder.latent_samples(pooled, samples, keeps, gen)
    return mean_gt(z, module.fc1.weight, module.fc1.bias, tau, samples).reshape(-1, 800, 800)


def _arg(check, flag):
    def parse(text):
        import argparse
        try:
            return check(int(text), flag)
        except ValueError as e:
            raise argparse.ArgumentTypeError(str(e) if flag in str(e) else f"{flag} must be an integer, got {text!r}") from None
    parse.__name__ = flag
    return parse


def add_mc_args(p):
    """``--mc_samples`` / ``--mc_seed``, for the ``add_model_specific_args`` of the models with a road-map head behind the encoder's tail."""
    p.add_argument("--mc_samples", type=_arg(_samples, "mc_samples"), default=1,
                   help="predict (and validate / calibrate the threshold) from the mean of this many dropout draws of the encoder's dense "
                        "tail per scene, 1 .. 64, in one pass of the road-map head; 1 = a single draw; kept in the checkpoint")
    p.add_argument("--mc_seed", type=_arg(_seed, "mc_seed"), default=0,
                   help="seed of the model's own generator for those draws: with mc_samples > 1 a prediction is a function of the weights, "
                        "the batch and this seed; kept in the checkpoint")
    return p
