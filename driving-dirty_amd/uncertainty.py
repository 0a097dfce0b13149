"""Per-pixel uncertainty from the S dropout draws of a sampled prediction, in the same one pass of the head.

``mc.py`` draws the encoder's dense tail S times per scene and keeps the mean of the S probabilities.  The spread of the draws is the
other half of what MC dropout is for: where the draws DISAGREE the model is unsure (model uncertainty: the mutual information between
prediction and weights, BALD); where every draw says 0.5 the data is (entropy without mutual information).  After the head's
contraction a workgroup holds all S draws of its 128 columns, so the statistics are taken there: neither logits nor probabilities of
the single draws are written.

Two parts.  The BINDER of ``csrc/libdd_head_uncert.so`` (``include/dd_head_uncert.h``), a ``_lib.Extension`` of its entry in
``build.UNCERTAINTY_EXTENSIONS``.  And what is composed of it: ``head_uncertainty`` on tensors, ``predict`` for a model's
``predict_uncertainty``, ``validation_scores`` for its ``validation_step`` under ``--mc_uncertainty``.

THE SEMANTICS are the header's, in nats: ``mean`` with the bits of ``mc.mean_prob``; ``entropy`` the binary entropy of the mean; ``mi``
= entropy minus the mean over the draws of each draw's entropy (taken from the logit: finite in both tails), never negative; ``var``
the population variance of the S probabilities; ``scores[b] = (mean_j entropy, mean_j mi, mean_j var)`` in fp64, added in a fixed order:
the same bits on every run and whatever else is written.

Off by default, and nothing imports this module until it is asked for.  ``hparams.mc_uncertainty`` (``--mc_uncertainty``) lives in the
hparams, as ``mc_samples`` does.
"""
from collections import namedtuple

import torch

from . import _lib
from . import build as _build
from . import mc as _mc
from ._lib import HotpathError
from .lightning import hparam

# ---- the binder ------------------------------------------------------------------------------------------------------------------
_EXT = _lib.Extension(_build.UNCERTAINTY_EXTENSIONS["head_uncert"])
LIB, SIGNATURES, STREAMED, OPERANDS = _EXT.library, _EXT.signatures, _EXT.streamed, _EXT.operands
lib, launch, last_error = _EXT.lib, _EXT.launch, _EXT.last_error      # module-level names: the functions below reach ``launch`` through the module's globals at call time

BLOCK = _EXT.constant("DD_HEAD_UNCERT_BLOCK")      # columns of a workgroup: ``partials`` holds one triple per block and scene
MAPS = ("mean", "entropy", "mi", "var")            # header order
SCORES = ("entropy", "mi", "var")                  # the columns of ``scores``
VAL_KEYS = ("val_mc_entropy", "val_mc_mi", "val_mc_var")


# ---- the launch as a function of tensors ---------------------------------------------------------------------------------------------
def _fields(maps, scores):
    if isinstance(maps, str):
        maps = (maps,)
    maps = tuple(maps)
    for m in maps:
        if m not in MAPS:
            raise ValueError(f"head_uncertainty: maps are chosen from {MAPS}, got {m!r}")
    if len(set(maps)) != len(maps):
        raise ValueError(f"head_uncertainty: a map is named twice in {maps}")
    if not maps and not scores:
        raise ValueError("head_uncertainty: no output requested (maps is empty and scores is off)")
    return maps


_RESULTS = {}


def _result(names):
    if names not in _RESULTS:
        _RESULTS[names] = namedtuple("HeadUncertainty", names)
    return _RESULTS[names]


def head_uncertainty(x, weight, bias, samples, maps=MAPS, scores=True):
    """fp32 ``x`` [scenes * samples, k], row ``b * samples + s`` draw ``s`` of scene ``b``; ``weight`` [n, k] and ``bias`` [n] (or None) of an
    nn.Linear -> a named tuple of the requested ``maps`` (fp32 [scenes, n] each, in the order asked for) and, under ``scores``, a last
    field ``scores``: fp64 [scenes, 3], the per-scene means of entropy, mutual information and variance (dd_head_uncert: one pass over
    the weight).  Outside autograd."""
    maps = _fields(maps, bool(scores))
    x, scenes, samples, n, k = _mc._operands("head_uncertainty", x, weight, bias, samples)
    out = {m: torch.empty((scenes, n), device=x.device, dtype=torch.float32) for m in maps}
    partials = result = None
    if scores:
        partials = torch.empty(((n + BLOCK - 1) // BLOCK, scenes, 3), device=x.device, dtype=torch.float64)
        result = torch.empty((scenes, 3), device=x.device, dtype=torch.float64)
    launch("dd_head_uncert", x, weight.detach(), None if bias is None else bias.detach(), *(out.get(m) for m in MAPS), partials, result,
           scenes, samples, n, k)
    names = maps + (("scores",) if scores else ())
    return _result(names)(*(out[m] for m in maps), *((result,) if scores else ()))


# ---- the mode --------------------------------------------------------------------------------------------------------------------
def enabled(hparams):
    """``hparams.mc_uncertainty``: anything but a bool (or absent = off) raises ValueError."""
    value = hparam(hparams, "mc_uncertainty", False)
    if not isinstance(value, bool):
        raise ValueError(f"mc_uncertainty must be True or False, got {value!r}")
    return value


def predict(module, encoder, pooled, samples, gen, maps=("mi",), scores=True, keeps=None):
    """``module.fc1`` (the road-map head) on ``samples`` draws of ``encoder``'s tail per row of ``pooled`` -> ``head_uncertainty``'s named
    tuple with the maps as [B,800,800]."""
    z = encoder.latent_samples(pooled, samples, keeps, gen)
    got = head_uncertainty(z, module.fc1.weight, module.fc1.bias, samples, maps, scores)
    return type(got)(*(v if name == "scores" else v.reshape(-1, 800, 800) for name, v in zip(got._fields, got)))


def validation_scores(out, scores):
    """``out`` <- ``val_mc_entropy`` / ``val_mc_mi`` / ``val_mc_var``: the batch means of the three per-scene scores."""
    out.update(zip(VAL_KEYS, scores.mean(0).float().unbind(0)))
    return out


def add_uncertainty_args(p):
    """``--mc_uncertainty``, for the ``add_model_specific_args`` of the model whose validation reports the draws' spread."""
    p.add_argument("--mc_uncertainty", action="store_true",
                   help="with mc_samples > 1: validation also reports val_mc_entropy / val_mc_mi / val_mc_var, the batch means of the "
                        "per-scene predictive entropy, mutual information (BALD) and variance of the dropout draws, from the same head pass; "
                        "kept in the checkpoint")
    return p

