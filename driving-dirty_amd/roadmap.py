"""``RoadMapBCE`` / ``RoadMap``: the road-map LightningModules on the HIP hot path.

Reference: src/roadmap_model/roadmap_bce_v2.py (registry name ``roadmap_bce``) and
src/roadmap_model/roadmap_pretrain_ae.py (``roadmap_mse``).  Same constructor, ``forward``,
``_run_step``, ``training_step``, ``validation_step``, ``validation_epoch_end``,
``configure_optimizers`` and ``state_dict`` keys (``ae.encoder.*``, ``fc1.*``).
"""
from argparse import ArgumentParser
from contextlib import contextmanager

import torch
from torch import nn
from torch.nn import functional as F

from . import mc as _mc
from . import ops
from . import tta as _tta
from . import augment as _augment
from .augment import Augmenter, add_augment_args, current_rank
from .adamw import add_weight_decay_args
from .ema import add_ema_args
from .autoencoder import BasicAE
from .lightning import LightningModule, hparam, pretrained_ae


@contextmanager
def eval_no_grad(module):
    """``module`` in ``eval()`` mode under ``no_grad``; on exit every submodule's mode is what it was (a frozen extractor stays in eval
    inside a training model)."""
    modes = [(m, m.training) for m in module.modules()]
    module.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        for m, was in modes:
            m.training = was


def prediction_threshold(module, threshold):
    """The operating point of a prediction: ``threshold``, else the calibrated ``rm_threshold`` of ``module.hparams`` where there is
    one, else the reference's 0.5."""
    if threshold is None:
        threshold = hparam(module.hparams, "rm_threshold", None)
    return 0.5 if threshold is None else float(threshold)


def predict_map(module, latent, threshold):
    """``module``'s road-map head as a boolean map: ``latent()`` (the encoder) -> ``ops.linear_sigmoid_gt`` with ``module.fc1``, under
    ``no_grad`` and in ``eval()`` mode; every submodule's mode is put back afterwards (a frozen extractor stays in eval inside a
    training model).  ``threshold=None``: the calibrated ``rm_threshold`` where there is one, else the reference's 0.5."""
    tau = prediction_threshold(module, threshold)
    with eval_no_grad(module):
        y = ops.linear_sigmoid_gt(latent(), module.fc1.weight, module.fc1.bias, tau)
    return y.reshape(y.size(0), 800, 800)


def predict_map_tta(module, encode, x, threshold):
    """``predict_map`` under mirror test-time averaging (tta.py): TWO passes at B, not one at 2 B -- ``encode(x)`` is the un-averaged
    path's encoder at its shapes, ``encode(tta.mirror_views(x))`` the same code on the mirrored scene -- ``ops.linear`` with
    ``module.fc1`` gives the logits of each, and ``tta.mean_gt`` the map: sigmoid of both, the mirrored one's rows reversed, the mean
    and the comparison in one kernel.  Same mode handling as ``predict_map``.  The dense blocks' dropout is on in eval mode too, as in
    the reference, so the two passes also draw two dropout masks."""
    tau = prediction_threshold(module, threshold)
    with eval_no_grad(module):
        weight, bias = module.fc1.weight, module.fc1.bias
        logits = ops.linear(encode(x), weight, bias).reshape(-1, 800, 800)
        logits_m = ops.linear(encode(_tta.mirror_views(x)), weight, bias).reshape(-1, 800, 800)
        return _tta.mean_gt(logits, logits_m, tau, True)


def predict_map_mc(module, pooled, x, threshold, tta, samples):
    """``predict_map`` / ``predict_map_tta`` from the mean of ``samples`` > 1 dropout draws per scene (mc.py): ``pooled(x)`` is the conv
    stack up to the encoder's pooled vector, run ONCE per pass; ``Encoder.latent_samples`` draws the tail ``samples`` times per scene
    from the module's own generator, reseeded from ``hparams.mc_seed`` here; ``mc.mean_gt`` with ``module.fc1`` is the head, the mean of a
    scene's probabilities and the comparison in one kernel.  Under the mirror mode ``tta`` each of the two passes yields its mean
    through ``mc.mean_prob`` (the mirrored pass goes on drawing from the same generator) and ``tta.mean_gt`` brings the two together.
    Same mode handling as ``predict_map``."""
    tau = prediction_threshold(module, threshold)
    with eval_no_grad(module):
        enc = module.ae.encoder
        gen = _mc.generator(module, module.fc1.weight.device)
        if tta is None:
            return _mc.head_mean_gt(module, enc, pooled(x), samples, gen, tau)
        probs = _mc.head_mean_prob(module, enc, pooled(x), samples, gen)
        probs_m = _mc.head_mean_prob(module, enc, pooled(_tta.mirror_views(x)), samples, gen)
        return _tta.mean_gt(probs, probs_m, tau, False)


def mc_road_map_scores(out, target_rm, avg_probs):
    """``out`` <- ``val_ts_mc`` / ``val_ts_rounded_mc``: ``road_map_scores`` of the probabilities averaged over the draws (hparams.mc_samples)."""
    out.update({k + "_mc": v for k, v in road_map_scores(target_rm, avg_probs).items()})
    return out


MC_ROAD_KEYS = ("val_ts_mc", "val_ts_rounded_mc")
VAL_UNCERTAINTY_KEYS = ("val_mc_entropy", "val_mc_mi", "val_mc_var")      # uncertainty.VAL_KEYS, under hparams.mc_uncertainty


def tta_road_map_scores(out, target_rm, avg_probs):
    """``out`` <- ``val_ts_tta`` / ``val_ts_rounded_tta``: ``road_map_scores`` of the averaged probabilities (hparams.tta_mirror)."""
    out.update({k + "_tta": v for k, v in road_map_scores(target_rm, avg_probs).items()})
    return out


TTA_ROAD_KEYS = ("val_ts_tta", "val_ts_rounded_tta")


def mc_validation_probs(module, out, target_rm, mc_probs, sample, samples, mode):
    """The validation step's extra pass under ``hparams.mc_samples`` > 1: ``mc_probs(sample, samples, gen)`` in ``eval()`` mode under
    ``no_grad`` -> ``out`` gains ``val_ts_mc`` / ``val_ts_rounded_mc``; under the mirror ``mode`` the same on the mirrored batch, and
    ``val_ts_tta`` / ``val_ts_rounded_tta`` from ``tta.mean_prob`` of the two means.  Returns the most-averaged probabilities, which
    ``ts_hist`` is taken from."""
    with eval_no_grad(module):
        gen = _mc.generator(module, module.fc1.weight.device)
        avg = mc_probs(sample, samples, gen)
        mc_road_map_scores(out, target_rm, avg)
        if mode is not None:
            avg = _tta.mean_prob(avg, mc_probs(_tta.mirror_views(sample), samples, gen), False)
            tta_road_map_scores(out, target_rm, avg)
    return avg


def mc_uncertainty_config(hparams):
    """``hparams.mc_uncertainty`` (off by default): False without importing ``uncertainty`` when the hparam is absent or
    false; anything but a bool raises ValueError here, when the module is built."""
    if hparam(hparams, "mc_uncertainty", False) is False:
        return False
    from . import uncertainty      # here, not at the top: a model with the flag off never imports it
    return uncertainty.enabled(hparams)


def compute_ts_road_map(road_map1, road_map2):
    """Threat score, reference src/utils/helper.py:74-77 (one fused pass on the device)."""
    return ops.threat_score(road_map1.contiguous(), road_map2.contiguous())


def road_map_scores(target_rm, probs):
    """{'val_ts', 'val_ts_rounded'} of a validation batch: the threat score of the probabilities and of the rounded probabilities
    against the fp32 target (roadmap_bce_v2.py:117-118)."""
    target_rm, probs = target_rm.contiguous(), probs.contiguous()
    return {"val_ts": ops.threat_score(target_rm, probs), "val_ts_rounded": ops.threat_score(target_rm, probs, round_b=True)}


RM_LOSS_KEYS = ("val_rm_bce", "val_rm_soft_ts")      # validation's components of the road-map loss, under an ``rm_*`` setting


def rm_loss_config(hparams):
    """The road-map loss as the hparams ask for it: None when it is off (``rm_pos_weight`` None, ``rm_ts_weight`` 0, ``rm_bce_weight`` 1:
    the reference's mean BCE-with-logits, roadmap_bce_v2.py:106), else the keyword arguments of ``rm_loss.road_map_loss`` -- weighted
    BCE-with-logits plus the soft threat score on the logits.  ``rm_pos_weight``: None, a positive number (or a string
    that parses as one), or "auto" = each sample's own negatives / positives.  A value the kernels would refuse raises ValueError
    here, when the module is built.  ``rm_loss`` itself is imported by the step that takes the loss, not here."""
    pos_weight = hparam(hparams, "rm_pos_weight", None)
    if isinstance(pos_weight, str) and pos_weight != "auto":
        try:
            pos_weight = float(pos_weight)
        except ValueError:
            raise ValueError(f"rm_pos_weight must be a positive number or 'auto', got {pos_weight!r}") from None
    if pos_weight is not None and pos_weight != "auto":
        if isinstance(pos_weight, bool) or not isinstance(pos_weight, (int, float)) or not 0 < pos_weight < float("inf"):
            raise ValueError(f"rm_pos_weight must be a positive number or 'auto', got {pos_weight!r}")
        pos_weight = float(pos_weight)
    weights = {}
    for name, default in (("rm_bce_weight", 1.0), ("rm_ts_weight", 0.0), ("rm_ts_eps", 1.0)):
        try:
            weights[name] = float(hparam(hparams, name, default))
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number, got {hparam(hparams, name, default)!r}") from None
        if not 0 <= weights[name] < float("inf"):
            raise ValueError(f"{name} must be a finite number >= 0, got {weights[name]!r}")
    if weights["rm_bce_weight"] == 0 and weights["rm_ts_weight"] == 0:
        raise ValueError("rm_bce_weight and rm_ts_weight are both 0: the loss would be constant")
    if pos_weight is None and weights["rm_ts_weight"] == 0 and weights["rm_bce_weight"] == 1:
        return None
    return {"pos_weight": pos_weight, "bce_weight": weights["rm_bce_weight"], "ts_weight": weights["rm_ts_weight"], "ts_eps": weights["rm_ts_eps"]}


def add_rm_loss_args(p):
    """``--rm_pos_weight`` / ``--rm_bce_weight`` / ``--rm_ts_weight`` / ``--rm_ts_eps``, for the modules with a road-map head on logits."""
    p.add_argument("--rm_pos_weight", type=str, default=None,
                   help="road-map loss: weight of the positive (road) elements in the BCE: a positive number, or 'auto' = each sample's own "
                        "negatives / positives; default: unweighted (the reference's loss)")
    p.add_argument("--rm_bce_weight", type=float, default=1.0, help="road-map loss: factor of the (weighted) BCE-with-logits term")
    p.add_argument("--rm_ts_weight", type=float, default=0.0,
                   help="road-map loss: factor of the soft threat-score term 1 - (I + eps) / (U + eps), per sample; 0 = off")
    p.add_argument("--rm_ts_eps", type=float, default=1.0, help="road-map loss: eps of the soft threat score (>= 0)")
    return p


def road_map_loss_parts(setting, logits, target):
    """The loss of ``rm_loss_config``'s ``setting`` (not None) on ``logits`` [B, P] -> (loss, probs [B, P], (L_bce, L_ts))."""
    from . import rm_loss      # here, not at the top: a model with the rm_* hparams off never imports or loads the library
    loss, probs, bce, ts, _ = rm_loss.road_map_loss(logits, target, return_parts=True, **setting)
    return loss, probs, (bce, ts)


def cons_config(hparams):
    """The mirror consistency loss as the hparams ask for it: None when it is off (``cons_weight`` 0 or absent), else
    ``(cons_weight, cons_rampup_steps)`` as ``consistency.check_hparams`` gives them; a negative or non-finite weight or a negative ramp
    raises ValueError here, when the module is built.  With both hparams 0 or absent ``consistency`` is not imported."""
    if not hparam(hparams, "cons_weight", 0) and not hparam(hparams, "cons_rampup_steps", 0):
        return None
    from . import consistency      # here, not at the top: a model with the hparams off never imports it
    weight, rampup_steps = consistency.check_hparams(hparams)
    return (weight, rampup_steps) if weight > 0 else None


def refuse_consistency(hparams, who, why):
    """For the modules the consistency loss is not built into: ValueError by name when ``hparams.cons_weight`` > 0."""
    if cons_config(hparams) is not None:
        raise ValueError(f"cons_weight > 0 asks for the mirror consistency loss on unlabelled scenes; {who} {why}: use RoadMapBCE")


def topk_config(hparams):
    """The bootstrapped road-map loss as the hparams ask for it: None when it is off (``rm_topk_frac`` 1 or absent), else
    ``(rm_topk_frac, rm_topk_warmup_steps)`` as ``topk_loss.check_hparams`` gives them; a fraction outside (0, 1] or a negative warm-up
    raises ValueError here, when the module is built.  With the fraction 1 or absent and no warm-up ``topk_loss`` is not imported."""
    frac = hparam(hparams, "rm_topk_frac", None)
    if (frac is None or (not isinstance(frac, bool) and isinstance(frac, (int, float)) and frac == 1)) and not hparam(hparams, "rm_topk_warmup_steps", 0):
        return None
    from . import topk_loss      # here, not at the top: a model with the hparams off never imports it
    frac, warmup_steps = topk_loss.check_hparams(hparams)
    return (frac, warmup_steps) if frac < 1 else None


def refuse_topk(hparams, who, why):
    """For the modules the bootstrapped loss is not built into: ValueError by name when ``hparams.rm_topk_frac`` < 1."""
    if topk_config(hparams) is not None:
        raise ValueError(f"rm_topk_frac < 1 asks for the BCE over each scene's hardest pixels, a loss on the road-map head's logits; {who} {why}: "
                         "use RoadMapBCE")


class CalibratedThreshold:
    """What a module with a road-map head needs to calibrate its operating point on validation data (hparams.calibrate_threshold)
    and to carry it: the ``rm_threshold`` property, the per-batch histogram and the epoch's argmax.  Shared by the road-map modules
    and the joint model."""

    @property
    def rm_threshold(self):
        """The operating point ``validation_epoch_end`` calibrated (hparams.calibrate_threshold), a plain float, or None.  Kept in
        ``hparams`` -- not a buffer, not in the state_dict -- so ``save_checkpoint`` / ``load_from_checkpoint`` carry it."""
        return hparam(self.hparams, "rm_threshold", None)

    @rm_threshold.setter
    def rm_threshold(self, value):
        self.hparams.rm_threshold = None if value is None else float(value)

    def _with_ts_hist(self, out, probs, target_rm):
        if hparam(self.hparams, "calibrate_threshold", False):
            out["ts_hist"] = ops.ts_histogram(probs.detach().contiguous(), target_rm.contiguous())
        return out

    def _calibrate(self, outputs, logs):
        """Under hparams.calibrate_threshold: ``rm_threshold`` <- the threshold with the best threat score of the DATA SET (the summed
        histograms; the ``avg_*`` values are means of per-batch scores), and its figures into ``logs``."""
        if hparam(self.hparams, "calibrate_threshold", False):
            hist = torch.stack([x["ts_hist"] for x in outputs]).sum(0)
            ts, best = ops.ts_curve(hist)
            self.rm_threshold = best / ts.numel()
            logs.update(best_threshold=self.rm_threshold, best_val_ts=float(ts[best]), val_ts_at_half=float(ts[ts.numel() // 2]))
        return logs


class RoadMapBCE(CalibratedThreshold, LightningModule):
    """``hparams.cons_weight`` > 0 (off by default): ``training_step`` also accepts ``(sample, target, road_image,
    unlabelled)`` and adds ``cons_weight * ramp(t) * L_cons``, the mirror consistency loss (consistency.py) on the ``B_u`` unlabelled
    scenes, to the supervised loss of the ``B_l`` labelled ones.  The step is ONE forward over ``N = B_l + 2 B_u`` rows -- the labelled
    scenes, the unlabelled ones, their mirrors -- and one backward:
      * ``B_l + 2 B_u <= 64`` keeps ``TrainStep``'s fast path: past 64 rows ``HipAdam.linear_factors`` declines the rank-B pass by itself
        and the big Linear layers' gradients are materialised;
      * the dense blocks' BatchNorm statistics are taken over all ``N`` rows, the unlabelled ones included;
      * ``t`` counts the steps that carried an unlabelled part.  It is a plain attribute (``cons_step``), not checkpointed: a resumed
        run restarts the ramp;
      * the loss is per rank; under a live ``GradSync`` nothing new is needed, but it has not been run on more than one GPU.
    A 3-tuple is a supervised-only step, the calls of a model without the hparams; a 4-tuple under ``cons_weight`` 0 raises ValueError.
    Validation, prediction and calibration do not know about it.

    ``hparams.rm_topk_frac`` < 1 (off by default): the TRAINING step's loss is the BCE averaged over each scene's K hardest
    pixels (topk_loss.py), ``K = keep_now(rm_topk_frac, rm_topk_warmup_steps, t, 640000)`` falling from all pixels to the fraction over
    the warm-up.  ``t`` counts the training steps taken under the setting, a plain attribute (``topk_step``), not checkpointed: a resumed
    run restarts the anneal.  The log gains ``rm_bce_all`` (the plain mean BCE of the same pass), ``rm_topk_kept`` (the share of pixels
    kept) and ``rm_topk_tau`` (the mean threshold margin).  Validation, prediction and calibration keep the mean BCE: ``val_loss`` stays
    comparable between runs with and without the setting.  Together with an ``rm_*`` setting it raises ValueError; with ``cons_weight``
    it composes: the supervised rows of the longer forward take this loss."""
    rm_loss = None      # rm_loss_config(hparams): None = mean BCE-with-logits, the reference's loss
    _rm_parts = None    # (L_bce, L_ts) of the last ``_run_step`` under a setting
    cons = None         # cons_config(hparams): None = off, else (cons_weight, cons_rampup_steps)
    cons_step = 0       # steps so far that carried unlabelled scenes: the ramp's t
    topk = None         # topk_config(hparams): None = off, else (rm_topk_frac, rm_topk_warmup_steps)
    topk_step = 0       # training steps so far under ``topk``: the anneal's t
    _topk_parts = None  # (rm_bce_all, rm_topk_kept, rm_topk_tau) of the last training step under ``topk``

    def __init__(self, hparams):
        super().__init__()
        self.hparams = hparams
        self.rm_loss = rm_loss_config(hparams)
        _mc.check_hparams(hparams)
        mc_uncertainty_config(hparams)
        self.cons = cons_config(hparams)
        self.topk = topk_config(hparams)
        if self.topk is not None and self.rm_loss is not None:
            raise ValueError("rm_topk_frac < 1 selects the BCE over each scene's hardest pixels; rm_pos_weight / rm_bce_weight / rm_ts_weight "
                             "select another loss on the same logits, and the combination is not built: set one of the two")
        self.output_dim = 800 * 800
        # pretrained feature extractor (roadmap_bce_v2.py:43-47); ``pretrained_ae`` lets callers hand in
        # an already-built BasicAE when no checkpoint file exists (the reference's paths are NYU-local)
        self.ae = pretrained_ae(hparams)
        self.frozen = True
        self.ae.freeze()
        self.ae.decoder = None
        self.ae.encoder.precision = str(hparam(hparams, "precision", self.ae.encoder.precision))
        if self.ae.encoder.precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {self.ae.encoder.precision!r}")
        self.fc1 = nn.Linear(self.ae.latent_dim, self.output_dim)
        self.augment = Augmenter(hparams, rank=current_rank())      # train-time only; off unless an aug_* hparam is set

    def wide_stitch_six_images(self, sample):
        """tuple of B [6,3,H,W] -> [B,3,H,6W] (NCHW), views re-ordered.  roadmap_bce_v2.py:53-64."""
        if ops.is_u8_frames(sample):    # decoded frames: ToTensor's /255 (a true division) inside the gather kernel
            return ops.nhwc_to_nchw(ops.wide_image(sample), 3)
        x = torch.stack(tuple(sample), dim=0) if isinstance(sample, (tuple, list)) else sample
        return ops.stitch6(x.contiguous(), want_nhwc4=False, want_nchw=True)[1]

    def _encode(self, sample, keeps=(None, None)):
        """The 6-view gather (+ NHWC, + ToTensor's /255 for uint8 frames, + the bf16 rounding) in one pass over whatever the data
        pipeline handed over -- ops.wide_image -- then the encoder."""
        wide4 = ops.wide_image(sample, self.ae.encoder.precision)
        return self.ae.encoder.forward_nhwc4(wide4, keeps)

    def _logits(self, x, keeps=(None, None)):
        representations = self._encode(x, keeps)
        y = ops.linear(representations, self.fc1.weight, self.fc1.bias)
        return y.reshape(y.size(0), 800, 800)

    def forward(self, x, keeps=(None, None)):
        """-> (logits [B,800,800], sigmoid(logits)).  roadmap_bce_v2.py:66-81."""
        y = self._logits(x, keeps)
        return y, ops.sigmoid(y.detach())

    def _pooled(self, sample):
        """``_encode`` up to the encoder's pooled vector: what ``Encoder.latent_samples`` reads."""
        return self.ae.encoder.pooled_nhwc4(ops.wide_image(sample, self.ae.encoder.precision))

    def _mc_probs(self, sample, samples, gen):
        """Probabilities [B,800,800] averaged over ``samples`` dropout draws per scene, masks from ``gen``; for ``eval_no_grad``."""
        return _mc.head_mean_prob(self, self.ae.encoder, self._pooled(sample), samples, gen)

    def _mc_probs_scored(self, out):
        """``_mc_probs`` for the validation step under ``hparams.mc_uncertainty``: the same draws through ``dd_head_uncert`` with ``mean``
        requested -- the bits of ``mc.mean_prob`` -- and the batch means of the three per-scene scores into ``out``."""
        from . import uncertainty

        def probs(sample, samples, gen):
            got = uncertainty.predict(self, self.ae.encoder, self._pooled(sample), samples, gen, maps=("mean",), scores=True)
            if VAL_UNCERTAINTY_KEYS[0] not in out:      # the first pass: under the mirror mode the mirrored batch's scores are not reported
                uncertainty.validation_scores(out, got.scores)
            return got.mean
        return probs

    def predict_uncertainty(self, x, mc_samples=None, maps=("mi",), scores=True):
        """Where the model is unsure about ``x`` (whatever ``forward`` takes), from the spread of ``mc_samples`` dropout draws of the
        encoder's tail per scene (uncertainty.py) -> a named tuple of the requested ``maps`` -- chosen from "mean",
        "entropy", "mi", "var", fp32 [B,800,800] each -- and, under ``scores``, ``scores``: fp64 [B,3], each scene's mean entropy, mean
        mutual information and mean variance over its pixels.  In nats.  ``mi``, the mutual information between prediction and
        weights (BALD), is large where the draws disagree; ``entropy`` is also large where every draw says 0.5.

        The path is ``predict_road_map``'s under S > 1: eval mode, ``no_grad``, the module's own generator reseeded from
        ``hparams.mc_seed`` (the same call gives the same bits; torch's global generators are not touched), the conv stack and ``fc1``'s
        Linear once, S draws of the tail, and ONE pass of the head, in which the statistics are taken: the draws of a call of
        ``predict_road_map(x, mc_samples=S)`` are these draws, and "mean" is its mean.  ``mc_samples``: None = ``hparams.mc_samples``; a
        resolved S < 2 raises ValueError (one draw has no spread).  ``hparams.tta_mirror`` is ignored: the statistics are those of the
        unmirrored scene's draws."""
        samples = _mc.resolve(self, mc_samples)
        if samples < 2:
            raise ValueError(f"predict_uncertainty: mc_samples must be at least 2 (the spread of one draw is zero), got {samples}: pass "
                             "mc_samples= or set hparams.mc_samples")
        from . import uncertainty      # here, not at the top: a model that is never asked never imports or loads the library
        with eval_no_grad(self):
            gen = _mc.generator(self, self.fc1.weight.device)
            return uncertainty.predict(self, self.ae.encoder, self._pooled(x), samples, gen, maps, scores)

    def predict_road_map(self, x, threshold=None, mc_samples=None, tta=None):
        """The reference's "Predicting test images" step (run_test.py) for one batch: torch.bool [B,800,800], equal to ``forward``'s
        probabilities ``> threshold`` in eval mode.  ``x``: whatever ``forward`` takes.  Encoder, then the head, the sigmoid and the
        comparison in one kernel: neither logits nor probabilities are written.  (The dense blocks' dropout is on in eval mode too, as
        in the reference, components.py:108.)

        ``tta``: None = ``hparams.tta_mirror`` (default off), False = off, True / "mirror" = mirror test-time averaging
        (``predict_map_tta``): the scene and its mirror, each through encoder and head, the mean of the two probabilities
        ``> threshold``.  With dropout on the two passes draw two masks.  ``threshold=None`` is the one calibrated ``rm_threshold`` in
        either mode: under ``hparams.tta_mirror`` validation calibrates it on the averaged probabilities, and ``tta=False`` on such a
        checkpoint reuses it as it is.

        ``mc_samples``: None = ``hparams.mc_samples`` (default 1), else S in 1 .. 64.  S > 1 (``predict_map_mc``): the conv stack and
        ``fc1``'s Linear once, S dropout draws of the tail per scene from the module's own generator (reseeded from ``hparams.mc_seed``
        at every call: the same call gives the same map), and the mean of the S probabilities ``> threshold`` inside the head's
        kernel; with ``tta`` the mean of the two passes' S-draw means.  S = 1 is the single draw described above, call for call."""
        samples, mode = _mc.resolve(self, mc_samples), _tta.resolve(self, tta)
        if samples > 1:
            return predict_map_mc(self, self._pooled, x, threshold, mode, samples)
        if mode is None:
            return predict_map(self, lambda: self._encode(x), threshold)
        return predict_map_tta(self, self._encode, x, threshold)

    def _run_step(self, batch, batch_idx, step_name, keeps=(None, None), logits=None):
        """``logits``: ``(sample, keeps) -> logits`` of the rows the loss is taken on, in place of ``self._logits`` (the step with an
        unlabelled part: the first rows of a longer forward)."""
        sample, target, road_image = batch
        if logits is None:
            logits = self._logits
        logging = self.logger is not None and batch_idx % self.hparams.output_img_freq == 0
        per_sample = tuple(road_image)
        if (step_name == "train" and not logging and 0 < len(per_sample) <= ops.PTR_TABLE_MAX and
                all(t.is_cuda and t.is_contiguous() and t.dtype in (torch.bool, torch.uint8) and t.numel() % 4 == 0 for t in per_sample)):
            # the training step only needs the masks inside the loss: the kernel reads them where the collate left them
            # (a pointer table) instead of torch.stack-ing them first (roadmap_bce_v2.py:87)
            pred_rm = logits(sample, keeps)
            b = len(per_sample)
            loss, probs = self._loss_and_probs(pred_rm.reshape(b, -1), per_sample, train=True)
            return loss, None, pred_rm, probs.reshape(b, 800, 800)
        masks = torch.stack(per_sample, dim=0)            # bool as the dataset hands them over (data_helper.py:137-139)
        # self(sample) of the reference = (logits, probabilities); here the probabilities come out of the loss kernel's pass
        # over the logits (same values as forward()'s), which saves reading the 82 MB of logits a second time
        pred_rm = logits(sample, keeps)                  # names as in the reference: pred_rm = logits, pred_logit_rm = probabilities
        # the loss reads the bool masks as bytes; the fp32 copy (roadmap_bce_v2.py:87) is only made where it is looked at
        target_rm = masks.float() if (logging or step_name != "train" or masks.dtype.is_floating_point) else masks
        batch_size = masks.size(0)
        loss_target = masks if masks.dtype in (torch.bool, torch.uint8) else target_rm
        loss, probs = self._loss_and_probs(pred_rm.reshape(batch_size, -1), loss_target.reshape(batch_size, -1).contiguous(),
                                           train=step_name == "train")
        pred_logit_rm = probs.reshape(batch_size, 800, 800)
        if logging:
            self._log_rm_images(self.wide_stitch_six_images(sample), target_rm, pred_logit_rm, step_name)
        return loss, target_rm, pred_rm, pred_logit_rm

    def _loss_and_probs(self, logits, target, train=False):
        """(loss, sigmoid(logits)) of ``logits`` [B, P] from one pass: the reference's mean BCE-with-logits, or under an ``rm_*`` setting
        (``rm_loss_config``) the weighted BCE + soft threat score, whose two components are then kept in ``_rm_parts``; on the training
        step (``train``) under ``rm_topk_frac`` < 1 the BCE over each sample's K hardest pixels, whose figures are kept in ``_topk_parts``."""
        if train and self.topk is not None:
            return self._topk_loss_and_probs(logits, target)
        if self.rm_loss is None:
            return ops.BceWithLogitsProbs.apply(logits, target)
        loss, probs, self._rm_parts = road_map_loss_parts(self.rm_loss, logits, target)
        return loss, probs

    def _topk_loss_and_probs(self, logits, target):
        from . import topk_loss      # here, not at the top: a model with the setting off never imports or loads the library
        frac, warmup_steps = self.topk
        b, per = logits.shape
        keep = topk_loss.keep_now(frac, warmup_steps, self.topk_step, per)
        self.topk_step += 1
        loss, probs, stats = topk_loss.topk_bce(logits, target, keep)
        self._topk_parts = ((stats[:, 3].sum() / (b * per)).float(), (stats[:, 0].sum() / (b * per)).float(), stats[:, 2].mean().float())
        return loss, probs

    def _log_topk(self, log):
        if self.topk is not None:
            log["rm_bce_all"], log["rm_topk_kept"], log["rm_topk_tau"] = self._topk_parts
        return log

    def _log_rm_images(self, x, target_rm, pred_rm, step_name, limit=1):
        exp = self.logger.experiment
        step = self.trainer.global_step if self.trainer is not None else 0
        exp.add_image(f"{step_name}_input_images", x[:limit][0], step)
        exp.add_image(f"{step_name}_target_roadmaps", target_rm[:limit], step)
        exp.add_image(f"{step_name}_pred_roadmaps", pred_rm[:limit].round(), step)

    def training_step(self, batch, batch_idx):
        if self.current_epoch >= self.hparams.unfreeze_epoch_no and self.frozen:
            self.frozen = False
            self.ae.unfreeze()
        if len(batch) == 4:
            return self._consistency_step(batch, batch_idx)
        batch = self.augment.apply(batch)
        train_loss, _, _, _ = self._run_step(batch, batch_idx, step_name="train")
        log = {"train_loss": train_loss}
        if self.rm_loss is not None:
            log["rm_bce"], log["rm_soft_ts"] = self._rm_parts
        return {"loss": train_loss, "log": self._log_topk(log)}

    def _consistency_draw(self, b, mirror):
        """One draw of the model's ``Augmenter`` for ``b`` unlabelled scenes with the mirror bit cleared or set; with the augmenter
        disabled the identity colour and no other flag, and nothing is drawn from its generator."""
        if self.augment.enabled:
            flags, color = self.augment.draw(b)
        else:
            flags, color = torch.zeros(b, dtype=torch.int64), torch.tensor([1.0, 0.0]).repeat(b, 6, 1)
        return (flags & ~_augment.FLAG_MIRROR) | (_augment.FLAG_MIRROR if mirror else 0), color

    def _consistency_step(self, batch, batch_idx):
        """The training step on ``(sample, target, road_image, unlabelled)`` (the class docstring): ``unlabelled`` is ``B_u`` scenes in any
        form ``forward`` takes.  The labelled triple is augmented as in a supervised step; the unlabelled scenes become two stochastic
        views, one with the rig mirrored; all ``N = B_l + 2 B_u`` rows go through ONE ``_logits`` call.  The supervised loss reads rows
        ``[:B_l]``, ``MirrorConsistency`` rows ``[B_l:]``.  The log gains ``cons_loss``, ``cons_disagree`` -- the share of the unlabelled
        maps' pixels on which the two views fall on different sides of logit 0 -- and ``cons_weight_now``."""
        if self.cons is None:
            raise ValueError("RoadMapBCE.training_step: the batch carries unlabelled scenes (a 4-tuple) but hparams.cons_weight is 0 or absent")
        from . import consistency
        weight, rampup_steps = self.cons
        sample, target, road_image = self.augment.apply(tuple(batch[:3]))
        unlabelled = batch[3]
        b_u = unlabelled.shape[0] if isinstance(unlabelled, torch.Tensor) else len(unlabelled)
        views = _augment.augment_views(unlabelled, *self._consistency_draw(b_u, mirror=False))
        mirrored = _augment.augment_views(unlabelled, *self._consistency_draw(b_u, mirror=True))
        if ops.is_u8_frames(sample):      # one dtype for ops.sample_table: the identity draw moves a frame's values as the gather does
            b_l = sample.shape[0] if isinstance(sample, torch.Tensor) else len(sample)
            sample = _augment.augment_views(sample, torch.zeros(b_l, dtype=torch.int64), torch.tensor([1.0, 0.0]).repeat(b_l, 6, 1))
        rows = tuple(sample) + tuple(views) + tuple(mirrored)      # N per-sample fp32 [6,3,H,W]
        b_l = len(rows) - 2 * b_u
        rest = []

        def labelled_logits(x, keeps):
            z = self._logits(x, keeps)
            rest.append(z[b_l:])
            return z[:b_l]

        sup_loss, _, _, _ = self._run_step((rows, target, road_image), batch_idx, step_name="train", logits=labelled_logits)
        cons_loss, stats = consistency.mirror_consistency(rest[0], return_stats=True)
        now = weight * consistency.ramp(self.cons_step, rampup_steps)
        self.cons_step += 1
        train_loss = sup_loss + now * cons_loss
        log = {"train_loss": train_loss, "cons_loss": cons_loss.detach(), "cons_disagree": stats[:, 1].sum() / (b_u * rest[0][0].numel()),
               "cons_weight_now": now}
        if self.rm_loss is not None:
            log["rm_bce"], log["rm_soft_ts"] = self._rm_parts
        return {"loss": train_loss, "log": self._log_topk(log)}

    def validation_step(self, batch, batch_idx):
        """Under ``hparams.tta_mirror`` also a mirrored pass (``no_grad``) and ``val_ts_tta`` / ``val_ts_rounded_tta``, the scores of the
        averaged probabilities; ``ts_hist`` (``hparams.calibrate_threshold``) is then taken from those, so ``rm_threshold`` is
        calibrated in the mode the checkpoint predicts in.  ``val_loss``, ``val_ts`` and ``val_ts_rounded`` keep their meaning.  Under an
        ``rm_*`` setting ``val_loss`` is the composite loss and ``val_rm_bce`` / ``val_rm_soft_ts`` its two components; the scores and
        ``ts_hist`` read the loss pass's probabilities as before.

        Under ``hparams.mc_samples`` > 1 also one encoder pass in ``eval()`` mode (``no_grad``) whose tail is drawn S times per scene
        (generator reseeded from ``hparams.mc_seed``), and ``val_ts_mc`` / ``val_ts_rounded_mc``, the scores of the S-draw mean.  With
        ``hparams.tta_mirror`` as well, a mirrored pass of the same kind joins it and ``val_ts_tta`` / ``val_ts_rounded_tta`` are taken
        from the mean of the two S-draw means: what ``predict_road_map`` thresholds in that mode.  ``ts_hist`` reads the most-averaged
        probabilities.  With ``hparams.mc_uncertainty`` on top the same head pass also yields ``val_mc_entropy`` /
        ``val_mc_mi`` / ``val_mc_var``: the batch means of the scenes' mean predictive entropy, mutual information and variance of the
        draws (the unmirrored batch's); ``val_ts_mc`` keeps its bits."""
        val_loss, target_rm, pred_rm, pred_logit_rm = self._run_step(batch, batch_idx, step_name="valid")
        out = {"val_loss": val_loss, **road_map_scores(target_rm, pred_logit_rm)}
        if self.rm_loss is not None:
            out["val_rm_bce"], out["val_rm_soft_ts"] = self._rm_parts
        samples, mode = _mc.resolve(self, None), _tta.resolve(self, None)
        if samples > 1 and mc_uncertainty_config(self.hparams):
            return self._with_ts_hist(out, mc_validation_probs(self, out, target_rm, self._mc_probs_scored(out), batch[0], samples, mode), target_rm)
        if samples > 1:
            return self._with_ts_hist(out, mc_validation_probs(self, out, target_rm, self._mc_probs, batch[0], samples, mode), target_rm)
        if mode is None:
            return self._with_ts_hist(out, pred_logit_rm, target_rm)
        with torch.no_grad():
            avg = _tta.mean_prob(pred_rm.detach().contiguous(), self._logits(_tta.mirror_views(batch[0])), True)
        return self._with_ts_hist(tta_road_map_scores(out, target_rm, avg), avg, target_rm)

    def validation_epoch_end(self, outputs):
        avg = {k: torch.stack([x[k] for x in outputs]).mean() for k in ("val_loss", "val_ts", "val_ts_rounded")}
        logs = {"avg_val_loss": avg["val_loss"], "avg_val_ts_rounded": avg["val_ts_rounded"], "avg_val_ts": avg["val_ts"]}
        logs.update({"avg_" + k: torch.stack([x[k] for x in outputs]).mean() for k in TTA_ROAD_KEYS + MC_ROAD_KEYS + RM_LOSS_KEYS + VAL_UNCERTAINTY_KEYS
                     if outputs and all(k in x for x in outputs)})
        self._calibrate(outputs, logs)
        return {"val_loss": avg["val_loss"], "log": logs}

    def configure_optimizers(self):
        optimizer = torch.optim.Adam(self.parameters(), lr=self.hparams.learning_rate)
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, patience=10)
        return [optimizer], [scheduler]

    @staticmethod
    def add_model_specific_args(parent_parser):
        p = ArgumentParser(parents=[parent_parser], add_help=False)
        p.add_argument("--learning_rate", type=float, default=1e-3)
        p.add_argument("--unfreeze_epoch_no", type=int, default=0)
        p.add_argument("--batch_size", type=int, default=16)
        p.add_argument("--link", type=str, default="/scratch/ab8690/DLSP20Dataset/data")
        p.add_argument("--pretrained_path", type=str, default="")
        p.add_argument("--output_img_freq", type=int, default=500)
        p.add_argument("--calibrate_threshold", action="store_true",
                       help="validation also finds the threshold with the best data-set threat score (rm_threshold)")
        add_augment_args(p)
        _tta.add_tta_args(p)
        _mc.add_mc_args(p)
        add_ema_args(p)
        add_weight_decay_args(p)
        add_rm_loss_args(p)
        return p


class NotInherited:
    """A class attribute that takes a base class's method out of a subclass: looking ``name`` up on the subclass or on an instance of it
    raises AttributeError, as if it had never been there."""

    def __init__(self, name, owner):
        self.name, self.owner = name, owner

    def __get__(self, obj, cls):
        raise AttributeError(f"{cls.__name__} has no {self.name}: it is {self.owner}'s alone")


class RoadMap(RoadMapBCE):
    """MSE twin (roadmap_pretrain_ae.py): sigmoid inside ``forward``, ``mse_loss(target, pred)``, unfreeze at epoch 30.  Its loss is taken
    from the probabilities: the ``rm_*`` hparams select a loss on logits and are refused."""

    def __init__(self, hparams):
        super().__init__(hparams)
        if self.rm_loss is not None:
            raise ValueError("rm_pos_weight / rm_bce_weight / rm_ts_weight select a loss on the road-map head's logits; RoadMap (roadmap_mse) "
                             "trains on the MSE of its probabilities: use RoadMapBCE")
        refuse_consistency(hparams, "RoadMap (roadmap_mse)", "takes its loss from the probabilities and has no step for them")
        refuse_topk(hparams, "RoadMap (roadmap_mse)", "trains on the MSE of its probabilities")
        if mc_uncertainty_config(hparams):
            raise ValueError("mc_uncertainty asks for the draws' spread in validation, which is built into RoadMapBCE only: use RoadMapBCE")

    predict_uncertainty = NotInherited("predict_uncertainty", "RoadMapBCE")      # the uncertainty outputs are RoadMapBCE's alone

    def forward(self, x, keeps=(None, None)):
        """-> sigmoid(Linear(z)) [B,800,800], differentiable (roadmap_pretrain_ae.py:67-82)."""
        y = ops.Sigmoid.apply(ops.linear(self._encode(x, keeps), self.fc1.weight, self.fc1.bias))
        return y.reshape(y.size(0), 800, 800)

    def _run_step(self, batch, batch_idx, step_name, keeps=(None, None)):
        sample, target, road_image = batch
        target_rm = torch.stack(tuple(road_image), dim=0).float()
        pred_rm = self(sample, keeps)
        loss = ops.MseLoss.apply(pred_rm.contiguous(), target_rm)      # F.mse_loss(target_rm, pred_rm), roadmap_pretrain_ae.py:100
        return loss, target_rm, pred_rm

    def training_step(self, batch, batch_idx):
        if self.current_epoch >= 30 and self.frozen:          # roadmap_pretrain_ae.py:131
            self.frozen = False
            self.ae.unfreeze()
        batch = self.augment.apply(batch)
        train_loss, _, _ = self._run_step(batch, batch_idx, step_name="train")
        return {"loss": train_loss, "log": {"train_loss": train_loss}}

    def validation_step(self, batch, batch_idx):
        val_loss, target_rm, pred_rm = self._run_step(batch, batch_idx, step_name="valid")
        out = {"val_loss": val_loss, "val_ts": compute_ts_road_map(target_rm, pred_rm),
               "val_ts_rounded": ops.threat_score(target_rm.contiguous(), pred_rm.contiguous(), round_b=True)}
        samples, mode = _mc.resolve(self, None), _tta.resolve(self, None)
        if samples > 1:      # as RoadMapBCE's: the head's probabilities are this model's output too
            return self._with_ts_hist(out, mc_validation_probs(self, out, target_rm, self._mc_probs, batch[0], samples, mode), target_rm)
        if mode is None:
            return self._with_ts_hist(out, pred_rm, target_rm)
        with torch.no_grad():      # ``forward`` ends in the head's sigmoid here: the mean of the two PROBABILITIES, the same bits as from the logits
            avg = _tta.mean_prob(pred_rm.detach().contiguous(), self(_tta.mirror_views(batch[0])).contiguous(), False)
        return self._with_ts_hist(tta_road_map_scores(out, target_rm, avg), avg, target_rm)
