"""``JointRoadMapBBox``: BASELINE.json config 4, the joint roadmap + bounding-box multi-task step.

The reference has no joint model: its ``c3_only`` switch (components.py:44-45) makes the two heads mutually
exclusive users of the encoder.  This is a build-side composition of rows a8 + a11 of SURVEY.md 8(a): ONE pass of
the encoder conv stack feeds both the latent path (pool -> dense blocks -> Linear(64, 640000) -> BCE-with-logits,
roadmap_bce_v2.py:66-108) and the box path (SpatialMappingCNN + RoadMapBoxesMergingCNN -> BCE on probabilities,
spatial_w_rm.py:67-131); the losses add, the two gradients of the shared c3 feature add inside the encoder's
backward.  Parity is checked per head against the oracle (tests/test_gpu_heads.py).

Camera-only use.  The box head reads a road map (``rm_conv_1``).  ``forward(x, rm)`` and the default training
step hand it the ground truth, as the reference's box model does (spatial_w_rm.py:67-83); at test time there is none, and the
model's own road-map head supplies it: ``predict`` / ``predict_boxes(x)`` / ``validation_step``'s ``val_ats`` and, with
``hparams.box_rm_input = "predicted"``, the training step feed the head's thresholded map into the box branch
(``_own_road_masks`` states the rule).  All of it runs on the entry points the two heads already use.
"""
from argparse import ArgumentParser
from collections import namedtuple

import torch
from torch import nn

from . import mc as _mc
from . import ops
from . import tta as _tta
from .augment import Augmenter, add_augment_args, current_rank
from .adamw import add_weight_decay_args
from .ema import add_ema_args
from .autoencoder import BasicAE
from .lightning import LightningModule, hparam, pretrained_ae
from .roadmap import (MC_ROAD_KEYS, RM_LOSS_KEYS, TTA_ROAD_KEYS, CalibratedThreshold, add_rm_loss_args, eval_no_grad, mc_validation_probs,
                      predict_map, predict_map_mc, predict_map_tta, prediction_threshold, refuse_consistency, refuse_topk, rm_loss_config, road_map_loss_parts,
                      road_map_scores, tta_road_map_scores)
from .spatial import (HALF_UNLESS_CALIBRATED, ONE_UNLESS_CONFIGURED, CalibratedBoxThreshold, RoadMapBoxesMergingCNN, SpatialMappingCNN,
                      add_box_args, bb_coord_to_map, box_decode_point, box_loss_config, boxes_from_map, decoded_box_ats, mean_logs,
                      per_sample_inputs, require_bounding_boxes)

Prediction = namedtuple("Prediction", ("road_map", "boxes"))      # torch.bool [B,800,800], tuple of B tensors [n_i,2,4]


class JointRoadMapBBox(CalibratedThreshold, CalibratedBoxThreshold, LightningModule):
    box_loss = None      # spatial.box_loss_config(hparams): None = BCE on probabilities, as the reference's box model
    rm_loss = None       # roadmap.rm_loss_config(hparams): None = mean BCE-with-logits, as the reference's road-map model
    box_rm_input = "target"      # the road map the TRAINING step's box branch reads: "target" (ground truth) | "predicted" (the head's own)

    def __init__(self, hparams):
        super().__init__()
        self.hparams = hparams
        self.ae = pretrained_ae(hparams)
        self.ae.decoder = None
        self.ae.encoder.c3_only = False
        self.fc1 = nn.Linear(self.ae.latent_dim, 800 * 800)          # roadmap head, roadmap_bce_v2.py:50
        self.space_map_cnn = SpatialMappingCNN()                      # spatial_w_rm.py:50-52
        self.box_merge = RoadMapBoxesMergingCNN()
        precision = hparam(hparams, "precision", None)                # "fp32" (default) | "fp32x3": the box head's up-convs by split products
        if precision is not None:
            if precision not in ("fp32", "fp32x3"):
                raise ValueError(f"precision must be 'fp32' or 'fp32x3', got {precision!r}")
            self.box_merge.precision = precision
        self.box_loss = box_loss_config(hparams)      # None: BCE on probabilities as the reference's box model (spatial_w_rm.py:131)
        self.rm_loss = rm_loss_config(hparams)        # None: mean BCE-with-logits (roadmap_bce_v2.py:106)
        _mc.check_hparams(hparams)                    # mc_samples / mc_seed: the road map from S dropout draws of the tail (mc.py)
        refuse_consistency(hparams, "JointRoadMapBBox", "has a box branch that needs labels for every scene of the batch")
        refuse_topk(hparams, "JointRoadMapBBox", "takes its road-map loss in a step of its own, into which the selection is not built")
        self.box_rm_input = hparam(hparams, "box_rm_input", "target")
        if self.box_rm_input not in ("target", "predicted"):
            raise ValueError(f"box_rm_input must be 'target' or 'predicted', got {self.box_rm_input!r}")
        self._check_box_decode()
        self.augment = Augmenter(hparams, rank=current_rank())      # train-time only; off unless an aug_* hparam is set

    # ------------------------------------------------------------------------------------------------ the parts of one pass
    def _features(self, x):
        """x as ``forward`` takes it -> (conv feature [B,32,128,918] as an NCHW-shaped view, pooled vector for the encoder's tail,
        SpatialMappingCNN's map [B,32,256,256]): everything both heads share or that reads the cameras, once."""
        x = tuple(t.contiguous() for t in x) if isinstance(x, (tuple, list)) else x.contiguous()
        wide4 = ops.wide_image(x)                                     # fp32 views or uint8 frames, tensor or the collate's tuple
        feat, pooled = self.ae.encoder.conv_feature_and_pooled(wide4)
        return feat, pooled, self.space_map_cnn(x)

    def _box_branch(self, feat, space_rep, rm):
        """-> box probabilities [B,800,800].  ``rm``: [B,1,800,800] fp32, or a tuple of B bool / uint8 [800,800] masks."""
        return self.box_merge(feat, space_rep, rm).squeeze(1)

    def _road_logits(self, pooled):
        """The encoder's dense tail and the road-map head -> logits [B,800,800]."""
        z = self.ae.encoder._tail(pooled, (None, None))
        return ops.linear(z, self.fc1.weight, self.fc1.bias).reshape(-1, 800, 800)

    @staticmethod
    def _own_road_masks(values, tau, logits=False):
        """The road-map head's output as the masks the box branch reads: a tuple of B contiguous torch.bool [800,800] views, the form
        ``heads.road_map_taps`` gathers from through ``ops.subsample_masks_nhwc4`` (any B: that entry point cuts its pointer table
        into chunks of ``ops.PTR_TABLE_MAX`` itself, so nothing is chunked here).

        THE RULE, stated once: a pixel is road where the head's PROBABILITY is ``> tau``, strictly, ``tau`` rounded to fp32.  The
        probability is the dense head's one sigmoid (csrc/dd_device.h) of the fp32 logit: what ``ops.sigmoid`` returns, what the BCE
        pass returns beside the loss, and what ``ops.linear_sigmoid_gt`` compares inside the head's kernel -- the same bits, so
        ``predict``, ``validation_step`` and the self-fed training step draw the same map from the same logits.  ``values`` holds
        probabilities; with ``logits=True`` it holds logits and goes through ``ops.sigmoid`` first (never compared against
        ``logit(tau)``: that is a different rounding).  No gradient passes through the map."""
        probs = ops.sigmoid(values.detach().contiguous()) if logits else values.detach()
        return tuple((probs.reshape(-1, 800, 800) > float(tau)).unbind(0))

    def _own_tau(self):
        return prediction_threshold(self, None)      # the calibrated rm_threshold, else the reference's 0.5

    def forward(self, x, rm):
        """x [B,6,3,256,306], rm [B,1,800,800] -> (roadmap logits [B,800,800], box probabilities [B,800,800]).  Both may also be
        the collate's tuples (per-sample views, bool road masks), read through pointer tables."""
        feat, pooled, space_rep = self._features(x)
        # the box branch FIRST, the encoder's dense tail and the road-map head after it: autograd runs the newest nodes first, so
        # the two tensors that are 99.6 % of the data-parallel message (encoder fc1.fc1.weight 481 MB, head fc1.weight 164 MB) get
        # their gradients at the START of the backward and their reduction has the whole box-head backward (~40 ms) to hide under
        # instead of its last 5 (tools/step_phases.py); same arithmetic, same results
        boxes = self._box_branch(feat, space_rep, rm)
        return self._road_logits(pooled), boxes

    # ------------------------------------------------------------------------------------------------ prediction
    def _tta_maps(self, scene, mirrored, tau, from_logits=True):
        """Mirror test-time averaging of the camera-only construction (tta.py), from the parts of the two passes: ``scene`` and
        ``mirrored`` are each ``(feat, space_rep, road logits)`` -- or, with ``from_logits=False``, ``(feat, space_rep, road probabilities)``:
        the S-draw means of mc.py.  -> (road map torch.bool [B,800,800], averaged box map fp32
        [B,800,800]).  The road map is ``tta.mean_gt`` of the two logits at ``tau``; the scene's box branch reads it, the mirrored
        box branch reads ``tta.mirror_masks`` of it -- the map a mirrored training sample's box head was given -- and ``tta.mean_prob``
        brings the two box maps together."""
        (feat, space_rep, logits), (feat_m, space_rep_m, logits_m) = scene, mirrored
        road = _tta.mean_gt(logits.detach().contiguous(), logits_m.detach().contiguous(), tau, from_logits)
        probs = self._box_branch(feat, space_rep, tuple(road.unbind(0)))
        probs_m = self._box_branch(feat_m, space_rep_m, _tta.mirror_masks(road))
        return road, _tta.mean_prob(probs.detach().contiguous(), probs_m.detach().contiguous(), False)

    def _mirrored_parts(self, x):
        """``(feat, space_rep, road logits)`` of the mirrored scene: the same code as the scene's pass on ``tta.mirror_views(x)``."""
        feat_m, pooled_m, space_rep_m = self._features(_tta.mirror_views(x))
        return feat_m, space_rep_m, self._road_logits(pooled_m)

    def predict(self, x, threshold=None, box_threshold=HALF_UNLESS_CALIBRATED, min_pixels=ONE_UNLESS_CONFIGURED, max_boxes=256, fit="extent",
                pad_px=0.5, split_px=0, grow_iters=None):
        """What the task asks for, from the six cameras alone: ``Prediction(road_map, boxes)``, torch.bool [B,800,800] and a tuple of
        B tensors [n_i,2,4].  One encoder pass under ``no_grad`` in ``eval()`` mode (every submodule's mode is put back): the road
        map from ``ops.linear_sigmoid_gt`` at ``threshold`` (None: the calibrated ``rm_threshold``, else 0.5), that map into the box
        branch, the box map at ``box_threshold`` through ``boxes_from_map``.  ``box_threshold`` left out (or None): the calibrated
        ``box_threshold`` where there is one, else 0.5; ``min_pixels`` left out (or None): ``hparams.box_min_pixels``, else 1; a value the
        caller gives wins, 0.5 and 1 included (``spatial.box_decode_point``; the two defaults show what they fall back to).  ``x``:
        whatever ``forward`` takes.  The same kernels on the same inputs as ``predict_road_map(x)`` followed by
        ``predict_boxes(x, masks)``, minus the second encoder conv pass.

        Under ``hparams.tta_mirror`` (default off) the prediction is made with mirror test-time averaging, under ``hparams.mc_samples``
        > 1 from the mean of that many dropout draws per scene, which the box head then reads thresholded (``_predict_mc``).  This
        method's signature is pinned, so it follows the hparams; ``predict_mode`` is the same method with both as arguments.

        Mirror test-time averaging (``_tta_maps``): two passes at B -- the scene, and the same code on ``tta.mirror_views(x)`` -- the
        road map from the mean of the two heads' probabilities, the box map the mean of the two box branches' maps, each fed the road
        map in its own orientation.  The dense
        blocks' dropout is on in eval mode too, as in the reference, so the two passes also draw two dropout masks.  The thresholds
        left out are the one ``rm_threshold`` / ``box_threshold`` in either mode: under ``hparams.tta_mirror`` validation calibrates them
        on the averaged maps, and ``tta=False`` on such a checkpoint reuses them as they are."""
        return self.predict_mode(x, None, threshold, box_threshold, min_pixels, max_boxes, fit, pad_px, split_px, grow_iters)

    def _pooled(self, x):
        """The encoder's pooled vector alone (no box-branch inputs): what ``Encoder.latent_samples`` reads."""
        x = tuple(t.contiguous() for t in x) if isinstance(x, (tuple, list)) else x.contiguous()
        return self.ae.encoder.pooled_nhwc4(ops.wide_image(x))

    def _mc_probs(self, x, samples, gen):
        """Road-map probabilities [B,800,800] averaged over ``samples`` dropout draws per scene, masks from ``gen``; for ``eval_no_grad``."""
        return _mc.head_mean_prob(self, self.ae.encoder, self._pooled(x), samples, gen)

    def _predict_mc(self, x, mode, tau, samples):
        """``predict_mode``'s two maps under ``samples`` > 1 dropout draws per scene (mc.py) -> (road map, box map): the road map is the
        S-draw mean of the head's probabilities ``> tau`` -- one pass of the conv stack and of ``fc1``, S draws of the tail from the
        module's own generator, the mean inside the head's kernel -- and the box branch reads that averaged map.  Under the mirror
        ``mode`` each pass yields its S-draw mean and ``_tta_maps`` goes on from the two as it does from two logits."""
        gen = _mc.generator(self, self.fc1.weight.device)
        enc = self.ae.encoder
        feat, pooled, space_rep = self._features(x)
        if mode is None:
            road = _mc.head_mean_gt(self, enc, pooled, samples, gen, tau)
            return road, self._box_branch(feat, space_rep, tuple(road.unbind(0)))
        probs = _mc.head_mean_prob(self, enc, pooled, samples, gen)
        feat_m, pooled_m, space_rep_m = self._features(_tta.mirror_views(x))
        probs_m = _mc.head_mean_prob(self, enc, pooled_m, samples, gen)
        return self._tta_maps((feat, space_rep, probs), (feat_m, space_rep_m, probs_m), tau, from_logits=False)

    def predict_mode(self, x, tta=None, threshold=None, box_threshold=HALF_UNLESS_CALIBRATED, min_pixels=ONE_UNLESS_CONFIGURED, max_boxes=256,
                     fit="extent", pad_px=0.5, split_px=0, grow_iters=None, mc_samples=None):
        """``predict`` with the averaging mode as an argument: ``tta`` None = ``hparams.tta_mirror`` (what ``predict`` does), False = off,
        True / "mirror" = mirror test-time averaging; ``mc_samples`` None = ``hparams.mc_samples`` (what ``predict`` does), else the number
        of dropout draws per scene the road map is averaged over (``_predict_mc``; 1 = a single draw, the calls below).  Everything else
        as ``predict``'s."""
        tau = prediction_threshold(self, threshold)
        box_threshold, min_pixels = box_decode_point(self.hparams, box_threshold, min_pixels)
        samples = _mc.resolve(self, mc_samples)
        if samples > 1:
            with eval_no_grad(self):
                road, probs = self._predict_mc(x, _tta.resolve(self, tta), tau, samples)
                boxes = boxes_from_map(probs, box_threshold, min_pixels, max_boxes, fit, pad_px, split_px, grow_iters)
            return Prediction(road, boxes)
        if _tta.resolve(self, tta) is not None:
            with eval_no_grad(self):
                feat, pooled, space_rep = self._features(x)
                road, probs = self._tta_maps((feat, space_rep, self._road_logits(pooled)), self._mirrored_parts(x), tau)
                boxes = boxes_from_map(probs, box_threshold, min_pixels, max_boxes, fit, pad_px, split_px, grow_iters)
            return Prediction(road, boxes)
        with eval_no_grad(self):
            feat, pooled, space_rep = self._features(x)
            z = self.ae.encoder._tail(pooled, (None, None))
            road = ops.linear_sigmoid_gt(z, self.fc1.weight, self.fc1.bias, tau).reshape(-1, 800, 800)
            probs = self._box_branch(feat, space_rep, tuple(road.unbind(0)))
            boxes = boxes_from_map(probs, box_threshold, min_pixels, max_boxes, fit, pad_px, split_px, grow_iters)
        return Prediction(road, boxes)

    def predict_boxes(self, x, rm=None, threshold=None, min_pixels=None, max_boxes=256, fit="extent", pad_px=0.5, split_px=0, grow_iters=None,
                      tta=None):
        """The box head's map as boxes, as ``BBSpatialRoadMap.predict_boxes``: a tuple of B tensors [n_i,2,4].  ``rm=None``: camera-only,
        the boxes of ``predict`` (the head's own road map at its calibrated threshold); a given ``rm`` is used as it is.
        ``threshold=None`` / ``min_pixels=None``: the calibrated ``box_threshold``, else 0.5 / ``hparams.box_min_pixels``, else 1.
        ``tta``: as ``predict``'s; with a given ``rm`` as ``BBSpatialRoadMap.predict_boxes``'s: the mean of ``self(x, rm)``'s box map and
        of the one of ``tta.mirror_views(x)`` with ``tta.mirror_masks(rm)``, in ``eval()`` mode."""
        if rm is None:
            return self.predict_mode(x, tta, None, threshold, min_pixels, max_boxes, fit, pad_px, split_px, grow_iters).boxes
        threshold, min_pixels = box_decode_point(self.hparams, threshold, min_pixels)
        if _tta.resolve(self, tta) is not None:
            with eval_no_grad(self):
                probs = _tta.mean_prob(self(x, rm)[1].detach().contiguous(),
                                       self(_tta.mirror_views(x), _tta.mirror_masks(rm))[1].detach().contiguous(), False)
                return boxes_from_map(probs, threshold, min_pixels, max_boxes, fit, pad_px, split_px, grow_iters)
        with torch.no_grad():
            return boxes_from_map(self(x, rm)[1], threshold, min_pixels, max_boxes, fit, pad_px, split_px, grow_iters)

    def predict_road_map(self, x, threshold=None, mc_samples=None, tta=None):
        """The road-map branch as a boolean map, as ``RoadMapBCE.predict_road_map`` (``tta`` and ``mc_samples`` included): torch.bool
        [B,800,800]; the box branch is not run."""
        views = tuple(t.contiguous() for t in x) if isinstance(x, (tuple, list)) else x.contiguous()
        samples = _mc.resolve(self, mc_samples)
        if samples > 1:
            return predict_map_mc(self, self._pooled, views, threshold, _tta.resolve(self, tta), samples)
        if _tta.resolve(self, tta) is not None:
            return predict_map_tta(self, lambda v: self.ae.encoder.forward_nhwc4(ops.wide_image(v)), views, threshold)
        return predict_map(self, lambda: self.ae.encoder.forward_nhwc4(ops.wide_image(views)), threshold)

    # ------------------------------------------------------------------------------------------------ the steps
    @staticmethod
    def _step_inputs(sample, road_image):
        """A batch's views and road masks -> (x, rm, target_rm, per_sample).  ``per_sample``: the collate's tuples are read where they
        lie (roadmap_bce_v2.py:87 / spatial_w_rm.py:100-105 without the stacks; ``target_rm`` is None then); else a stacked tensor of
        views, rm [b,1,800,800] fp32 and target_rm [b,800,800]."""
        per_sample = (per_sample_inputs(sample, road_image) and all(t.numel() % 4 == 0 for t in road_image)
                      and len(road_image) <= ops.PTR_TABLE_MAX)
        if per_sample:
            return tuple(sample), tuple(road_image), None, True
        sample = torch.stack(tuple(sample), dim=0) if isinstance(sample, (tuple, list)) else sample
        target_rm = torch.stack(tuple(road_image), dim=0).float()
        return sample, target_rm.unsqueeze(1), target_rm, False

    def _camera_only_box_map(self, feat, space_rep, values, logits=False):
        """The box map [B,800,800] as ``predict`` computes it: the box branch fed the road-map head's own map (``_own_road_masks`` of
        ``values`` at ``rm_threshold``, else 0.5), contiguous."""
        return self._box_branch(feat, space_rep, self._own_road_masks(values, self._own_tau(), logits)).contiguous()

    def _box_sweep_of(self, batch):
        sample, target, road_image = batch
        require_bounding_boxes(target)
        x = self._step_inputs(sample, road_image)[0]
        feat, pooled, space_rep = self._features(x)
        if _tta.resolve(self, None) is not None:      # the averaged box map: the one ``predict`` decodes in this mode
            return self._with_box_sweep({}, self._tta_maps((feat, space_rep, self._road_logits(pooled)), self._mirrored_parts(x), self._own_tau())[1], target)
        return self._with_box_sweep({}, self._camera_only_box_map(feat, space_rep, self._road_logits(pooled), logits=True), target)

    def _run_step(self, batch, own_rm, want_probs):
        """One pass over a batch -> a dict: both losses (``loss_rm``, ``loss_bb``, the class-balanced loss's ``parts`` or None), the
        tensors validation scores (``logits``, ``boxes``, ``target_bb`` [b,800,800], ``probs`` when ``want_probs``) and what a second
        box-branch call needs (``feat``, ``space_rep``).  ``own_rm``: the box branch reads the head's own map instead of the batch's."""
        sample, target, road_image = batch
        sample, rm, target_rm, per_sample = self._step_inputs(sample, road_image)
        dev = sample[0].device if per_sample else sample.device
        b = len(road_image)
        target_bb = bb_coord_to_map(target, dev).to(dev).float()
        feat, pooled, space_rep = self._features(sample)
        if own_rm:
            logits = self._road_logits(pooled)
            boxes = self._box_branch(feat, space_rep, self._own_road_masks(logits, self._own_tau(), logits=True))
        else:
            boxes = self._box_branch(feat, space_rep, rm)      # first: see forward
            logits = self._road_logits(pooled)
        probs, rm_parts = None, None
        if self.rm_loss is not None:      # weighted BCE-with-logits + soft threat score; its pass writes the probabilities in either form
            loss_rm, probs, rm_parts = road_map_loss_parts(self.rm_loss, logits.reshape(b, -1), rm if per_sample else target_rm.reshape(b, -1))
        elif per_sample:
            loss_rm, probs = ops.BceWithLogitsProbs.apply(logits.reshape(b, -1), rm)
        else:
            loss_rm = ops.BceWithLogits.apply(logits.reshape(b, -1), target_rm.reshape(b, -1))
            if want_probs:
                probs = ops.sigmoid(logits.detach())
        parts = None
        if self.box_loss is not None:
            loss_bb, *parts = ops.box_loss(boxes.reshape(b, -1), target_bb.reshape(b, -1).contiguous(), return_parts=True, **self.box_loss)
        else:
            loss_bb = ops.BceProbs.apply(boxes.reshape(b, -1), target_bb.reshape(b, -1))
        return {"b": b, "loss_rm": loss_rm, "loss_bb": loss_bb, "parts": parts, "rm_parts": rm_parts, "logits": logits, "boxes": boxes, "target_bb": target_bb,
                "probs": None if probs is None else probs.detach().reshape(b, 800, 800), "feat": feat, "space_rep": space_rep, "sample": sample}

    def training_step(self, batch, batch_idx):
        """``hparams.box_rm_input = "target"`` (the default): the box branch reads the batch's road map, the step the reference's two
        models add up to.  ``"predicted"``: it reads the head's own map at ``rm_threshold`` (else 0.5), cut from the detached logits of
        this very pass, so the box head trains on the input it gets at test time; the road-map loss still uses the ground truth and
        no gradient of the box loss reaches the road-map head through the map.  The logits have to exist before the box branch
        then, so the autograd order of the two branches SWAPS: the box head's backward runs first and the two big Linear gradients
        (``forward`` says why they come first by default) finish late in the backward, with little left to hide their reduction
        under in data-parallel training."""
        batch = self.augment.apply(batch)
        s = self._run_step(batch, self.box_rm_input == "predicted", False)
        log = {}
        if s["parts"] is not None:
            log["bbox_bce"], log["bbox_soft_ts"] = s["parts"]
        if s["rm_parts"] is not None:
            log["rm_bce"], log["rm_soft_ts"] = s["rm_parts"]
        loss = s["loss_rm"] + s["loss_bb"]
        return {"loss": loss, "log": {"train_loss": loss, "roadmap_loss": s["loss_rm"], "bbox_loss": s["loss_bb"], **log}}

    def validation_step(self, batch, batch_idx):
        """One encoder pass, one road-map head pass.  Always: ``val_loss`` = ``val_roadmap_loss`` + ``val_bbox_loss`` (the training
        step's losses; ``val_bce`` / ``val_soft_ts`` with the class-balanced box loss, ``val_rm_bce`` / ``val_rm_soft_ts`` under an ``rm_*`` setting), the road map's ``val_ts`` / ``val_ts_rounded`` as
        ``RoadMapBCE`` reports them, ``ts_hist`` under ``hparams.calibrate_threshold``.  Under ``hparams.box_metrics`` also
        ``val_ats_gt_rm`` (boxes decoded from the box map computed WITH the ground-truth road map), ``val_ats`` (the honest one: a
        second box-branch call fed the head's own map of this pass, at ``rm_threshold`` or 0.5) and ``val_box_ts`` (the rounded
        map-level threat score of that camera-only box map); both decode at the calibrated ``box_threshold`` once there is one.  Under
        ``hparams.calibrate_box_threshold`` also ``box_ats_sweep``: that same camera-only box map, the one ``predict`` decodes, decoded and
        scored at every threshold of the grid.  With both calibrations on, an epoch's sweep is made of maps computed with the
        ``rm_threshold`` found at the end of the PREVIOUS epoch (0.5 in the first): the two operating points are not iterated to a joint
        optimum; the box threshold found is the best one for the road map the model had during that epoch.

        Under ``hparams.tta_mirror`` also one pass over the mirrored batch (``no_grad``): the road map's ``val_ts_tta`` /
        ``val_ts_rounded_tta`` from the averaged probabilities, which ``ts_hist`` is then taken from; under ``hparams.box_metrics``
        ``val_ats_tta``, camera-only, the construction of ``predict`` in this mode (``_tta_maps``) with the features of both passes
        reused; and ``box_ats_sweep`` reads that averaged box map.  Every other key keeps its meaning.

        Under ``hparams.mc_samples`` > 1 also one encoder pass in ``eval()`` mode whose tail is drawn S times per scene: ``val_ts_mc`` /
        ``val_ts_rounded_mc`` from the S-draw mean (with the mirror, ``val_ts_tta`` / ``val_ts_rounded_tta`` from the mean of the two
        passes' S-draw means), and ``ts_hist`` from the most-averaged probabilities, so ``rm_threshold`` is calibrated in the mode
        ``predict`` runs in.  The box keys (``val_ats*``, ``box_ats_sweep``) go on reading the single-draw pass's road map."""
        sample, target, road_image = batch
        s = self._run_step(batch, False, True)
        out = {"val_loss": s["loss_rm"] + s["loss_bb"], "val_roadmap_loss": s["loss_rm"], "val_bbox_loss": s["loss_bb"]}
        if s["parts"] is not None:
            out["val_bce"], out["val_soft_ts"] = s["parts"]
        if s["rm_parts"] is not None:
            out["val_rm_bce"], out["val_rm_soft_ts"] = s["rm_parts"]
        target_rm = torch.stack(tuple(road_image), dim=0).float()
        out.update(road_map_scores(target_rm, s["probs"]))
        mode, samples = _tta.resolve(self, None), _mc.resolve(self, None)
        averaged = mode is not None
        if averaged:
            with torch.no_grad():
                mirrored = self._mirrored_parts(s["sample"])
        if samples > 1:      # val_ts_mc / val_ts_rounded_mc; under the mirror the _tta keys from the two S-draw means; ts_hist from the most-averaged
            self._with_ts_hist(out, mc_validation_probs(self, out, target_rm, self._mc_probs, s["sample"], samples, mode), target_rm)
        elif averaged:
            with torch.no_grad():
                avg = _tta.mean_prob(s["logits"].detach().contiguous(), mirrored[2].detach().contiguous(), True)
            self._with_ts_hist(tta_road_map_scores(out, target_rm, avg), avg, target_rm)
        else:
            self._with_ts_hist(out, s["probs"], target_rm)
        box_metrics, sweep = hparam(self.hparams, "box_metrics", False), self._wants_box_sweep()
        if box_metrics or sweep:
            with torch.no_grad():
                require_bounding_boxes(target)
                if box_metrics or not averaged:
                    own = self._camera_only_box_map(s["feat"], s["space_rep"], s["probs"])      # once, for whichever asks
                if box_metrics:
                    out["val_ats_gt_rm"] = decoded_box_ats(self.hparams, s["boxes"].detach().contiguous(), target)
                    out["val_ats"] = decoded_box_ats(self.hparams, own, target)
                    out["val_box_ts"] = ops.threat_score(s["target_bb"].contiguous(), own, round_b=True)
                own_avg = self._tta_maps((s["feat"], s["space_rep"], s["logits"]), mirrored, self._own_tau())[1] if averaged else None
                if box_metrics and averaged:
                    out["val_ats_tta"] = decoded_box_ats(self.hparams, own_avg, target)
                if sweep:
                    self._with_box_sweep(out, own_avg if averaged else own, target)
        return out

    def validation_epoch_end(self, outputs):
        """The mean of every per-batch value as ``avg_*``; ``val_loss`` is the monitored value; under ``hparams.calibrate_threshold``
        ``rm_threshold`` is set from the epoch's summed histogram, as in ``RoadMapBCE``."""
        keys = ("val_loss", "val_roadmap_loss", "val_bbox_loss", "val_bce", "val_soft_ts", "val_ts", "val_ts_rounded", "val_ats_gt_rm",
                "val_ats", "val_box_ts", "val_ats_tta") + TTA_ROAD_KEYS + MC_ROAD_KEYS + RM_LOSS_KEYS
        logs = mean_logs(outputs, keys)
        self._calibrate(outputs, logs)
        if self._wants_box_sweep():
            self._calibrate_boxes(outputs, logs)      # sets box_threshold (spatial.CalibratedBoxThreshold)
        return {"val_loss": logs["avg_val_loss"], "log": logs}

    def configure_optimizers(self):
        return torch.optim.Adam(self.parameters(), lr=self.hparams.learning_rate)

    @staticmethod
    def add_model_specific_args(parent_parser):
        p = ArgumentParser(parents=[parent_parser], add_help=False)
        p.add_argument("--learning_rate", type=float, default=1e-3)
        p.add_argument("--batch_size", type=int, default=16)
        p.add_argument("--calibrate_threshold", action="store_true",
                       help="validation also finds the road-map threshold with the best data-set threat score (rm_threshold)")
        add_box_args(p)
        p.add_argument("--box_rm_input", type=str, default="target", choices=("target", "predicted"),
                       help="the road map the box head reads in TRAINING: the ground truth (the reference's step), or the road-map head's "
                            "own thresholded map, as at test time")
        p.add_argument("--link", type=str, default="/scratch/ab8690/DLSP20Dataset/data")
        p.add_argument("--pretrained_path", type=str, default="")
        p.add_argument("--output_img_freq", type=int, default=500)
        p.add_argument("--precision", type=str, default="fp32", choices=("fp32", "fp32x3"),
                       help="fp32: the reference's arithmetic; fp32x3: the box head's dilated up-convs as six bf16 products per fp32 product")
        add_augment_args(p)
        _tta.add_tta_args(p)
        _mc.add_mc_args(p)
        add_ema_args(p)
        add_weight_decay_args(p)
        add_rm_loss_args(p)
        return p
