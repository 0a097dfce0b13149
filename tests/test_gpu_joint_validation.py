"""GPU tests of ``JointRoadMapBBox.validation_step``: the training step's losses, the road map's scores, and under ``box_metrics`` the box
score twice -- with the ground-truth road map (``val_ats_gt_rm``) and from the cameras alone (``val_ats``)."""
import copy
import os
import sys
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _joint_cases as jc  # noqa: E402

ALWAYS = {"val_loss", "val_roadmap_loss", "val_bbox_loss", "val_ts", "val_ts_rounded"}
BOX = {"val_ats_gt_rm", "val_ats", "val_box_ts"}
ON = dict(box_pos_weight="auto", box_ts_weight=1.0)
B = 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def not_in(boxes, others):
    """The boxes of ``boxes`` [n,2,4] that are no box of ``others`` [m,2,4]."""
    same = (boxes.reshape(-1, 1, 8) == others.reshape(1, -1, 8)).all(dim=2).any(dim=1)
    return boxes[~same]


@pytest.fixture(scope="module")
def case(dev):
    """(model, batch, decoded-with-the-target-map boxes, camera-only boxes).  The targets' cars are CHOSEN so that both box scores mean
    something: six boxes that only the decoding with the ground-truth road map finds and three that only the camera-only decoding
    finds, per sample -- each decoding then matches its own (IoU 1) and the two scores are non-zero and differ."""
    model = jc.build_joint(dev)
    model.eval()
    views, road = jc.views_and_roads(dev, B)
    x, rm = tuple(views), tuple(road)
    jc.centre_box_map(model, x, rm)
    with_gt = model.predict_boxes(x, rm)
    own = model.predict(x).boxes
    targets = []
    for g, o in zip(with_gt, own):
        only_g, only_o = not_in(g, o), not_in(o, g)
        assert only_g.shape[0] >= 6 and only_o.shape[0] >= 3, (g.shape, o.shape, only_g.shape, only_o.shape)
        targets.append({"bounding_box": torch.cat([only_g[:6], only_o[:3]]).double().cpu()})
    return model, (x, tuple(targets), rm), with_gt, own


def test_key_sets_are_exact(dev, case):
    from driving_dirty_amd.spatial import box_loss_config
    model, batch, _, _ = case
    try:
        for box_metrics in (False, True):
            for calibrate in (False, True):
                for loss in (None, box_loss_config(Namespace(**ON))):
                    model.hparams.box_metrics, model.hparams.calibrate_threshold, model.box_loss = box_metrics, calibrate, loss
                    out = model.validation_step(batch, 0)
                    want = ALWAYS | (BOX if box_metrics else set()) | ({"ts_hist"} if calibrate else set()) | \
                        ({"val_bce", "val_soft_ts"} if loss else set())
                    assert set(out) == want, (box_metrics, calibrate, loss is not None)
                    assert all(v.dim() == 0 for k, v in out.items() if k != "ts_hist")
                    assert torch.equal(out["val_loss"], out["val_roadmap_loss"] + out["val_bbox_loss"])
                    end = model.validation_epoch_end([out, out])
                    assert {"avg_" + k for k in want - {"ts_hist"}} <= set(end["log"]) and torch.equal(end["val_loss"], out["val_loss"])
    finally:
        model.hparams.box_metrics = model.hparams.calibrate_threshold = False
        model.box_loss = None
        model.rm_threshold = None
    del model.hparams.rm_threshold      # as built


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("balanced", [False, True])
def test_losses_are_the_training_steps(dev, case, mode, balanced):
    from driving_dirty_amd.spatial import box_loss_config
    model, batch, _, _ = case
    state = copy.deepcopy(model.state_dict())      # train mode moves BatchNorm's running statistics: the other tests get the model back as it was
    try:
        model.box_loss = box_loss_config(Namespace(**ON)) if balanced else None
        getattr(model, mode)()
        with torch.no_grad():
            log = model.training_step(batch, 0)["log"]
            out = model.validation_step(batch, 0)
        assert torch.equal(out["val_roadmap_loss"], log["roadmap_loss"]) and torch.equal(out["val_bbox_loss"], log["bbox_loss"])
        assert torch.equal(out["val_loss"], log["train_loss"])
        assert float(out["val_roadmap_loss"]) > 0 and float(out["val_bbox_loss"]) > 0
        if balanced:
            assert torch.equal(out["val_bce"], log["bbox_bce"]) and torch.equal(out["val_soft_ts"], log["bbox_soft_ts"])
    finally:
        model.box_loss = None
        model.eval()
        model.load_state_dict(state)


@pytest.mark.parametrize("form", ["tuple", "stacked"])
def test_road_map_scores_are_forwards(dev, case, form):
    """In both forms of the batch: the collate's tuples (read where they lie) and a stacked tensor of views (the fallback path)."""
    from driving_dirty_amd import ops
    model, (x, targets, rm), _, _ = case
    sample = x if form == "tuple" else torch.stack(x)
    model.hparams.calibrate_threshold = True
    try:
        out = model.validation_step((sample, targets, rm), 0)
    finally:
        model.hparams.calibrate_threshold = False
    with torch.no_grad():
        logits, _ = model(sample, rm)
    probs, target = ops.sigmoid(logits), torch.stack(rm).float()
    assert torch.equal(out["val_ts"], ops.threat_score(target, probs))
    assert torch.equal(out["val_ts_rounded"], ops.threat_score(target, probs, round_b=True))
    assert 0 < float(out["val_ts_rounded"]) < 1
    assert torch.equal(out["ts_hist"], ops.ts_histogram(probs, target))


def test_box_scores_with_and_without_the_target_map(dev, case):
    from driving_dirty_amd import ops
    from driving_dirty_amd.spatial import bb_coord_to_map
    model, batch, with_gt, own = case
    x, targets, rm = batch
    boxes = [t["bounding_box"] for t in targets]
    model.hparams.box_metrics = True
    try:
        out = model.validation_step(batch, 0)
        want_gt = ops.ats_bounding_boxes(model.predict_boxes(x, rm), boxes).mean()
        want_own = ops.ats_bounding_boxes(model.predict(x).boxes, boxes).mean()
        print(f"val_ats_gt_rm {float(out['val_ats_gt_rm']):.6f}  val_ats {float(out['val_ats']):.6f}  val_box_ts {float(out['val_box_ts']):.6f}; "
              f"boxes per sample with the target map {[t.shape[0] for t in with_gt]}, camera-only {[t.shape[0] for t in own]}")
        assert torch.equal(out["val_ats_gt_rm"], want_gt) and torch.equal(out["val_ats"], want_own)
        assert float(out["val_ats_gt_rm"]) > 0 and float(out["val_ats"]) > 0 and float(out["val_ats_gt_rm"]) != float(out["val_ats"])
        with torch.no_grad():
            own_map = model(x, tuple(model.predict_road_map(x)))[1]
        assert torch.equal(out["val_box_ts"], ops.threat_score(bb_coord_to_map(targets, dev).float(), own_map.contiguous(), round_b=True))
        # the decoding follows the hparams, in both scores
        model.hparams.box_fit, model.hparams.box_pad_px = "oriented", 0.25
        fitted = model.validation_step(batch, 0)
        kw = dict(fit="oriented", pad_px=0.25)
        assert torch.equal(fitted["val_ats_gt_rm"], ops.ats_bounding_boxes(model.predict_boxes(x, rm, **kw), boxes).mean())
        assert torch.equal(fitted["val_ats"], ops.ats_bounding_boxes(model.predict(x, **kw).boxes, boxes).mean())
        assert torch.equal(fitted["val_box_ts"], out["val_box_ts"]) and torch.equal(fitted["val_loss"], out["val_loss"])
        # the camera-only map is cut at the calibrated threshold
        model.rm_threshold = 0.3
        assert not torch.equal(model.predict_road_map(x), model.predict_road_map(x, 0.5))
        moved = model.validation_step(batch, 0)
        assert torch.equal(moved["val_ats"], ops.ats_bounding_boxes(model.predict(x, **kw).boxes, boxes).mean())
        assert torch.equal(moved["val_ats_gt_rm"], fitted["val_ats_gt_rm"])
    finally:
        model.hparams.box_metrics = False
        for k in ("box_fit", "box_pad_px", "rm_threshold"):
            if hasattr(model.hparams, k):
                delattr(model.hparams, k)


def test_a_target_without_boxes_is_refused(dev, case):
    model, (x, targets, rm), _, _ = case
    maps = torch.zeros(B, 800, 800, device=dev)
    no_boxes = ({"bb_map": maps[0], "bounding_box": targets[0]["bounding_box"]}, {"bb_map": maps[1]})
    out = model.validation_step((x, no_boxes, rm), 0)      # not asked for boxes: fine
    assert set(out) == ALWAYS
    model.hparams.box_metrics = True
    try:
        with pytest.raises(KeyError, match=r"box_metrics needs a 'bounding_box' tensor in every target \(missing in samples \[1\]\)"):
            model.validation_step((x, no_boxes, rm), 0)
    finally:
        model.hparams.box_metrics = False
