"""GPU tests of mirror test-time averaging in the models: ``predict_*`` against the composition written out from
public pieces, the exact equivariance that cannot hold without the feature, "off is the parent", and ``validation_step`` under
``hparams.tta_mirror``.  Every comparison is on raw bits.  Models as tests/_joint_cases.py builds them: hidden 16, latent 8, the
cameras' own 256 x 306, dropout off, B = 2."""
import math
import os
import sys
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _joint_cases as jc  # noqa: E402

from driving_dirty_amd import synth  # noqa: E402

B = 2
TAU = 0.47      # the filled head's probabilities straddle it (tests/_joint_cases.py: HEAD_GAIN)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import tta
    tta.lib()
    return torch.device("cuda:0")


def build(cls, dev, seed=29):
    from driving_dirty_amd.autoencoder import BasicAE
    model = cls(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=16, latent_dim=8)), unfreeze_epoch_no=0, **jc.HP))
    synth.fill_module(model, seed=seed)
    if hasattr(model, "fc1"):
        with torch.no_grad():
            model.fc1.weight.mul_(jc.HEAD_GAIN)
            model.fc1.bias.mul_(jc.HEAD_GAIN)
    model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0      # the reference's dropout is on in eval mode too
    return model.to(dev).eval()


@pytest.fixture(scope="module")
def data(dev):
    return jc.views_and_roads(dev, B)


@pytest.fixture(scope="module")
def road_model(dev):
    from driving_dirty_amd.roadmap import RoadMapBCE
    return build(RoadMapBCE, dev)


@pytest.fixture(scope="module")
def box_model(dev, data):
    """The untrained box head's map lies on one side of 0.5: its last bias is moved so that the map's median is 0.5."""
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    model = build(BBSpatialRoadMap, dev)
    views, road = data
    with torch.no_grad():
        m = float(model(tuple(views), tuple(road)).median())
        assert 0.0 < m < 1.0
        model.box_merge.up_conv_5.bias -= math.log(m / (1.0 - m))
    return model


@pytest.fixture(scope="module")
def joint_model(dev, data):
    model = jc.build_joint(dev).eval()
    views, road = data
    jc.centre_box_map(model, tuple(views), tuple(road))
    return model


def targets_from(*box_sets):
    """Targets whose cars are CHOSEN among the boxes each of the given decodings finds (six of the first, four of the second, two of
    the third, per sample), so that every decoding matches some target exactly and the scores are non-zero and differ: the decoding is
    what these tests are about."""
    take = (6, 4, 2)
    assert all(s[i].shape[0] >= n for s, n in zip(box_sets, take) for i in range(B))
    return tuple({"bounding_box": torch.cat([s[i][:n] for s, n in zip(box_sets, take)]).double().cpu()} for i in range(B))


def same_boxes(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want))


# ---- the compositions, from public pieces -------------------------------------------------------------------------------------------
def road_logits(model, x):
    from driving_dirty_amd.joint import JointRoadMapBBox
    with torch.no_grad():
        if isinstance(model, JointRoadMapBBox):
            return model._road_logits(model._features(x)[1])
        return model._logits(x)


def composed_road_map(model, x, tau):
    from driving_dirty_amd import tta
    return tta.mean_gt(road_logits(model, x), road_logits(model, tta.mirror_views(x)), tau, True)


def composed_box_map(model, x, rm):
    from driving_dirty_amd import tta
    from driving_dirty_amd.joint import JointRoadMapBBox
    pick = (lambda out: out[1]) if isinstance(model, JointRoadMapBBox) else (lambda out: out)
    with torch.no_grad():
        return tta.mean_prob(pick(model(x, rm)).contiguous(), pick(model(tta.mirror_views(x), tta.mirror_masks(rm))).contiguous(), False)


def composed_joint(model, x, tau):
    """-> (road map, averaged logits' probabilities, averaged camera-only box map), the construction of ``predict``."""
    from driving_dirty_amd import tta
    with torch.no_grad():
        feat, pooled, space = model._features(x)
        feat_m, pooled_m, space_m = model._features(tta.mirror_views(x))
        logits, logits_m = model._road_logits(pooled), model._road_logits(pooled_m)
        road = tta.mean_gt(logits, logits_m, tau, True)
        probs = model._box_branch(feat, space, tuple(road.unbind(0)))
        probs_m = model._box_branch(feat_m, space_m, tta.mirror_masks(road))
        return road, tta.mean_prob(logits, logits_m, True), tta.mean_prob(probs.contiguous(), probs_m.contiguous(), False)


# ---- composition --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["stacked", "tuple", "uint8"])
def test_road_map_prediction_is_the_composition(dev, data, road_model, joint_model, form):
    x = jc.input_forms(data[0])[form]
    for model in (road_model, joint_model):
        got = model.predict_road_map(x, TAU, tta="mirror")
        assert got.dtype == torch.bool and tuple(got.shape) == (B, 800, 800)
        assert torch.equal(got, composed_road_map(model, x, TAU))
        assert 0.05 < float(got.float().mean()) < 0.95, "both classes present"
        assert torch.equal(model.predict_road_map(x, TAU, tta=True), got)
        assert not torch.equal(got, model.predict_road_map(x, TAU, tta=False)), "the averaged map is another map"


@pytest.mark.parametrize("form", ["stacked", "tuple", "uint8"])
def test_box_prediction_with_a_given_road_map_is_the_composition(dev, data, box_model, joint_model, form):
    from driving_dirty_amd.spatial import boxes_from_map
    x = jc.input_forms(data[0])[form]
    road = data[1]
    for model in (box_model, joint_model):
        for rm in (tuple(road), road.float().unsqueeze(1)):      # the collate's bool masks; the fp32 [B,1,800,800] map
            got = model.predict_boxes(x, rm, tta="mirror")
            want = boxes_from_map(composed_box_map(model, x, rm), 0.5, 1)
            assert same_boxes(got, want) and sum(g.shape[0] for g in got) > 0
            assert not same_boxes(got, model.predict_boxes(x, rm, tta=False))


@pytest.mark.parametrize("form", ["stacked", "tuple", "uint8"])
def test_camera_only_prediction_is_the_composition(dev, data, joint_model, form):
    from driving_dirty_amd.spatial import boxes_from_map
    x = jc.input_forms(data[0])[form]
    got = joint_model.predict_mode(x, "mirror", TAU)
    road, _, box_map = composed_joint(joint_model, x, TAU)
    assert torch.equal(got.road_map, road) and same_boxes(got.boxes, boxes_from_map(box_map, 0.5, 1))
    assert sum(g.shape[0] for g in got.boxes) > 0
    assert same_boxes(joint_model.predict_boxes(x, tta="mirror"), joint_model.predict_mode(x, "mirror").boxes)


# ---- equivariance: cannot pass without the feature ----------------------------------------------------------------------------------
def test_the_averaged_prediction_of_the_mirrored_scene_is_the_row_reversed_prediction(dev, data, road_model, joint_model):
    from driving_dirty_amd import tta
    from driving_dirty_amd.spatial import boxes_from_map
    x = data[0]
    xm = tta.mirror_views(x)
    assert torch.equal(tta.mirror_views(xm).view(torch.int32), x.view(torch.int32)), "the mirror is an involution, bit for bit"
    for model in (road_model, joint_model):
        plain, plain_m = model.predict_road_map(x, TAU, tta=False), model.predict_road_map(xm, TAU, tta=False)
        assert not torch.equal(plain_m, plain.flip(1)), "the plain prediction of this untrained model is NOT equivariant"
        assert torch.equal(model.predict_road_map(xm, TAU, tta="mirror"), model.predict_road_map(x, TAU, tta="mirror").flip(1))
    road, _, box_map = composed_joint(joint_model, x, TAU)
    got = joint_model.predict_mode(xm, "mirror", TAU)
    assert torch.equal(got.road_map, road.flip(1))
    assert same_boxes(got.boxes, boxes_from_map(box_map.flip(1).contiguous(), 0.5, 1)) and sum(g.shape[0] for g in got.boxes) > 0
    off, off_m = joint_model.predict_mode(x, False, TAU), joint_model.predict_mode(xm, False, TAU)
    with torch.no_grad():
        feat, pooled, space = joint_model._features(x)
        plain_map = joint_model._box_branch(feat, space, tuple(off.road_map.unbind(0)))
    assert same_boxes(off.boxes, boxes_from_map(plain_map, 0.5, 1)), "the plain box map, as predict decodes it"
    assert not same_boxes(off_m.boxes, boxes_from_map(plain_map.flip(1).contiguous(), 0.5, 1)), "... whose boxes are NOT equivariant"


# ---- off is the parent ----------------------------------------------------------------------------------------------------------------
def test_off_launches_nothing_from_either_extension_and_the_flag_turns_it_on(dev, data, road_model, box_model, joint_model, monkeypatch):
    from driving_dirty_amd import augment, tta
    calls = []
    for mod in (tta, augment):
        real = mod.launch
        monkeypatch.setattr(mod, "launch", lambda name, *ops, _real=real: (calls.append(name), _real(name, *ops))[1])
    x, rm = data[0], tuple(data[1])
    predictions = {
        "road": lambda **kw: road_model.predict_road_map(x, TAU, **kw),
        "joint road": lambda **kw: joint_model.predict_road_map(x, TAU, **kw),
        "box": lambda **kw: box_model.predict_boxes(x, rm, **kw),
        "joint box": lambda **kw: joint_model.predict_boxes(x, rm, **kw),
        "joint camera-only box": lambda **kw: joint_model.predict_boxes(x, **kw),
    }
    models = {"road": road_model, "joint road": joint_model, "box": box_model, "joint box": joint_model, "joint camera-only box": joint_model}

    def same(p, q):
        return torch.equal(p, q) if isinstance(p, torch.Tensor) else same_boxes(p, q)

    for name, predict in predictions.items():
        del calls[:]
        default, off = predict(), predict(tta=False)
        assert not calls, (name, calls)
        assert same(default, off), name
        on = predict(tta="mirror")
        assert any(c.startswith("dd_tta_") for c in calls) and any(c.startswith("dd_aug_") for c in calls), (name, calls)
        assert not same(on, off), name
        model = models[name]
        model.hparams.tta_mirror = True
        try:
            assert same(predict(), on) and same(predict(tta=None), on) and same(predict(tta=False), off), name
        finally:
            del model.hparams.tta_mirror
    del calls[:]
    plain = joint_model.predict(x, TAU)
    assert not calls and torch.equal(plain.road_map, joint_model.predict_mode(x, False, TAU).road_map)
    joint_model.hparams.tta_mirror = True
    try:
        flagged = joint_model.predict(x, TAU)
    finally:
        del joint_model.hparams.tta_mirror
    want = joint_model.predict_mode(x, "mirror", TAU)
    assert torch.equal(flagged.road_map, want.road_map) and same_boxes(flagged.boxes, want.boxes)


# ---- validation under the flag ----------------------------------------------------------------------------------------------------------
def with_flags(model, **flags):
    class Flags:
        def __enter__(self):
            for k, v in flags.items():
                setattr(model.hparams, k, v)

        def __exit__(self, *exc):
            for k in flags:
                delattr(model.hparams, k)
    return Flags()


@pytest.mark.parametrize("name", ["RoadMapBCE", "RoadMap"])
def test_road_map_validation_under_the_flag(dev, data, name):
    from driving_dirty_amd import ops, roadmap, tta
    model = build(getattr(roadmap, name), dev)
    views, road = data
    batch = (tuple(views), None, tuple(road))
    with with_flags(model, calibrate_threshold=True):
        off = model.validation_step(batch, 0)
        with with_flags(model, tta_mirror=True):
            on = model.validation_step(batch, 0)
        log = model.validation_epoch_end([on, on])["log"]
    assert set(on) == set(off) | {"val_ts_tta", "val_ts_rounded_tta"} and "ts_hist" in off
    assert all(torch.equal(on[k], off[k]) for k in ("val_loss", "val_ts", "val_ts_rounded"))
    target = torch.stack(tuple(road)).float()
    with torch.no_grad():
        if name == "RoadMapBCE":
            avg = tta.mean_prob(model._logits(tuple(views)), model._logits(tta.mirror_views(tuple(views))), True)
        else:
            avg = tta.mean_prob(model(tuple(views)).contiguous(), model(tta.mirror_views(tuple(views))).contiguous(), False)
    assert torch.equal(on["val_ts_tta"], ops.threat_score(target, avg))
    assert torch.equal(on["val_ts_rounded_tta"], ops.threat_score(target, avg, round_b=True))
    assert torch.equal(on["ts_hist"], ops.ts_histogram(avg, target)) and not torch.equal(on["ts_hist"], off["ts_hist"])
    assert torch.equal(log["avg_val_ts_tta"], on["val_ts_tta"]) and "best_threshold" in log


def test_box_validation_under_the_flag(dev, data, box_model):
    from driving_dirty_amd import ops
    from driving_dirty_amd.spatial import decoded_box_ats
    model = box_model
    views, road = data
    targets = targets_from(model.predict_boxes(tuple(views), tuple(road), tta=False), model.predict_boxes(tuple(views), tuple(road), tta="mirror"))
    batch = (tuple(views), targets, tuple(road))
    with with_flags(model, box_metrics=True, calibrate_box_threshold=True):
        off = model.validation_step(batch, 0)
        with with_flags(model, tta_mirror=True):
            on = model.validation_step(batch, 0)
            swept = model._box_sweep_of(batch)
        box_map = composed_box_map(model, tuple(views), tuple(road))
        assert set(on) == set(off) | {"val_ats_tta", "val_ts_tta"}
        assert all(torch.equal(on[k], off[k]) for k in ("val_loss", "val_ats", "val_ts"))
        target_map = model.bb_coord_to_map(targets, dev).to(dev).float().reshape(B, -1)
        assert torch.equal(on["val_ats_tta"], decoded_box_ats(model.hparams, box_map, targets))
        assert float(on["val_ats_tta"]) > 0 and float(on["val_ats"]) > 0 and not torch.equal(on["val_ats_tta"], on["val_ats"])
        assert torch.equal(on["val_ts_tta"], ops.threat_score(target_map.contiguous(), box_map.reshape(B, -1), round_b=True))
        want = model._with_box_sweep({}, box_map, targets)[model.BOX_SWEEP]
        assert torch.equal(on[model.BOX_SWEEP], want) and torch.equal(swept[model.BOX_SWEEP], want)
        assert not torch.equal(on[model.BOX_SWEEP], off[model.BOX_SWEEP])


def test_joint_validation_under_the_flag(dev, data, joint_model):
    from driving_dirty_amd import ops
    from driving_dirty_amd.spatial import decoded_box_ats
    model = joint_model
    views, road = data
    x = tuple(views)
    targets = targets_from(model.predict_boxes(x, tuple(road), tta=False), model.predict_mode(x, False).boxes, model.predict_mode(x, "mirror").boxes)
    batch = (x, targets, tuple(road))
    with with_flags(model, box_metrics=True, calibrate_box_threshold=True, calibrate_threshold=True):
        off = model.validation_step(batch, 0)
        with with_flags(model, tta_mirror=True):
            on = model.validation_step(batch, 0)
            swept = model._box_sweep_of(batch)
        _, avg, box_map = composed_joint(model, tuple(views), 0.5)      # nothing calibrated: the reference's 0.5
        assert set(on) == set(off) | {"val_ts_tta", "val_ts_rounded_tta", "val_ats_tta"}
        unchanged = ("val_loss", "val_roadmap_loss", "val_bbox_loss", "val_ts", "val_ts_rounded", "val_ats_gt_rm", "val_ats", "val_box_ts")
        assert all(torch.equal(on[k], off[k]) for k in unchanged)
        target = torch.stack(tuple(road)).float()
        assert torch.equal(on["val_ts_tta"], ops.threat_score(target, avg))
        assert torch.equal(on["val_ts_rounded_tta"], ops.threat_score(target, avg, round_b=True))
        assert torch.equal(on["ts_hist"], ops.ts_histogram(avg, target)) and not torch.equal(on["ts_hist"], off["ts_hist"])
        assert torch.equal(on["val_ats_tta"], decoded_box_ats(model.hparams, box_map, targets))
        assert min(float(on[k]) for k in ("val_ats_tta", "val_ats", "val_ats_gt_rm")) > 0 and not torch.equal(on["val_ats_tta"], on["val_ats"])
        want = model._with_box_sweep({}, box_map, targets)[model.BOX_SWEEP]
        assert torch.equal(on[model.BOX_SWEEP], want) and torch.equal(swept[model.BOX_SWEEP], want)
        assert not torch.equal(on[model.BOX_SWEEP], off[model.BOX_SWEEP])
        log = model.validation_epoch_end([on, on])["log"]
        assert all("avg_" + k in log for k in ("val_ts_tta", "val_ts_rounded_tta", "val_ats_tta"))
    for k in ("rm_threshold", "box_threshold"):      # as built
        if hasattr(model.hparams, k):
            delattr(model.hparams, k)
