"""GPU tests of ``JointRoadMapBBox.predict``: the road map and the boxes from the cameras alone, in one encoder pass, equal to what the
two-call composition ``predict_road_map`` -> ``predict_boxes(x, masks)`` gives."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _joint_cases as jc  # noqa: E402
import _predict_cases as pc  # noqa: E402

CAP = 4096      # max_boxes of the decoding at the map's median: an untrained head's map is noise


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return jc.build_joint(dev)


def same_boxes(a, b):
    return len(a) == len(b) and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("form,b", [("stacked", 2), ("tuple", 3), ("uint8", 2)])
def test_predict_is_the_two_calls_in_one_pass(dev, model, form, b):
    from driving_dirty_amd import ops
    from driving_dirty_amd.joint import Prediction
    views, _ = jc.views_and_roads(dev, b, seed=21)
    x = jc.input_forms(views)[form]
    model.eval()
    got = model.predict(x)
    assert isinstance(got, Prediction) and got.road_map is got[0] and got.boxes is got[1]
    assert got.road_map.dtype == torch.bool and tuple(got.road_map.shape) == (b, 800, 800)
    assert isinstance(got.boxes, tuple) and len(got.boxes) == b and all(t.dim() == 3 and tuple(t.shape[1:]) == (2, 4) for t in got.boxes)

    # 1. the road map: predict_road_map's, and forward's probabilities thresholded
    road = model.predict_road_map(x)
    assert torch.equal(got.road_map, road)
    share_on = float(road.float().mean())
    assert 0.05 < share_on < 0.95, share_on      # both classes: the comparison means something
    masks = tuple(road)
    with torch.no_grad():
        logits, box_map = model(x, masks)
    assert torch.equal(got.road_map, ops.sigmoid(logits) > 0.5)      # the rule of _own_road_masks, bit for bit
    logit64 = logits.double()
    band = pc.band_mask(logit64, 0.5)
    share = float(band.double().mean())
    wrong = (got.road_map != (torch.sigmoid(logit64) > 0.5)) & ~band
    print(f"{form}: road share {share_on:.3f}, band share {share:.2e}, mismatches outside the band {int(wrong.sum())}")
    assert share <= pc.BAND_CAP
    assert not bool(wrong.any())

    # 2. the boxes: the same kernels on the same inputs, so the same bits -- at the defaults, and where the untrained head's map has components
    assert same_boxes(got.boxes, model.predict_boxes(x, masks))
    assert same_boxes(got.boxes, model.predict_boxes(x))      # rm=None: camera-only
    thr = float(box_map.median())
    kw = dict(min_pixels=6, max_boxes=CAP, fit="oriented", pad_px=0.0)
    fitted = model.predict(x, box_threshold=thr, **kw)
    assert torch.equal(fitted.road_map, road) and min(t.shape[0] for t in fitted.boxes) > 0
    assert same_boxes(fitted.boxes, model.predict_boxes(x, masks, threshold=thr, **kw))
    assert same_boxes(fitted.boxes, model.predict_boxes(x, None, thr, **kw))
    assert all(not t.requires_grad for t in fitted.boxes) and all(p.grad is None for p in model.parameters())
    with pytest.raises(ValueError):
        model.predict(x, fit="calipers")


def test_every_mode_flag_is_put_back(dev, model):
    views, _ = jc.views_and_roads(dev, 2, seed=22)
    model.eval()
    want = model.predict(views)

    def frozen_extractor():      # a frozen extractor inside a training model
        model.train()
        model.ae.eval()

    for prepare in (model.train, model.eval, frozen_extractor):
        prepare()
        before = jc.flags(model)
        stats = model.ae.encoder.fc1.fc_bn.running_mean.clone()
        got = model.predict(views)
        boxes = model.predict_boxes(views)
        assert jc.flags(model) == before
        # ... and it ran in eval mode: the same answer whatever the mode, the running statistics untouched
        assert torch.equal(got.road_map, want.road_map) and same_boxes(got.boxes, want.boxes) and same_boxes(boxes, want.boxes)
        assert torch.equal(model.ae.encoder.fc1.fc_bn.running_mean, stats)
    model.train()
    before = jc.flags(model)
    with pytest.raises(ValueError):
        model.predict(views, fit="calipers")
    assert jc.flags(model) == before      # also when the call fails
    model.eval()


def test_the_calibrated_threshold_is_the_default(dev, model):
    views, _ = jc.views_and_roads(dev, 2, seed=23)
    x = tuple(views)
    model.eval()
    assert model.rm_threshold is None
    at_half, at_03 = model.predict(x, threshold=0.5), model.predict(x, threshold=0.3)
    for p in (at_half, at_03):      # neither map is constant, and the two differ: nothing below can pass vacuously
        assert bool(p.road_map.any()) and not bool(p.road_map.all())
    assert not torch.equal(at_half.road_map, at_03.road_map)
    print(f"road share at 0.5: {float(at_half.road_map.float().mean()):.3f}, at 0.3: {float(at_03.road_map.float().mean()):.3f}")
    assert torch.equal(model.predict(x).road_map, at_half.road_map)      # not calibrated: the reference's 0.5
    try:
        model.rm_threshold = 0.3
        got = model.predict(x)
        assert torch.equal(got.road_map, at_03.road_map) and same_boxes(got.boxes, at_03.boxes)
        assert same_boxes(model.predict_boxes(x), at_03.boxes)
        assert torch.equal(got.road_map, model.predict_road_map(x))
        over = model.predict(x, threshold=0.5)      # an explicit argument wins
        assert torch.equal(over.road_map, at_half.road_map) and same_boxes(over.boxes, at_half.boxes)
    finally:
        model.rm_threshold = None


def test_dropout_follows_the_seed(dev):
    model = jc.build_joint(dev, dropout=True)
    assert model.ae.encoder.fc1.drop_p > 0
    views, _ = jc.views_and_roads(dev, 2, seed=24)
    model.eval()
    torch.manual_seed(5)
    a = model.predict(views)
    torch.manual_seed(5)
    b = model.predict(views)
    assert torch.equal(a.road_map, b.road_map) and same_boxes(a.boxes, b.boxes)
    torch.manual_seed(6)
    assert not torch.equal(model.predict(views).road_map, a.road_map)      # the dropout is on (components.py:108)
