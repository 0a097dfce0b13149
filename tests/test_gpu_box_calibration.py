"""GPU tests of the box threshold calibration: ``spatial.box_ats_sweep`` against the fp64 CPU reference on maps with a
known answer and against the existing decode, then both modules end to end: validation, ``calibrate_boxes``, the predictions' default."""
import copy
import math
import os
import sys
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _box_eval_ref as ref  # noqa: E402
import _joint_cases as jc  # noqa: E402

GRID = tuple(k / 16 for k in range(1, 16))
ATS_TOL = 1e-6      # tests/test_gpu_box_eval.py: ops.ats_bounding_boxes against this reference, per sample
JOINT_ALWAYS = {"val_loss", "val_roadmap_loss", "val_bbox_loss", "val_ts", "val_ts_rounded"}
JOINT_BOX = {"val_ats_gt_rm", "val_ats", "val_box_ts"}
KEY = "box_ats_sweep"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def same_boxes(a, b):
    return len(a) == len(b) and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(a, b))


def pick(curve, thresholds=GRID):
    """The rule, restated: the maximum; ties to the threshold nearest 0.5, then to the lower one."""
    top = max(curve)
    return min((k for k, v in enumerate(curve) if v == top), key=lambda k: (abs(thresholds[k] - 0.5), k))


# ------------------------------------------------------------------------------------------------ 1. a known answer
CAR_H, CAR_W, CAR, BRIDGE, SPECKLE = 45, 20, 0.35, 0.2, 0.6


def synthetic_maps():
    """(maps fp32 [3,800,800], cars-only maps): per sample four cars of 20 x 45 pixels at 0.35, the first two 10 pixels apart and joined
    by a bridge 3 pixels thick at 0.2, and three single pixels at 0.6 far from everything.  Every sample at places of its own."""
    maps, cars = np.zeros((3, 800, 800), dtype=np.float32), np.zeros((3, 800, 800), dtype=np.float32)
    for i in range(3):
        r, c = 101 + 53 * i, 97 + 31 * i
        for (y, x) in ((r, c), (r, c + CAR_W + 10), (r + 200, c + 300), (r + 330, c + 77)):
            cars[i, y:y + CAR_H, x:x + CAR_W] = CAR
        maps[i] = cars[i]
        maps[i, r + 20:r + 23, c + CAR_W:c + CAR_W + 10] = BRIDGE
        for (y, x) in ((700 + 7 * i, 40), (30, 700 - 11 * i), (650, 650 + i)):
            assert cars[i, y - 2:y + 3, x - 2:x + 3].max() == 0
            maps[i, y, x] = SPECKLE
    return maps, cars


@pytest.fixture(scope="module")
def known(dev):
    """(maps on the device, targets, {min_pixels: the reference's curve}): the targets are the reference's boxes of the cars alone at 0.25;
    the curve is the reference's labelling, boxes and ATS of ``maps > fp32(t)``, computed once on the CPU."""
    maps, cars = synthetic_maps()
    target_boxes = [ref.component_boxes(cars[i] > np.float32(0.25))[0].astype(np.float64) for i in range(3)]
    assert all(len(t) == 4 for t in target_boxes)
    curves = {}
    for min_pixels in (1, 2):
        curves[min_pixels] = [sum(ref.ats(ref.component_boxes(maps[i] > np.float32(t), min_pixels)[0], target_boxes[i]) for i in range(3)) / 3
                              for t in GRID]
    targets = tuple({"bounding_box": torch.from_numpy(t)} for t in target_boxes)
    return torch.from_numpy(maps).to(dev), targets, curves


def test_the_reference_gives_the_constructed_answer(known):
    """The construction, checked on the CPU reference alone: 0.35 > 5/16 and not > 6/16, 0.2 > 3/16 and not > 4/16, 0.6 > 9/16."""
    _, _, curves = known
    two, one = curves[2], curves[1]
    assert two[3] == two[4] == 1.0 and pick(two) == 4
    assert all(0 < v < 1 for v in two[:3]) and all(v == 0 for v in two[5:])
    assert one[3] == one[4] == max(one) and 0 < one[3] < 1 and pick(one) == 4
    assert all(0 < v < one[3] for v in one[:3]) and all(v == 0 for v in one[5:])


@pytest.mark.parametrize("min_pixels", [2, 1])
def test_the_sweep_against_the_reference(dev, known, min_pixels):
    from driving_dirty_amd.spatial import best_box_threshold, box_ats_sweep
    maps, targets, curves = known
    sums, count = box_ats_sweep(Namespace(box_min_pixels=min_pixels), maps, targets, GRID)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (15,) and sums.is_cuda and count == 3
    k, curve = best_box_threshold(sums, count, GRID)
    err = np.abs(curve.numpy() - np.array(curves[min_pixels])).max()
    print(f"min_pixels {min_pixels}: curve {[round(v, 6) for v in curve.tolist()]}, worst |sweep - reference| {err:.3e}, chosen {GRID[k]}")
    assert err <= ATS_TOL
    assert k == pick(curves[min_pixels]) == 4 and GRID[k] == 5 / 16
    assert curve[3] == curve[4]      # the same boxes at 4/16 and 5/16: the same bits, a true tie
    if min_pixels == 2:
        assert abs(float(curve[4]) - 1.0) <= ATS_TOL and not curve[5:].any()


# ------------------------------------------------------------------------------------------------ 2. the sweep is the existing decode
@pytest.mark.parametrize("fit,pad_px", [("extent", 0.5), ("oriented", 0.25)])
@pytest.mark.parametrize("split_px", [0, 2])
def test_the_sweep_is_the_existing_decode(dev, known, fit, pad_px, split_px):
    from driving_dirty_amd import ops
    from driving_dirty_amd.spatial import box_ats_sweep, boxes_from_map, decoded_box_ats
    maps, targets, _ = known
    boxes = [t["bounding_box"] for t in targets]
    hp = Namespace(box_fit=fit, box_pad_px=pad_px, box_split_px=split_px, box_min_pixels=2)
    sums, count = box_ats_sweep(hp, maps, targets, GRID)
    assert count == 3
    for k, t in enumerate(GRID):
        per_sample = ops.ats_bounding_boxes(boxes_from_map(maps, t, 2, fit=fit, pad_px=pad_px, split_px=split_px), boxes)
        assert torch.equal(sums[k], per_sample.double().sum()), (k, t)
    # ... and decoded_box_ats at a calibrated threshold is that mean
    hp.box_threshold = 3 / 16
    at = decoded_box_ats(hp, maps, targets)
    assert torch.equal(at, ops.ats_bounding_boxes(boxes_from_map(maps, 3 / 16, 2, fit=fit, pad_px=pad_px, split_px=split_px), boxes).mean())
    assert abs(float(at) - float(sums[2]) / 3) <= 3 * 2.0 ** -24      # fp32 mean of 3 scores in [0, 1] against the fp64 one
    assert len({round(float(v), 9) for v in sums}) >= 3


# ------------------------------------------------------------------------------------------------ 4. no overflow noise
def test_an_overflowing_threshold_is_swept_quietly(dev):
    from driving_dirty_amd import ops
    from driving_dirty_amd.spatial import box_ats_sweep, boxes_from_map
    maps = torch.zeros(1, 800, 800, device=dev)
    maps[0, 100:140:2, 100:140:2] = 0.9      # 400 single-pixel components
    with pytest.warns(UserWarning, match="more than max_boxes=256"):
        first = boxes_from_map(maps, GRID[0])
    assert first[0].shape[0] == 256
    targets = ({"bounding_box": first[0][:100].double().cpu()},)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sums, count = box_ats_sweep(Namespace(), maps, targets, GRID[:1])
        quiet = boxes_from_map(maps, GRID[0], warn_overflow=False)
    assert not caught, [str(w.message) for w in caught]
    assert count == 1 and same_boxes(quiet, first)
    # it scores what its first 256 boxes score: 100 of them match a target exactly
    want = ops.ats_bounding_boxes(first, [targets[0]["bounding_box"]])
    assert torch.equal(sums[0], want.double().sum()) and abs(float(sums[0]) - 100 / 256) <= ATS_TOL


# ------------------------------------------------------------------------------------------------ 3. both modules, end to end
BOX_GAIN = 48.0      # up_conv_5's weight times this: the centred map of the filled head then spans 0.02 .. 0.998, every threshold cuts it
BEST = 11            # the intended best threshold, in sixteenths: the targets are the model's own boxes there
MIN_PIXELS = 30      # the untrained head's map is per-pixel noise (1e5 components): at 30 pixels a few to a few hundred per sample are left


def box_map(model, x, rm):
    out = model(x, rm)
    return out[1] if isinstance(out, tuple) else out


def build(kind, dev, **extra):
    if kind == "joint":
        model = jc.build_joint(dev, **extra)
    else:
        from driving_dirty_amd import synth
        from driving_dirty_amd.autoencoder import BasicAE
        from driving_dirty_amd.spatial import BBSpatialRoadMap
        model = BBSpatialRoadMap(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=16, latent_dim=8)), unfreeze_epoch_no=5, **jc.HP, **extra))
        synth.fill_module(model, seed=29)
        model = model.to(dev)
    return model.eval()


def spread_and_centre(model, x, rm):
    """``_joint_cases.centre_box_map`` after widening the map as HEAD_GAIN widens the road head's: the last layer's weight times BOX_GAIN,
    then its bias moved so that the map's median is 0.5."""
    with torch.no_grad():
        model.box_merge.up_conv_5.weight.mul_(BOX_GAIN)
        m = float(box_map(model, x, rm).median())
        assert 0.0 < m < 1.0
        model.box_merge.up_conv_5.bias -= math.log(m / (1.0 - m))


def decode(kind, model, x, rm, threshold):
    """The model's own boxes, the map the module validates: with the batch's road map for the box module, camera-only for the joint one."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # more than 256 components at some thresholds: expected here
        return model.predict_boxes(x, rm, threshold=threshold) if kind == "box" else model.predict_boxes(x, threshold=threshold)


@pytest.fixture(scope="module", params=["box", "joint"])
def case(request, dev):
    """(kind, model, two batches of B = 2 and 3, the pooled curve recomputed from ``predict_boxes`` threshold by threshold, and the same
    per batch).  The targets are the model's own boxes at BEST / 16 (25 - 29 per sample), so the curve is 1.0 there; the filled head's
    map is per-pixel noise, so the boxes of any other threshold hardly meet them: measured on an MI355X, 0.0016 (box) and 0.0005
    (joint) at 10/16 and 0 elsewhere -- three distinct values, the maximum away from 0.5, which the fixture asserts."""
    from driving_dirty_amd import ops
    kind = request.param
    model = build(kind, dev, calibrate_box_threshold=True, box_min_pixels=MIN_PIXELS)
    inputs = []
    for b, seed in ((2, 17), (3, 18)):
        views, road = jc.views_and_roads(dev, b, seed=seed)
        inputs.append((tuple(views), tuple(road)))
    spread_and_centre(model, *inputs[0])
    with torch.no_grad():
        q = torch.quantile(box_map(model, *inputs[0]).flatten()[::16].float(), torch.tensor([0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99], device=dev))
    print(f"{kind}: box map quantiles 1/10/25/50/75/90/99 % {[round(v, 3) for v in q.tolist()]}")
    batches = []
    for x, rm in inputs:
        own = decode(kind, model, x, rm, BEST / 16)
        assert all(t.shape[0] > 0 for t in own)
        print(f"{kind}: target boxes per sample {[t.shape[0] for t in own]}")
        batches.append((x, tuple({"bounding_box": t.double().cpu()} for t in own), rm))
    total = [0.0] * len(GRID)
    per_batch = []
    for x, targets, rm in batches:
        rows = [ops.ats_bounding_boxes(decode(kind, model, x, rm, t), [d["bounding_box"] for d in targets]).double().cpu() for t in GRID]
        per_batch.append([float(r.sum()) / len(x) for r in rows])
        total = [a + float(r.sum()) for a, r in zip(total, rows)]
    curve = [v / 5 for v in total]
    print(f"{kind}: pooled curve {[round(v, 4) for v in curve]}")
    # the conditions under which the tests below mean something: not a flat curve, and an operating point that is not the default
    assert len(set(curve)) >= 3 and pick(curve) != 7 and pick(curve) == BEST - 1
    return kind, model, batches, curve, per_batch


def test_validation_calibrates_and_the_predictions_follow(dev, case):
    kind, model, batches, curve, per_batch = case
    x, targets, rm = batches[0]
    model.box_threshold = None
    before = model.predict(x).boxes if kind == "joint" else model.predict_boxes(x, rm)      # nothing calibrated: 0.5
    assert same_boxes(before, decode(kind, model, x, rm, 0.5))
    with torch.no_grad():
        outs = [model.validation_step(batch, i) for i, batch in enumerate(batches)]
    always = JOINT_ALWAYS if kind == "joint" else {"val_loss"}
    for out, batch in zip(outs, batches):
        assert set(out) == always | {KEY}
        assert out[KEY].dtype == torch.float64 and tuple(out[KEY].shape) == (16,) and float(out[KEY][-1]) == len(batch[0])
    end = model.validation_epoch_end(outs)
    k = pick(curve)
    assert model.box_threshold == GRID[k] and end["log"]["best_box_threshold"] == GRID[k]
    # sums of at most five fp32 scores in fp64: the order of the additions costs at most a few ulp
    assert abs(end["log"]["best_val_ats"] - curve[k]) <= 1e-12 and abs(end["log"]["val_ats_at_half"] - curve[7]) <= 1e-12
    assert end["log"]["best_val_ats"] > end["log"]["val_ats_at_half"]
    # the predictions decode there by default; an explicit argument wins
    if kind == "joint":
        got = model.predict(x).boxes
        assert same_boxes(got, model.predict(x, box_threshold=model.box_threshold).boxes) and same_boxes(got, model.predict_boxes(x))
        assert same_boxes(model.predict(x, box_threshold=0.5).boxes, before) and not same_boxes(got, before)
    else:
        got = model.predict_boxes(x, rm)
        assert same_boxes(got, model.predict_boxes(x, rm, threshold=model.box_threshold))
        assert same_boxes(model.predict_boxes(x, rm, threshold=0.5), before) and not same_boxes(got, before)
    assert same_boxes(got, decode(kind, model, x, rm, GRID[k]))
    # val_ats under box_metrics now decodes at the calibrated threshold: the curve's value there, for each batch
    model.hparams.box_metrics = True
    try:
        for i, batch in enumerate(batches):
            with torch.no_grad():
                out = model.validation_step(batch, i)
            assert set(out) == always | {KEY} | (JOINT_BOX if kind == "joint" else {"val_ats", "val_ts"})
            b = len(batch[0])
            assert torch.equal(out[KEY], outs[i][KEY])
            assert abs(float(out["val_ats"]) - float(out[KEY][k]) / b) <= b * 2.0 ** -24      # an fp32 mean of b scores in [0, 1]
            assert abs(float(out["val_ats"]) - per_batch[i][k]) <= b * 2.0 ** -24
    finally:
        model.hparams.box_metrics = False


def test_calibrate_boxes_is_the_validation_path(dev, case):
    from driving_dirty_amd.spatial import best_box_threshold
    kind, model, batches, curve, _ = case
    with torch.no_grad():
        outs = [model.validation_step(batch, i) for i, batch in enumerate(batches)]
    total = torch.stack([o[KEY] for o in outs]).sum(0).cpu()
    k, want = best_box_threshold(total[:-1], 5, GRID)
    fresh = copy.deepcopy(model)
    fresh.hparams.calibrate_box_threshold = False      # a checkpoint trained without the flag
    fresh.box_threshold = None
    fresh.train()
    fresh.ae.eval()      # a frozen extractor inside a training model
    before = jc.flags(fresh)
    threshold, got = fresh.calibrate_boxes(iter(batches))
    assert jc.flags(fresh) == before
    assert threshold == fresh.box_threshold == GRID[k] == GRID[pick(curve)]
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert all(p.grad is None for p in fresh.parameters())


def test_the_flag_off_leaves_the_outputs_as_they_were(dev, case):
    kind, model, batches, _, _ = case
    always = JOINT_ALWAYS if kind == "joint" else {"val_loss"}
    model.hparams.calibrate_box_threshold = False
    saved = model.box_threshold
    try:
        for box_metrics in (False, True):
            model.hparams.box_metrics = box_metrics
            with torch.no_grad():
                out = model.validation_step(batches[0], 0)
            assert set(out) == always | ((JOINT_BOX if kind == "joint" else {"val_ats", "val_ts"}) if box_metrics else set())
            end = model.validation_epoch_end([out, out])
            assert set(end["log"]) == {"avg_" + k for k in out} and model.box_threshold == saved
    finally:
        model.hparams.calibrate_box_threshold, model.hparams.box_metrics = True, False
