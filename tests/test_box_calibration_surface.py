"""CPU tests of the box threshold calibration: the argmax and its tie-break, the data-set mean, the grid's and
``box_min_pixels``' validation, the command line, where the operating point is kept, the resolution order of a decode's arguments and
``validation_epoch_end`` on hand-made outputs, for both modules with a box head."""
import inspect
from argparse import ArgumentParser, Namespace

import pytest
import torch

GRID = tuple(k / 16 for k in range(1, 16))
JOINT_ALWAYS = ("val_loss", "val_roadmap_loss", "val_bbox_loss", "val_ts", "val_ts_rounded")
NEW = {"best_box_threshold", "best_val_ats", "val_ats_at_half"}


def small_ae():
    from driving_dirty_amd.autoencoder import BasicAE
    return BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))


def build_joint(**extra):
    from driving_dirty_amd.joint import JointRoadMapBBox
    return JointRoadMapBBox(Namespace(pretrained_ae=small_ae(), learning_rate=1e-3, output_img_freq=500, **extra))


def build_box(**extra):
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    return BBSpatialRoadMap(Namespace(pretrained_ae=small_ae(), unfreeze_epoch_no=5, learning_rate=1e-3, output_img_freq=500, **extra))


BUILDERS = [build_box, build_joint]


def curve_with(values, default=0.1):
    """A curve over GRID: ``default`` everywhere but at the sixteenths named in ``values``."""
    c = [default] * len(GRID)
    for sixteenth, v in values.items():
        c[sixteenth - 1] = v
    return torch.tensor(c, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ best_box_threshold
def test_a_unique_maximum_is_found():
    from driving_dirty_amd.spatial import BOX_THRESHOLD_GRID, best_box_threshold
    assert BOX_THRESHOLD_GRID == GRID and all(float(torch.tensor(t, dtype=torch.float32)) == t for t in GRID)      # exact in fp32
    sums = curve_with({3: 0.5, 11: 2.25, 12: 2.0}) * 4
    k, curve = best_box_threshold(sums, 4, GRID)
    assert k == 10 and GRID[k] == 11 / 16
    assert curve.dtype == torch.float64 and curve.device.type == "cpu" and torch.equal(curve, sums / 4)
    k32, curve32 = best_box_threshold(sums.float().tolist(), 4, GRID)      # any K numbers will do
    assert k32 == 10 and curve32.dtype == torch.float64


def test_ties_go_to_the_threshold_nearest_half_then_to_the_lower_one():
    from driving_dirty_amd.spatial import best_box_threshold
    assert best_box_threshold(curve_with({6: 0.7, 9: 0.7}), 1, GRID)[0] == 8          # 9/16 is nearer 0.5 than 6/16
    assert best_box_threshold(curve_with({2: 0.7, 4: 0.7, 15: 0.7}), 1, GRID)[0] == 3  # 4/16, on the low side
    assert best_box_threshold(curve_with({7: 0.7, 9: 0.7}), 1, GRID)[0] == 6          # equidistant: the lower one
    assert best_box_threshold(curve_with({4: 1.0, 5: 1.0}), 1, GRID)[0] == 4          # 5/16
    assert best_box_threshold(curve_with({7: 0.7, 8: 0.7, 9: 0.7}), 1, GRID)[0] == 7  # 0.5 itself
    # a grid without 0.5, unevenly spaced: the distance is measured on the thresholds, not on their indices
    assert best_box_threshold(torch.tensor([1.0, 1.0, 1.0]), 1, (0.1, 0.45, 0.6))[0] == 1
    assert best_box_threshold(torch.tensor([1.0, 0.0, 1.0]), 1, (0.4, 0.5, 0.6))[0] == 0


def test_an_all_zero_curve_picks_half_on_the_default_grid():
    from driving_dirty_amd.spatial import best_box_threshold
    k, curve = best_box_threshold(torch.zeros(15, dtype=torch.float64), 7, GRID)
    assert GRID[k] == 0.5 and not curve.any()


def test_no_samples_and_mismatched_lengths_raise():
    from driving_dirty_amd.spatial import best_box_threshold
    for count in (0, -1):
        with pytest.raises(ValueError, match="no samples"):
            best_box_threshold(torch.zeros(15, dtype=torch.float64), count, GRID)
    with pytest.raises(ValueError, match="14 sums for 15 thresholds"):
        best_box_threshold(torch.zeros(14, dtype=torch.float64), 1, GRID)


def test_the_curve_is_the_data_set_mean_not_the_mean_of_batch_means():
    """Two batches of 2 and 3 samples.  At 4/16 the per-sample scores are (1, 1) and (0, 0, 0.5): batch means 1 and 1/6, their mean
    7/12, the pooled mean 2.5/5 = 0.5.  At 5/16 they are (0.5, 0.5) and (0.6, 0.6, 0.6): batch means 0.5 and 0.6, their mean 0.55,
    pooled 0.56.  The mean of batch means would pick 4/16; the data set's mean picks 5/16."""
    from driving_dirty_amd.spatial import best_box_threshold
    per_sample = {4: ([1.0, 1.0], [0.0, 0.0, 0.5]), 5: ([0.5, 0.5], [0.6, 0.6, 0.6])}
    sums = [torch.zeros(15, dtype=torch.float64), torch.zeros(15, dtype=torch.float64)]
    for sixteenth, batches in per_sample.items():
        for s, scores in zip(sums, batches):
            s[sixteenth - 1] = sum(scores)
    k, curve = best_box_threshold(sums[0] + sums[1], 2 + 3, GRID)
    assert GRID[k] == 5 / 16
    assert curve[3] == 2.5 / 5 and curve[4] == pytest.approx(2.8 / 5, abs=1e-15)
    batch_means = (sums[0] / 2 + sums[1] / 3) / 2
    assert int(batch_means.argmax()) == 3 and batch_means[3] == pytest.approx(7 / 12)      # what must NOT be computed


# ------------------------------------------------------------------------------------------------ hparams: validation, flags, carrying
@pytest.mark.parametrize("build", BUILDERS)
def test_bad_grids_and_min_pixels_are_refused_when_the_module_is_built(build):
    from driving_dirty_amd.spatial import box_threshold_grid
    for bad in ((0.5, 0.25), (0.25, 0.25), (0.0, 0.5), (0.5, 1.0), (-0.1,), (1.5,), (), [], "0.5", 0.5, (0.25, "0.5"), (True,), (float("nan"),)):
        with pytest.raises(ValueError, match="box_threshold_grid"):
            build(box_threshold_grid=bad)
    model = build(box_threshold_grid=[0.125, 0.5, 0.75])
    assert box_threshold_grid(model.hparams) == (0.125, 0.5, 0.75)
    assert box_threshold_grid(build().hparams) == GRID
    for bad in (0, -3, 1.5, "2", True):
        with pytest.raises(ValueError, match="box_min_pixels"):
            build(box_min_pixels=bad)
    assert build(box_min_pixels=4).hparams.box_min_pixels == 4


def test_the_flags_parse_through_both_modules():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.lightning import hparam
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    for cls, build in ((BBSpatialRoadMap, build_box), (JointRoadMapBBox, build_joint)):
        parser = cls.add_model_specific_args(ArgumentParser(add_help=False))
        args = parser.parse_args([])
        assert args.calibrate_box_threshold is False and args.box_min_pixels == 1
        assert hparam(args, "box_threshold", None) is None and hparam(args, "box_threshold_grid", None) is None
        args = parser.parse_args(["--calibrate_box_threshold", "--box_min_pixels", "5"])
        assert args.calibrate_box_threshold is True and args.box_min_pixels == 5
        model = build(**{k: v for k, v in vars(args).items() if k not in ("pretrained_ae", "learning_rate", "output_img_freq", "unfreeze_epoch_no")})
        assert model.box_threshold is None and model._wants_box_sweep()
        with pytest.raises(ValueError, match="box_min_pixels"):
            build(box_min_pixels=parser.parse_args(["--box_min_pixels", "0"]).box_min_pixels)
        with pytest.raises(SystemExit):
            parser.parse_args(["--box_min_pixels", "1.5"])


@pytest.mark.parametrize("build", BUILDERS)
def test_box_threshold_lives_in_hparams_and_in_the_checkpoint(build, tmp_path):
    from driving_dirty_amd.spatial import CalibratedBoxThreshold
    model = build(box_min_pixels=3)
    assert isinstance(model, CalibratedBoxThreshold)
    assert isinstance(inspect.getattr_static(type(model), "box_threshold"), property)
    assert model.box_threshold is None and not hasattr(model.hparams, "box_threshold")
    keys = list(model.state_dict().keys())
    model.box_threshold = 5 / 16
    assert type(model.box_threshold) is float and model.hparams.box_threshold == 0.3125 and list(model.state_dict().keys()) == keys
    path = str(tmp_path / "model.ckpt")
    model.save_checkpoint(path)
    loaded = type(model).load_from_checkpoint(path)
    assert type(loaded.box_threshold) is float and loaded.box_threshold == 0.3125 and loaded.hparams.box_min_pixels == 3
    model.box_threshold = None
    assert model.box_threshold is None
    model.save_checkpoint(path)
    assert type(model).load_from_checkpoint(path).box_threshold is None


def test_both_modules_share_the_mixin():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.spatial import BBSpatialRoadMap, CalibratedBoxThreshold
    for name in ("box_threshold", "_with_box_sweep", "_calibrate_boxes", "calibrate_boxes"):
        assert inspect.getattr_static(JointRoadMapBBox, name) is inspect.getattr_static(BBSpatialRoadMap, name) \
            is inspect.getattr_static(CalibratedBoxThreshold, name), name
    for cls in (JointRoadMapBBox, BBSpatialRoadMap):      # ... and each runs its own forward pass for calibrate_boxes
        assert "_box_sweep_of" in vars(cls)


# ------------------------------------------------------------------------------------------------ the resolution order
def test_explicit_argument_then_calibrated_value_then_half():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.spatial import BBSpatialRoadMap, box_decode_point
    plain, tuned = Namespace(), Namespace(box_threshold=0.3125, box_min_pixels=4)
    assert box_decode_point(plain) == (0.5, 1) and box_decode_point(tuned) == (0.3125, 4)
    assert box_decode_point(Namespace(box_threshold=None)) == (0.5, 1)
    assert box_decode_point(tuned, 0.5, 1) == (0.5, 1) and box_decode_point(tuned, 0.75) == (0.75, 4)      # explicit wins, 0.5 and 1 too
    assert box_decode_point(tuned, None, 2) == (0.3125, 2)
    # the methods' own defaults mean "not given", whatever a signature shows for them
    for fn, names in ((BBSpatialRoadMap.predict_boxes, ("threshold", "min_pixels")), (JointRoadMapBBox.predict_boxes, ("threshold", "min_pixels")),
                      (JointRoadMapBBox.predict, ("box_threshold", "min_pixels"))):
        sig = inspect.signature(fn).parameters
        given = tuple(sig[n].default for n in names)
        assert box_decode_point(tuned, *given) == (0.3125, 4) and box_decode_point(plain, *given) == (0.5, 1), fn
    assert [p.default for p in list(inspect.signature(JointRoadMapBBox.predict_boxes).parameters.values())[3:5]] == [None, None]
    assert [p.default for p in list(inspect.signature(BBSpatialRoadMap.predict_boxes).parameters.values())[3:5]] == [None, None]


# ------------------------------------------------------------------------------------------------ validation_epoch_end
def sweeps():
    """The sweeps of two batches (2 and 3 samples) of test_the_curve_is_the_data_set_mean, as ``validation_step`` stores them: the K sums,
    then the sample count."""
    a, b = torch.zeros(16, dtype=torch.float64), torch.zeros(16, dtype=torch.float64)
    a[3], a[4], a[7], a[15] = 2.0, 1.0, 0.5, 2
    b[3], b[4], b[7], b[15] = 0.5, 1.8, 0.3, 3
    return a, b


@pytest.mark.parametrize("build,always", [(build_box, ("val_loss",)), (build_joint, JOINT_ALWAYS)])
def test_epoch_end_calibrates_from_the_summed_sweeps(build, always):
    from driving_dirty_amd.spatial import CalibratedBoxThreshold
    key = CalibratedBoxThreshold.BOX_SWEEP
    outs = [{k: torch.tensor(0.25 * (i + 1)) for k in always} for i in range(2)]
    base = {"avg_" + k for k in always}
    off = build()
    end = off.validation_epoch_end(outs)
    assert set(end["log"]) == base and off.box_threshold is None      # the parent's log
    for o, s in zip(outs, sweeps()):
        o[key] = s
    end = off.validation_epoch_end(outs)      # not asked for: the sweeps are ignored
    assert set(end["log"]) == base and off.box_threshold is None and not hasattr(off.hparams, "box_threshold")
    model = build(calibrate_box_threshold=True)
    end = model.validation_epoch_end(outs)
    assert set(end) == {"val_loss", "log"} and set(end["log"]) == base | NEW
    assert type(model.box_threshold) is float and model.box_threshold == 5 / 16
    log = end["log"]
    assert log["best_box_threshold"] == 5 / 16 and log["best_val_ats"] == pytest.approx(2.8 / 5, abs=1e-15)
    assert log["val_ats_at_half"] == pytest.approx(0.8 / 5, abs=1e-15)
    assert all(type(log[k]) is float for k in NEW)
    # a grid without 0.5 has no val_ats_at_half
    model = build(calibrate_box_threshold=True, box_threshold_grid=(0.25, 0.75))
    for o, s in zip(outs, (torch.tensor([1.0, 0.5, 2], dtype=torch.float64), torch.tensor([0.0, 1.0, 3], dtype=torch.float64))):
        o[key] = s
    end = model.validation_epoch_end(outs)
    assert set(end["log"]) == base | (NEW - {"val_ats_at_half"}) and model.box_threshold == 0.75 and end["log"]["best_val_ats"] == 0.3
