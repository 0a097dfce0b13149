"""CPU tests of the joint model's surface past ``training_step``: validation, camera-only prediction, the calibrated threshold, the
command line, and the promise that all of it runs on the C ABI as it was (no entry point added or removed)."""
import inspect
import json
import os
import re
import sys
from argparse import ArgumentParser, Namespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ts_curve_ref import ts_curve_ref  # noqa: E402


def build(**extra):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.joint import JointRoadMapBBox
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))
    return JointRoadMapBBox(Namespace(pretrained_ae=ae, learning_rate=1e-3, output_img_freq=500, **extra))


def test_the_module_has_the_surface_of_the_single_task_modules():
    from driving_dirty_amd.joint import JointRoadMapBBox
    for name in ("validation_step", "validation_epoch_end", "predict", "predict_boxes", "predict_road_map", "add_model_specific_args",
                 "_features", "_box_branch", "_road_logits", "_own_road_masks"):
        assert callable(getattr(JointRoadMapBBox, name, None)), name
    assert isinstance(inspect.getattr_static(JointRoadMapBBox, "rm_threshold"), property)
    sig = inspect.signature(JointRoadMapBBox.predict_boxes)
    assert sig.parameters["rm"].default is None                      # camera-only is the default
    assert list(sig.parameters)[:3] == ["self", "x", "rm"]          # ... and a given rm still goes where it went
    sig = inspect.signature(JointRoadMapBBox.predict)
    assert list(sig.parameters) == ["self", "x", "threshold", "box_threshold", "min_pixels", "max_boxes", "fit", "pad_px", "split_px", "grow_iters"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, 0.5, 1, 256, "extent", 0.5, 0, None]


def test_rm_threshold_lives_in_hparams():
    model = build()
    assert model.rm_threshold is None and model.box_rm_input == "target"
    keys = list(model.state_dict().keys())
    model.rm_threshold = 0.3
    assert type(model.rm_threshold) is float and model.hparams.rm_threshold == 0.3 and list(model.state_dict().keys()) == keys
    model.rm_threshold = None
    assert model.rm_threshold is None


def test_box_rm_input_is_checked_when_the_module_is_built():
    assert build(box_rm_input="target").box_rm_input == "target"
    assert build(box_rm_input="predicted").box_rm_input == "predicted"
    for bad in ("nonsense", "", None, "Predicted"):
        with pytest.raises(ValueError, match="box_rm_input"):
            build(box_rm_input=bad)


def test_the_parser_takes_every_flag():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.spatial import box_loss_config
    parser = JointRoadMapBBox.add_model_specific_args(ArgumentParser(add_help=False))
    args = parser.parse_args([])
    assert args.box_rm_input == "target" and args.calibrate_threshold is False and args.box_metrics is False
    assert (args.box_fit, args.box_pad_px, args.box_split_px, args.box_grow_iters) == ("extent", 0.5, 0, None)
    assert box_loss_config(args) is None and args.precision == "fp32" and args.learning_rate == 1e-3
    args = parser.parse_args(["--box_rm_input", "predicted", "--calibrate_threshold", "--box_metrics", "--box_fit", "oriented", "--box_pad_px", "0",
                              "--box_split_px", "3", "--box_grow_iters", "5", "--box_pos_weight", "auto", "--box_bce_weight", "2", "--box_ts_weight",
                              "1", "--box_ts_eps", "0.5", "--precision", "fp32x3", "--learning_rate", "0.01", "--batch_size", "4",
                              "--pretrained_path", "ae.ckpt", "--link", "data", "--output_img_freq", "7"])
    assert args.box_rm_input == "predicted" and args.calibrate_threshold and args.box_metrics and args.precision == "fp32x3"
    assert (args.box_fit, args.box_pad_px, args.box_split_px, args.box_grow_iters) == ("oriented", 0.0, 3, 5)
    assert box_loss_config(args) == {"pos_weight": "auto", "bce_weight": 2.0, "ts_weight": 1.0, "ts_eps": 0.5}
    with pytest.raises(SystemExit):
        parser.parse_args(["--box_rm_input", "nonsense"])
    # the flags the two single-task parsers share with it mean the same there
    from driving_dirty_amd.roadmap import RoadMapBCE
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    box = BBSpatialRoadMap.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([])
    rm = RoadMapBCE.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([])
    joint = vars(parser.parse_args([]))
    for other in (vars(box), vars(rm)):
        for k in set(other) & set(joint):
            assert other[k] == joint[k], k
    assert set(joint) == (set(vars(box)) | set(vars(rm)) | {"box_rm_input"}) - {"unfreeze_epoch_no", "mse_loss"}      # the joint model freezes nothing


ALWAYS = ("val_loss", "val_roadmap_loss", "val_bbox_loss", "val_ts", "val_ts_rounded")


def _outputs(keys, n=3, seed=0):
    rs = np.random.RandomState(seed)
    return [{k: torch.tensor(float(rs.random_sample()), dtype=torch.float32) for k in keys} for _ in range(n)]


@pytest.mark.parametrize("extra", [(), ("val_bce", "val_soft_ts"), ("val_ats_gt_rm", "val_ats", "val_box_ts"),
                                   ("val_bce", "val_soft_ts", "val_ats_gt_rm", "val_ats", "val_box_ts")])
def test_epoch_end_averages_every_key_present(extra):
    model = build()
    outs = _outputs(ALWAYS + extra)
    end = model.validation_epoch_end(outs)
    assert set(end) == {"val_loss", "log"} and set(end["log"]) == {"avg_" + k for k in ALWAYS + extra}
    for k in ALWAYS + extra:
        assert torch.equal(end["log"]["avg_" + k], torch.stack([o[k] for o in outs]).mean()), k
    assert torch.equal(end["val_loss"], end["log"]["avg_val_loss"])      # the monitored value
    assert model.rm_threshold is None


def test_epoch_end_calibrates_from_the_summed_histograms():
    rs = np.random.RandomState(3)
    hists = []
    for _ in range(3):      # positives lean high, negatives low: a curve with an inner maximum
        pos = np.bincount(np.clip(rs.normal(150, 40, 4000), 0, 256).astype(np.int64), minlength=257)
        neg = np.bincount(np.clip(rs.normal(90, 40, 9000), 0, 256).astype(np.int64), minlength=257)
        hists.append(np.stack([neg, pos]))
    ts, best = ts_curve_ref(np.sum(hists, axis=0))
    assert 0 < best < 255 and best != 128
    outs = _outputs(ALWAYS)
    for o, h in zip(outs, hists):
        o["ts_hist"] = torch.from_numpy(h)
    off = build()
    end_off = off.validation_epoch_end(outs)      # not asked for: the histograms are ignored
    assert off.rm_threshold is None and set(end_off["log"]) == {"avg_" + k for k in ALWAYS}
    model = build(calibrate_threshold=True)
    end = model.validation_epoch_end(outs)
    assert type(model.rm_threshold) is float and model.rm_threshold == best / 256
    log = end["log"]
    assert set(log) == {"avg_" + k for k in ALWAYS} | {"best_threshold", "best_val_ts", "val_ts_at_half"}
    assert log["best_threshold"] == best / 256 and log["best_val_ts"] == ts[best] and log["val_ts_at_half"] == ts[128]
    # ... by the code RoadMapBCE calibrates with
    from driving_dirty_amd.roadmap import CalibratedThreshold, RoadMapBCE
    from driving_dirty_amd.joint import JointRoadMapBBox
    assert JointRoadMapBBox._calibrate is RoadMapBCE._calibrate is CalibratedThreshold._calibrate
    assert inspect.getattr_static(JointRoadMapBBox, "rm_threshold") is inspect.getattr_static(RoadMapBCE, "rm_threshold")


def test_the_header_declares_the_functions_it_declared():
    with open(os.path.join(ROOT, "include", "dd_hotpath.h")) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dd_\w+)\s*\(", text)))
    with open(os.path.join(ROOT, "tests", "golden", "abi_names.json")) as f:
        want = json.load(f)
    assert want == sorted(set(want)) and names == want
    from driving_dirty_amd import _lib
    assert sorted(_lib.SIGNATURES) == want
