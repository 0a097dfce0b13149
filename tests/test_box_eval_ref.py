"""Pins the CPU reference of the box-level validation ops (tests/_box_eval_ref.py) on cases whose answers are known by hand, and the
host-side surface of the new entry points (no GPU: nothing is launched here).  The GPU tests (test_gpu_box_eval.py) then hold the
HIP kernels to this reference."""
import ctypes
import math
from argparse import ArgumentParser
from fractions import Fraction

import numpy as np
import pytest
import torch

import _box_eval_ref as ref


def test_iou_known_answers():
    for box1, box2, expected in ref.exact_cases():
        assert ref.iou(box1, box2) == pytest.approx(expected, abs=1e-12)
        assert ref.iou(box2, box1) == pytest.approx(expected, abs=1e-12)
    # the octagon case, spelled out: I = 2 (sqrt 2 - 1), IoU = I / (2 - I) ~ 0.7071
    sq = ref.rotated_rect(0.0, 0.0, 1.0, 1.0, 0.0)
    assert ref.iou(sq, ref.rotated_rect(0.0, 0.0, 1.0, 1.0, math.pi / 4)) == pytest.approx(0.70710678, abs=1e-8)
    # far from the origin the same shapes give the same answer (the reference translates before it multiplies)
    a, b = ref.rotated_rect(38.5, -39.0, 1.0, 1.0, 0.0), ref.rotated_rect(39.0, -39.0, 1.0, 1.0, 0.0)
    assert ref.iou(a, b) == pytest.approx(1.0 / 3.0, abs=1e-12)


def test_hull_is_the_outline_for_either_corner_order():
    """The reference takes the convex hull of the four corners: column order and orientation do not matter."""
    rng = np.random.default_rng(5)
    boxes = np.concatenate([ref.random_rects(rng, 6, (3.0, -4.0)), ref.random_convex_quads(rng, 6, (3.0, -4.0))])
    for a in boxes:
        ring = [a[:, k] for k in (0, 1, 3, 2)]
        area = abs(ref.polygon_area(ring))
        assert area > 0 and ref.polygon_area(ref.convex_hull(a.T)) == pytest.approx(area, rel=1e-12)
        for b in boxes:
            assert ref.iou(a, b) == pytest.approx(ref.iou(a[:, ::-1], b[:, [2, 3, 0, 1]]), abs=1e-12)
            assert 0.0 <= ref.iou(a, b) <= 1.0 + 1e-12


def test_ats_hand_computed_three_against_two():
    """Set 2: unit squares at (0,0) and (10,10).  Set 1: the first exactly, the second shifted by 0.2 (I = 0.8, U = 1.2, IoU = 2/3),
    and a stray.  iou_max = [1, 2/3]: tp = 2 at 0.5 and 0.6 (ts = 2/3), tp = 1 at 0.7, 0.8, 0.9 (ts = 1/4)."""
    set2 = np.array([ref.rotated_rect(0, 0, 1, 1, 0), ref.rotated_rect(10, 10, 1, 1, 0)])
    set1 = np.array([ref.rotated_rect(0, 0, 1, 1, 0), ref.rotated_rect(10.2, 10, 1, 1, 0), ref.rotated_rect(-20, 5, 2, 1, 0.4)])
    m = ref.iou_matrix(set1, set2)
    assert m.shape == (3, 2)
    assert m[0, 0] == pytest.approx(1.0) and m[1, 1] == pytest.approx(2.0 / 3.0) and m[2].max() == 0 and m[0, 1] == 0 and m[1, 0] == 0
    w = [Fraction(10, k) for k in (5, 6, 7, 8, 9)]
    ts = [Fraction(2, 3), Fraction(2, 3), Fraction(1, 4), Fraction(1, 4), Fraction(1, 4)]
    expected = sum(a * b for a, b in zip(w, ts)) / sum(w)
    assert ref.ats(set1, set2) == pytest.approx(float(expected), abs=1e-12)
    assert float(expected) == pytest.approx(0.4548962, abs=1e-6)
    assert ref.ats(set1[:0], set2) == 0.0 and ref.ats(set1, set2[:0]) == 0.0


def test_labels_of_a_hand_drawn_mask():
    """6 x 7, two components that touch only diagonally (4-connectivity keeps them apart) and a lone pixel."""
    mask = np.array([[0, 1, 1, 0, 0, 0, 0],
                     [0, 0, 1, 0, 0, 0, 0],
                     [0, 0, 1, 0, 0, 0, 1],
                     [0, 0, 0, 1, 1, 0, 0],
                     [0, 0, 0, 1, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0]], dtype=bool)
    a, b, c = 0 * 7 + 1 + 1, 3 * 7 + 3 + 1, 2 * 7 + 6 + 1
    expected = np.array([[0, a, a, 0, 0, 0, 0],
                         [0, 0, a, 0, 0, 0, 0],
                         [0, 0, a, 0, 0, 0, c],
                         [0, 0, 0, b, b, 0, 0],
                         [0, 0, 0, b, 0, 0, 0],
                         [0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    assert np.array_equal(ref.label(mask), expected)
    assert ref.components(mask) == [(a, 4, 1, 2, 0, 2), (c, 1, 6, 6, 2, 2), (b, 3, 3, 4, 3, 4)]
    assert ref.components(mask, min_pixels=3) == [(a, 4, 1, 2, 0, 2), (b, 3, 3, 4, 3, 4)]
    # a U shape whose first pixel is not in the extent's first column
    u = np.array([[0, 0, 1], [1, 0, 1], [1, 1, 1]], dtype=bool)
    assert np.array_equal(ref.label(u), np.where(u, 3, 0)) and ref.components(u) == [(3, 6, 0, 2, 0, 2)]


def test_extent_to_box_is_the_inverse_pixel_mapping():
    """Pixel (r,c) of an 800 x 800 map covers x in [(c-400)/10, (c+1-400)/10] and y in [(399-r)/10, (400-r)/10] (px = x*10+400, then the
    vertical flip, bb_to_img.py:14-20); corner columns 0 = (x_max,y_max), 1 = (x_max,y_min), 2 = (x_min,y_max), 3 = (x_min,y_min)."""
    box = ref.extent_to_box(410, 429, 380, 389, 800, 800)
    f = np.float32
    assert box.dtype == np.float32
    assert np.array_equal(box, np.array([[f(3.0), f(3.0), f(1.0), f(1.0)], [f(2.0), f(1.0), f(2.0), f(1.0)]], dtype=np.float32))
    # the ring 0,1,3,2 is the outline
    ring = [box[:, k] for k in (0, 1, 3, 2)]
    assert abs(ref.polygon_area(ring)) == pytest.approx(2.0)
    odd = ref.extent_to_box(0, 256, 0, 129, 130, 257)
    assert np.array_equal(odd[0], np.array([f(128.5) / f(10), f(128.5) / f(10), f(-128.5) / f(10), f(-128.5) / f(10)]))
    assert np.array_equal(odd[1], np.array([f(65) / f(10), f(-65) / f(10), f(65) / f(10), f(-65) / f(10)]))


def test_ats_generator_rarely_needs_a_discard():
    """The GPU test regenerates pairs of sets with an IoU within 1e-3 of a threshold; at most 1 in 20 may go that way."""
    rng = np.random.default_rng(2024)
    discarded, total = 0, 60
    for _ in range(total):
        s1, s2 = ref.ats_pair(rng, int(rng.integers(1, 30)), int(rng.integers(0, 10)), int(rng.integers(0, 3)), int(rng.integers(0, 8)),
                              int(rng.integers(0, 8)))
        discarded += ref.threshold_margin(ref.iou_matrix(s1, s2)) < 1e-3
    assert discarded * 20 <= total, (discarded, total)


# ------------------------------------------------------------------------------------------------ host-side surface, no launches
def test_entry_points_refuse_what_they_do_not_support():
    from driving_dirty_amd import _lib, ops
    lib = _lib.lib()
    assert lib.dd_label_components_workspace_bytes(4, 800, 800) == 0
    assert lib.dd_label_components_workspace_bytes(1, 9000, 800) == -1 and b"8192" in lib.dd_last_error()
    assert lib.dd_component_boxes_workspace_bytes(0, 800, 800) == -1
    n = 4 * 800 * 800
    assert lib.dd_component_boxes_workspace_bytes(4, 800, 800) == 20 * n + 2 * 4 * 4 * 800
    assert lib.dd_label_components(None, 0.5, None, 1, 8, 8, None) == 2
    assert lib.dd_label_components(ctypes.c_void_p(16), 0.5, ctypes.c_void_p(16), 1, 8, 0, None) == 1
    assert lib.dd_component_boxes(None, 0.5, 1, 4, None, None, 1, 8, 8, None, 0, None) == 2
    off = (ctypes.c_int32 * 2)(0, 5000)
    ok = (ctypes.c_int32 * 2)(0, 3)
    assert lib.dd_box_iou_ats_workspace_bytes(off, ok, 1) == -1 and b"4096" in lib.dd_last_error()
    assert lib.dd_box_iou_ats_workspace_bytes(ok, ok, 1) >= 9 * 4
    assert lib.dd_box_iou_ats(ctypes.c_void_p(16), 0, off, ctypes.c_void_p(16), 0, ok, None, ctypes.c_void_p(16), 1, None, 0, None) == 1
    assert lib.dd_box_iou_ats(ctypes.c_void_p(16), 0, ok, ctypes.c_void_p(16), 0, ok, None, ctypes.c_void_p(16), 1, None, 0, None) == 4
    assert lib.dd_box_iou_ats(None, 0, ok, None, 0, ok, None, None, 1, None, 0, None) == 2
    # the Python shims refuse CPU tensors: there is no CPU fallback
    with pytest.raises(_lib.HotpathError):
        ops.label_components(torch.zeros(1, 8, 8))
    with pytest.raises(_lib.HotpathError):
        ops.component_boxes(torch.zeros(1, 8, 8))
    with pytest.raises(_lib.HotpathError):
        ops.box_iou(torch.zeros(2, 2, 4), torch.zeros(3, 2, 4))
    with pytest.raises(_lib.HotpathError):
        ops.ats_bounding_boxes([torch.zeros(2, 2, 4)], [torch.zeros(3, 2, 4)])


def test_box_metrics_flag_is_off_unless_asked_for():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.lightning import hparam
    from driving_dirty_amd.spatial import BBSpatialRoadMap, compute_ats_bounding_boxes
    parser = BBSpatialRoadMap.add_model_specific_args(ArgumentParser(add_help=False))
    assert parser.parse_args([]).box_metrics is False and parser.parse_args(["--box_metrics"]).box_metrics is True
    assert hparam(parser.parse_args([]), "box_metrics", False) is False
    assert callable(compute_ats_bounding_boxes) and hasattr(BBSpatialRoadMap, "predict_boxes") and hasattr(JointRoadMapBBox, "predict_boxes")
    # validation_epoch_end averages the keys that are present, and returns what it always did when they are absent
    m = BBSpatialRoadMap.__new__(BBSpatialRoadMap)
    plain = BBSpatialRoadMap.validation_epoch_end(m, [{"val_loss": torch.tensor(1.0)}, {"val_loss": torch.tensor(3.0)}])
    assert set(plain) == {"val_loss", "log"} and set(plain["log"]) == {"avg_val_loss"} and float(plain["val_loss"]) == 2.0
    full = BBSpatialRoadMap.validation_epoch_end(m, [{"val_loss": torch.tensor(1.0), "val_ats": torch.tensor(0.5), "val_ts": torch.tensor(0.2)},
                                                      {"val_loss": torch.tensor(3.0), "val_ats": torch.tensor(0.0), "val_ts": torch.tensor(0.4)}])
    assert set(full["log"]) == {"avg_val_loss", "avg_val_ats", "avg_val_ts"}
    assert float(full["log"]["avg_val_ats"]) == 0.25 and float(full["log"]["avg_val_ts"]) == pytest.approx(0.3)


def test_ats_generator_of_the_130_sample_batches():
    """The generator of tests/test_gpu_batch_boundaries.py alone (ref.ats_arrangements): at most 1 pair in 20 discarded, no kept IoU
    within 1e-3 of a threshold, and the empty sets where the two arrangements say (samples 0, 63, 64, 129; every sample of 64-127)."""
    arrangements, cases, generated = ref.ats_arrangements()
    assert len(cases) == 130 and (generated - len(cases)) * 20 <= generated, f"{generated - len(cases)} of {generated} pairs discarded"
    for _, _, m in cases:
        assert ref.threshold_margin(m) >= 1e-3
    assert len({(len(a), len(b)) for a, b, _ in cases}) > 20 and sum(m.size for _, _, m in cases) > 1000
    s1, s2, mats = arrangements["edges"]
    assert [i for i in range(130) if not mats[i].size] == [0, 63, 64, 129]
    assert len(s1[0]) == 0 and len(s2[63]) == 0 and len(s1[64]) == 0 and len(s2[129]) == 0
    s1, s2, mats = arrangements["middle"]
    assert all(mats[i].size == 0 for i in range(64, 128)) and all(mats[i].size > 0 for i in list(range(64)) + [128, 129])
    assert any(len(s1[i]) == 0 for i in range(64, 128)) and any(len(s2[i]) == 0 for i in range(64, 128))
