"""Pins the CPU reference of the oriented box fit (tests/_box_fit_ref.py) on cases whose answers are known, shows on the reference alone
what the fit is for (rotated cars: the axis-aligned extent scores a perfect map at an ATS near 0.1, the oriented fit near 0.9), and
checks the host-side surface of dd_component_obb (no GPU: nothing is launched here).  test_gpu_box_fit.py then holds the HIP kernels to
this reference."""
import ctypes
import math
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

import _box_eval_ref as ref
import _box_fit_ref as fit

from oracle import raster


def block(c0, c1, r0, r1):
    cols, rows = np.meshgrid(np.arange(c0, c1 + 1), np.arange(r0, r1 + 1))
    return cols.ravel(), rows.ravel()


# ------------------------------------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize("extent,theta", [((410, 429, 380, 389), 0.0),            # wide: the major axis is the row direction
                                          ((410, 419, 380, 399), math.pi / 2),    # tall: atan2(0, negative) = pi
                                          ((0, 256, 0, 0), 0.0), ((7, 7, 0, 129), math.pi / 2),
                                          ((5, 5, 9, 9), 0.0),                    # a single pixel: atan2(0, 0) = 0
                                          ((100, 131, 200, 231), 0.0)])           # a square
def test_axis_aligned_blocks_give_the_extent_box(extent, theta):
    """At pad_px = 0.5 the fit of an axis-aligned block is the box dd_component_boxes gives -- as a corner SET (the ring starts
    elsewhere), and to within one fp32 ulp, not bit for bit: extent_to_box divides in fp32, this fit rounds an fp64 result, and
    cos(pi/2) is 6e-17, not 0."""
    c0, c1, r0, r1 = extent
    for h, w in ((800, 800), (130, 257)):
        if c1 >= w or r1 >= h:
            continue
        box, got_theta, m = fit.fit_pixels(*block(c0, c1, r0, r1), h, w, 0.5)
        assert got_theta == theta
        assert box.dtype == np.float32 and box.shape == (2, 4)
        want = ref.extent_to_box(c0, c1, r0, r1, h, w)
        assert fit.ulp_distance(np.array(fit.corner_set(box)), np.array(fit.corner_set(want))) <= 1.0
        assert m[0] == (c1 - c0 + 1) * (r1 - r0 + 1)
        # columns 0, 1, 3, 2 are the outline: the ring's area is the block's (a 0.1 m side between fp32 coordinates of up to 40 m,
        # each rounded by up to 2e-6 m, is known to 4e-5 of itself)
        area = abs(ref.polygon_area([box[:, k].astype(np.float64) for k in (0, 1, 3, 2)]))
        assert area == pytest.approx(m[0] / 100.0, rel=1e-4)
        # pad_px = 0: the hull of the pixel centres, half a pixel less on every side
        inner, _, _ = fit.fit_pixels(*block(c0, c1, r0, r1), h, w, 0.0)
        assert abs(ref.polygon_area([inner[:, k].astype(np.float64) for k in (0, 1, 3, 2)])) == pytest.approx((c1 - c0) * (r1 - r0) / 100.0, rel=1e-4,
                                                                                                              abs=1e-9)


def test_a_45_degree_staircase_heads_along_the_diagonal():
    """Pixels (i,i), (i+1,i), (i,i+1): 4-connected and symmetric under X <-> Y, so mxx == myy exactly and theta = atan2(+, 0) / 2 =
    pi/4; mirrored in X it is -pi/4.  The fitted box is the band: long side along the diagonal, about sqrt(2) * k pixels."""
    k = 40
    cols = np.array([i for i in range(k)] + [i + 1 for i in range(k)] + [i for i in range(k)])
    rows = np.array([i for i in range(k)] + [i for i in range(k)] + [i + 1 for i in range(k)])
    box, theta, m = fit.fit_pixels(cols + 300, rows + 200, 800, 800, 0.5)
    assert theta == math.pi / 4 and m[0] == 3 * k
    ring = [box[:, c].astype(np.float64) for c in (0, 1, 3, 2)]
    sides = sorted(math.dist(ring[i], ring[(i + 1) % 4]) for i in range(4))
    assert sides[3] == pytest.approx((math.sqrt(2) * (k - 1) + 1 / math.sqrt(2) + math.sqrt(2) * 0.5 * 2) / 10, abs=1e-5)
    assert sides[0] == pytest.approx((math.sqrt(2) + math.sqrt(2) * 0.5 * 2) / 10, abs=1e-5)      # v from -1/sqrt 2 to +1/sqrt 2, plus the pad
    _, mirrored, _ = fit.fit_pixels(500 - cols, rows + 200, 800, 800, 0.5)
    assert mirrored == -math.pi / 4
    # in image coordinates +theta turns from +X towards +Y (down): the band runs from top-left to bottom-right, so in metres
    # (y flipped) its long side has a negative slope
    long_edge = max(((ring[i], ring[(i + 1) % 4]) for i in range(4)), key=lambda e: math.dist(*e))
    d = long_edge[1] - long_edge[0]
    assert d[0] * d[1] < 0 and abs(d[0]) == pytest.approx(abs(d[1]), rel=1e-5)


def test_integer_moments_and_the_vectorised_reference():
    """fit_components (vectorised, int64) against fit_pixels (Python integers, one component at a time) on random masks: moments
    exactly, order by canonical label, corners within the libm differences of numpy and math (one fp32 ulp)."""
    for shape, density, min_pixels, seed in (((5, 7), 0.5, 1, 1), ((64, 64), 0.45, 1, 2), ((130, 257), 0.55, 3, 3)):
        mask = np.random.default_rng(seed).random(shape) < density
        for pad in (0.5, 0.0):
            boxes, moments, theta = fit.fit_components(mask, min_pixels, pad)
            comps = ref.components(mask, min_pixels)
            assert len(boxes) == len(comps) > 0 and moments.dtype == np.int64
            lab = ref.label(mask)
            for i, (label, pixels, *_rest) in enumerate(comps):
                rows, cols = np.nonzero(lab == label)
                box, th, m = fit.fit_pixels(cols, rows, shape[0], shape[1], pad)
                assert tuple(int(v) for v in moments[i]) == m and m[0] == pixels
                assert abs(theta[i] - th) <= 1e-15 and -math.pi / 2 < th <= math.pi / 2
                assert fit.ulp_distance(boxes[i], box) <= 1.0
    # a run's closed forms, as the kernel adds them: [x, x + n) in row y
    for x, y, n in ((0, 0, 1), (3, 9, 64), (960, 1023, 64), (17, 5, 33)):
        tri = n * (n - 1) // 2
        want = fit.moments_of(range(x, x + n), [y] * n)
        assert want == (n, n * x + tri, n * y, n * x * x + 2 * x * tri + (n - 1) * n * (2 * n - 1) // 6, y * (n * x + tri), n * y * y)
    # the range the kernel accepts: a full 1024 x 1024 component keeps every product inside int64
    n, s1, s2 = 1024 * 1024, 1024 * (1023 * 1024 // 2), 1024 * (1023 * 1024 * 2047 // 6)
    assert n * s2 < 2 ** 60 and s1 * s1 < 2 ** 60


# ------------------------------------------------------------------------------------------------ 2. what the fit is for
def scene_scores(seed, pad_px):
    cars = fit.car_scene(seed)
    mask = raster.boxes_to_binary_map(torch.from_numpy(cars).numpy()) > 0.5
    extent, n_extent = ref.component_boxes(mask)
    oriented, _, _ = fit.fit_components(mask, 1, pad_px)
    m = ref.iou_matrix(oriented, cars)
    return len(cars), n_extent, len(oriented), ref.ats(extent, cars), ref.ats_from_iou(m), m


def test_oriented_fit_scores_a_perfect_map_of_rotated_cars():
    """Eight scenes of 40 car-sized rectangles with uniformly random heading that do not merge, painted with the oracle rasteriser;
    the perfect map is decoded back to boxes with both fits and scored against the boxes that painted it.  Asserted: the oriented
    fit's ATS is at least twice the extent fit's, and every car's best IoU under the oriented fit exceeds 0.5.  Also the condition
    the device round trip (test_gpu_box_fit.py) relies on: in at least three quarters of the scenes no IoU lies within 1e-4 of a
    threshold, for both paddings."""
    qualifying = {0.5: 0, 0.0: 0}
    for seed in fit.CAR_SCENE_SEEDS:
        for pad in (0.5, 0.0):
            n, n_extent, n_oriented, ats_extent, ats_oriented, m = scene_scores(seed, pad)
            worst = float(m.max(axis=0).min())
            print(f"seed {seed} pad_px {pad}: {n_oriented} components, ATS extent {ats_extent:.4f} oriented {ats_oriented:.4f}, "
                  f"mean best IoU {m.max(axis=0).mean():.4f}, worst {worst:.4f}, threshold margin {ref.threshold_margin(m):.2e}")
            assert n_extent == n and n_oriented == n                               # nothing merged, nothing lost
            assert ats_oriented >= 2.0 * ats_extent and ats_oriented > 0.5
            assert float(m.max(axis=1).min()) > 0.5 and worst > 0.5                # every component, and every car
            qualifying[pad] += ref.threshold_margin(m) >= 1e-4
    assert all(4 * q >= 3 * len(fit.CAR_SCENE_SEEDS) for q in qualifying.values()), qualifying


# ------------------------------------------------------------------------------------------------ 3. host-side surface, no launches
def test_obb_entry_point_refuses_what_it_does_not_support():
    from driving_dirty_amd import _lib, ops
    lib = _lib.lib()
    n = 4 * 800 * 800
    assert lib.dd_component_obb_workspace_bytes(4, 800, 800, 256) == 20 * n + 2 * 4 * 4 * 800 + 4 * 256 * 80
    assert lib.dd_component_obb_workspace_bytes(4, 800, 800, 256) == lib.dd_component_boxes_workspace_bytes(4, 800, 800) + 4 * 256 * 80
    assert lib.dd_component_obb_workspace_bytes(1, 1024, 1024, 1 << 20) > 0
    assert lib.dd_component_obb_workspace_bytes(1, 1025, 800, 256) == -1 and b"1024" in lib.dd_last_error()
    assert lib.dd_component_obb_workspace_bytes(1, 800, 1025, 256) == -1 and b"1024" in lib.dd_last_error()
    assert lib.dd_component_obb_workspace_bytes(0, 800, 800, 256) == -1
    assert lib.dd_component_obb_workspace_bytes(1, 800, 800, 0) == -1
    assert lib.dd_component_obb_workspace_bytes(1, 800, 800, (1 << 20) + 1) == -1 and b"1048576" in lib.dd_last_error()
    p = ctypes.c_void_p(16)
    assert lib.dd_component_obb(None, 0.5, 1, 4, 0.5, None, None, None, 1, 8, 8, None, 0, None) == 2
    assert lib.dd_component_obb(p, 0.5, 1, 4, 0.5, p, p, None, 1, 8, 8, None, 0, None) == 2          # no workspace
    assert lib.dd_component_obb(p, 0.5, 0, 4, 0.5, p, p, None, 1, 8, 8, p, 1 << 20, None) == 2         # min_pixels
    assert lib.dd_component_obb(p, 0.5, 1, 4, -1.0, p, p, None, 1, 8, 8, p, 1 << 20, None) == 2 and b"pad_px" in lib.dd_last_error()
    assert lib.dd_component_obb(p, 0.5, 1, 4, float("nan"), p, p, None, 1, 8, 8, p, 1 << 20, None) == 2
    assert lib.dd_component_obb(p, 0.5, 1, 4, 0.5, p, p, None, 1, 8, 8, ctypes.c_void_p(24), 1 << 20, None) == 2 and b"aligned" in lib.dd_last_error()
    assert lib.dd_component_obb(p, 0.5, 1, 4, 0.5, p, p, None, 1, 8, 0, p, 1 << 20, None) == 1
    assert lib.dd_component_obb(p, 0.5, 1, 4, 0.5, p, p, None, 1, 2000, 8, p, 1 << 40, None) == 1 and b"1024" in lib.dd_last_error()
    need = lib.dd_component_obb_workspace_bytes(1, 8, 8, 4)
    assert need == 20 * 64 + 2 * 32 + 4 * 80
    assert lib.dd_component_obb(p, 0.5, 1, 4, 0.5, p, p, None, 1, 8, 8, p, need - 1, None) == 4 and str(need).encode() in lib.dd_last_error()
    # the Python shim: a bad fit is a ValueError, a CPU tensor is refused (there is no CPU fallback), moments belong to the oriented fit
    with pytest.raises(ValueError):
        ops.component_boxes(torch.zeros(1, 8, 8), fit="rotated")
    with pytest.raises(ValueError):
        ops.component_boxes(torch.zeros(1, 8, 8), want_moments=True)
    with pytest.raises(_lib.HotpathError):
        ops.component_boxes(torch.zeros(1, 8, 8), fit="oriented")


def test_box_fit_flags_default_to_the_extent_fit():
    import inspect
    from driving_dirty_amd import ops
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.lightning import hparam
    from driving_dirty_amd.spatial import BBSpatialRoadMap, boxes_from_map
    parser = BBSpatialRoadMap.add_model_specific_args(ArgumentParser(add_help=False))
    args = parser.parse_args([])
    assert args.box_fit == "extent" and args.box_pad_px == 0.5 and args.box_metrics is False
    args = parser.parse_args(["--box_metrics", "--box_fit", "oriented", "--box_pad_px", "0"])
    assert args.box_fit == "oriented" and args.box_pad_px == 0.0
    with pytest.raises(SystemExit):
        parser.parse_args(["--box_fit", "calipers"])
    assert hparam(parser.parse_args([]), "box_fit", "extent") == "extent"
    for fn in (ops.component_boxes, boxes_from_map, BBSpatialRoadMap.predict_boxes, JointRoadMapBBox.predict_boxes):
        sig = inspect.signature(fn).parameters
        assert sig["fit"].default == "extent" and sig["pad_px"].default == 0.5, fn
