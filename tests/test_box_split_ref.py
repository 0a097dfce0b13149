"""Marker-based splitting without a GPU: the numpy reference of tests/_box_split_ref.py on cases whose label images are written out
here, the tiled formulation against the global one, what splitting is worth on cars in contact, and the refusals of the entry points
(host-side validation: nothing is launched)."""
import ctypes
import inspect
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

import _box_eval_ref as ref
import _box_fit_ref as fit
import _box_split_ref as sp


def image(rows, names):
    """Rows of characters -> int32 label image: '.' = 0, any other character = names[character]."""
    return np.array([[0 if ch == "." else names[ch] for ch in row] for row in rows], dtype=np.int32)


# two 9 x 9 squares at columns 1-9 and 13-21 of an 11 x 23 image; their 5 x 5 cores start at (3,3) and (3,15)
A, B = 1 + 3 * 23 + 3, 1 + 3 * 23 + 15


def test_a_three_wide_neck_splits_and_the_tie_takes_the_smaller_label():
    want = image([".......................",
                  ".aaaaaaaaa...bbbbbbbbb.",
                  ".aaaaaaaaa...bbbbbbbbb.",
                  ".aaaaaaaaa...bbbbbbbbb.",
                  ".aaaaaaaaaaabbbbbbbbbb.",
                  ".aaaaaaaaaaabbbbbbbbbb.",
                  ".aaaaaaaaaaabbbbbbbbbb.",
                  ".aaaaaaaaa...bbbbbbbbb.",
                  ".aaaaaaaaa...bbbbbbbbb.",
                  ".aaaaaaaaa...bbbbbbbbb.",
                  "......................."], {"a": A, "b": B})
    mask = sp.two_squares(3)
    assert np.array_equal(mask, want > 0)
    got = sp.split(mask, 2, 4)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # column 11 of the neck is four steps from either core: both reach it in round 4, and the smaller label has it
    assert A < B and (got[4:7, 11] == A).all() and (got[4:7, 12] == B).all()
    # one round less and the middle column is left over: a region of its own, named by its first pixel
    short = sp.split(mask, 2, 3)
    assert (short[4:7, 11] == 1 + 4 * 23 + 11).all() and (short[4:7, 10] == A).all() and (short[4:7, 12] == B).all()
    # unsplit, the whole thing is one component
    assert len(np.unique(ref.label(mask))) == 2


def test_a_seven_wide_neck_stays_one_region():
    mask = sp.two_squares(7)
    got = sp.split(mask, 2, 4)
    assert np.array_equal(got, np.where(mask, A, 0))                               # the neck keeps a core 3 rows high: one core, one region
    assert (sp.erode(mask, 2)[4:7, 3:20]).all()


def test_a_bar_without_a_core_keeps_its_component_label():
    mask = sp.place(np.ones((3, 12), dtype=bool), (8, 20), 2, 4)
    assert not sp.erode(mask, 2).any()
    want = image(["....................",
                  "....................",
                  "....cccccccccccc....",
                  "....cccccccccccc....",
                  "....cccccccccccc....",
                  "....................",
                  "....................",
                  "...................."], {"c": 1 + 2 * 20 + 4})
    assert np.array_equal(sp.split(mask, 2, 4), want) and np.array_equal(ref.label(mask), want)


def test_no_growth_leaves_the_ring_as_a_leftover_region():
    mask = sp.place(np.ones((9, 9), dtype=bool), (11, 12), 1, 2)
    core, ring = 1 + 3 * 12 + 4, 1 + 1 * 12 + 2
    want = image(["............",
                  "..rrrrrrrrr.",
                  "..rrrrrrrrr.",
                  "..rrkkkkkrr.",
                  "..rrkkkkkrr.",
                  "..rrkkkkkrr.",
                  "..rrkkkkkrr.",
                  "..rrkkkkkrr.",
                  "..rrrrrrrrr.",
                  "..rrrrrrrrr.",
                  "............"], {"k": core, "r": ring})
    assert np.array_equal(sp.split(mask, 2, 0), want)
    # one round takes one ring of pixels, corners included (8 neighbours); the rest is still a leftover ring
    one = sp.split(mask, 2, 1)
    assert (one[2:9, 3:10] == core).all() and one[1, 2] == ring and (one > 0).sum() == 81 and set(np.unique(one)) == {0, core, ring}
    assert np.array_equal(sp.split(mask, 2, 2), np.where(mask, core, 0))


def test_labels_name_a_pixel_of_their_own_region_and_partition_the_mask():
    rng = np.random.default_rng(3)
    for density, r, g in ((0.6, 1, 1), (0.9, 2, 3), (0.95, 3, 0)):
        mask = rng.random((50, 70)) < density
        lab = sp.split(mask, r, g)
        assert np.array_equal(lab > 0, mask)
        flat = lab.ravel()
        for v in np.unique(flat[flat > 0]):
            assert flat[v - 1] == v


@pytest.mark.parametrize("r,g", [(1, 0), (1, 2), (2, 4), (3, 16), (8, 16)])
def test_the_tiled_formulation_equals_the_global_one(r, g):
    rng = np.random.default_rng(100 * r + g)
    for density in (0.3, 0.6, 0.9, 0.98):
        mask = rng.random((70, 100)) < density
        assert np.array_equal(sp.split_tiled(mask, r, g), sp.split(mask, r, g)), (density, r, g)
    # blobs with real cores: squares joined by necks, across the tile borders at 32 and 64 and on the image's edges
    mask = np.zeros((70, 100), dtype=bool)
    for y0, x0 in ((0, 0), (27, 20), (59, 77), (25, 55), (40, 0)):
        small = sp.two_squares(3)[1:10, 1:22]
        mask[y0:y0 + 9, x0:x0 + 21] |= small[:70 - y0, :100 - x0]
    assert np.array_equal(sp.split_tiled(mask, r, g), sp.split(mask, r, g))


def test_the_region_fits_equal_the_component_fits_on_components():
    rng = np.random.default_rng(8)
    mask = rng.random((90, 130)) < 0.55
    lab = ref.label(mask)
    for min_pixels in (1, 5):
        assert np.array_equal(sp.region_boxes(lab, min_pixels), ref.component_boxes(mask, min_pixels)[0])
        for pad_px in (0.0, 0.5):
            boxes, moments, _ = fit.fit_components(mask, min_pixels, pad_px)
            got_boxes, got_moments = sp.fit_regions(lab, min_pixels, pad_px)
            assert np.array_equal(got_boxes, boxes) and np.array_equal(got_moments, moments)
    # a region named by a pixel below its top row: the extent's r0 is a minimum over rows, not the naming pixel's row
    lab = np.zeros((6, 8), dtype=np.int32)
    lab[1:5, 2:4] = 1 + 3 * 8 + 2
    assert np.array_equal(sp.region_boxes(lab)[0], ref.extent_to_box(2, 3, 1, 4, 6, 8))


def test_splitting_is_worth_it_on_cars_in_contact():
    """Six scenes of 20 pairs of cars in contact (sp.contact_pairs, seeds 21-26), rasterised, oriented fit with pad_px = 0 and
    min_pixels = 1, scored against the cars themselves with the reference ATS.  Measured with this reference:
        unsplit                          0.0244 - 0.2067   (20-25 blobs for 40 cars)
        split_px = 4, grow_iters = 8     0.2207 - 0.5020   (28-32 regions)
    Every unsplit score lies below every split score; each range is asserted where it was measured, with 0.02 of slack."""
    unsplit, split = [], []
    for seed in sp.CONTACT_SCENE_SEEDS:
        cars, mask = sp.contact_scene_mask(seed)
        assert len(cars) == 40
        unsplit.append(ref.ats(fit.fit_components(mask, 1, 0.0)[0].astype(np.float64), cars))
        split.append(ref.ats(sp.fit_regions(sp.split(mask, 4, 8), 1, 0.0)[0].astype(np.float64), cars))
    print("unsplit", np.round(unsplit, 4), "split", np.round(split, 4))
    assert max(unsplit) < min(split)
    assert 0.0244 - 0.02 <= min(unsplit) and max(unsplit) <= 0.2067 + 0.02
    assert 0.2207 - 0.02 <= min(split) and max(split) <= 0.5020 + 0.02


def test_split_entry_points_refuse_what_they_do_not_support():
    from driving_dirty_amd import _lib, ops
    lib = _lib.lib()
    n = 4 * 800 * 800
    assert lib.dd_split_components_workspace_bytes(4, 800, 800, 4, 8) == 8 * n
    assert lib.dd_split_components_workspace_bytes(1, 70, 100, 8, 16) == 8 * 7000
    assert lib.dd_split_components_workspace_bytes(1, 70, 100, 1, 0) > 0
    for split_px, grow_iters in ((9, 8), (4, 17), (0, 4), (-1, 4), (4, -1)):
        assert lib.dd_split_components_workspace_bytes(1, 70, 100, split_px, grow_iters) == -1
        assert b"[1,8]" in lib.dd_last_error() and b"[0,16]" in lib.dd_last_error()
    assert lib.dd_split_components_workspace_bytes(0, 70, 100, 4, 8) == -1
    assert lib.dd_split_components_workspace_bytes(1, 8193, 100, 4, 8) == -1
    p = ctypes.c_void_p(16)
    assert lib.dd_split_components(None, 0.5, 4, 8, None, 1, 8, 8, None, 0, None) == 2
    assert lib.dd_split_components(p, 0.5, 4, 8, p, 1, 8, 8, None, 0, None) == 2                      # no workspace
    assert lib.dd_split_components(p, 0.5, 4, 8, p, 1, 8, 8, ctypes.c_void_p(24), 1 << 20, None) == 2 and b"aligned" in lib.dd_last_error()
    for split_px, grow_iters in ((9, 8), (4, 17), (0, 4), (-1, 4), (4, -1)):
        assert lib.dd_split_components(p, 0.5, split_px, grow_iters, p, 1, 8, 8, p, 1 << 20, None) == 1
        assert b"[1,8]" in lib.dd_last_error() and b"[0,16]" in lib.dd_last_error()
    need = lib.dd_split_components_workspace_bytes(1, 8, 8, 4, 8)
    assert need == 8 * 64
    assert lib.dd_split_components(p, 0.5, 4, 8, p, 1, 8, 8, p, need - 1, None) == 4 and str(need).encode() in lib.dd_last_error()

    # the fits of a label image: the checks of dd_component_boxes / dd_component_obb
    assert lib.dd_labelled_boxes_workspace_bytes(4, 800, 800) == 20 * n + 2 * 4 * 4 * 800
    assert lib.dd_labelled_obb_workspace_bytes(4, 800, 800, 256) == lib.dd_labelled_boxes_workspace_bytes(4, 800, 800) + 4 * 256 * 80
    assert lib.dd_labelled_boxes_workspace_bytes(1, 8193, 8) == -1
    assert lib.dd_labelled_obb_workspace_bytes(1, 1025, 800, 256) == -1 and b"1024" in lib.dd_last_error()
    assert lib.dd_labelled_obb_workspace_bytes(1, 800, 800, 0) == -1
    assert lib.dd_labelled_boxes(None, 1, 4, None, None, 1, 8, 8, None, 0, None) == 2
    assert lib.dd_labelled_boxes(p, 0, 4, p, p, 1, 8, 8, p, 1 << 20, None) == 2                        # min_pixels
    assert lib.dd_labelled_boxes(p, 1, 4, p, p, 1, 8, 0, p, 1 << 20, None) == 1
    need = lib.dd_labelled_boxes_workspace_bytes(1, 8, 8)
    assert need == 20 * 64 + 2 * 32
    assert lib.dd_labelled_boxes(p, 1, 4, p, p, 1, 8, 8, p, need - 1, None) == 4 and str(need).encode() in lib.dd_last_error()
    assert lib.dd_labelled_obb(None, 1, 4, 0.5, None, None, None, 1, 8, 8, None, 0, None) == 2
    assert lib.dd_labelled_obb(p, 1, 4, -1.0, p, p, None, 1, 8, 8, p, 1 << 20, None) == 2 and b"pad_px" in lib.dd_last_error()
    assert lib.dd_labelled_obb(p, 1, 4, 0.5, p, p, None, 1, 2000, 8, p, 1 << 40, None) == 1 and b"1024" in lib.dd_last_error()
    need = lib.dd_labelled_obb_workspace_bytes(1, 8, 8, 4)
    assert need == 20 * 64 + 2 * 32 + 4 * 80
    assert lib.dd_labelled_obb(p, 1, 4, 0.5, p, p, None, 1, 8, 8, p, need - 1, None) == 4 and str(need).encode() in lib.dd_last_error()

    # the Python shims: no CPU fallback, whole numbers only
    with pytest.raises(_lib.HotpathError):
        ops.split_components(torch.zeros(1, 8, 8), 0.5, 4, 8)
    with pytest.raises(_lib.HotpathError):
        ops.component_boxes(torch.zeros(1, 8, 8), split_px=4)
    with pytest.raises(_lib.HotpathError):
        ops.labelled_boxes(torch.zeros(1, 8, 8, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.component_boxes(torch.zeros(1, 8, 8), split_px=1.5)
    with pytest.raises(ValueError):
        ops.labelled_boxes(torch.zeros(1, 8, 8, dtype=torch.int32), fit="rotated")


def test_splitting_is_off_by_default_everywhere():
    from driving_dirty_amd import ops
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.spatial import BBSpatialRoadMap, boxes_from_map
    args = BBSpatialRoadMap.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([])
    assert args.box_split_px == 0 and args.box_grow_iters is None
    args = BBSpatialRoadMap.add_model_specific_args(ArgumentParser(add_help=False)).parse_args(["--box_split_px", "4", "--box_grow_iters", "6"])
    assert args.box_split_px == 4 and args.box_grow_iters == 6
    for fn in (ops.component_boxes, boxes_from_map, BBSpatialRoadMap.predict_boxes, JointRoadMapBBox.predict_boxes):
        params = inspect.signature(fn).parameters
        assert params["split_px"].default == 0 and params["grow_iters"].default is None, fn
    assert ops._split_args(4, None, "t") == (4, 8) and ops._split_args(3, 5, "t") == (3, 5) and ops._split_args(0, None, "t") == (0, 0)
