"""Marker-based splitting on the device (csrc/boxeval.hip: dd_split_components, dd_labelled_boxes, dd_labelled_obb; ops.split_components,
ops.component_boxes(split_px=...)) against the numpy reference of tests/_box_split_ref.py, and the module surface built on it.

Labels, counts, order, extent boxes and moments are integers (or one fp32 division of an exact number): compared exactly.  Oriented
corners: ULP_BOUND = 1 fp32 ulp, the bound test_gpu_box_fit.py derives for the same arithmetic; IoU: IOU_BOUND of test_gpu_box_eval.py."""
import functools

import numpy as np
import pytest
import torch

import _box_eval_ref as ref
import _box_fit_ref as fit
import _box_split_ref as sp

from driving_dirty_amd import synth
from test_gpu_box_eval import IOU_BOUND, build_model, random_mask
from test_gpu_box_fit import ULP_BOUND

pytestmark = pytest.mark.gpu

SETTINGS = [(1, 0), (1, 2), (2, 4), (3, 16), (8, 16)]
SHAPE = (3, 70, 100)          # tiles of 32 cut by both image edges: 3 x 4 tiles, the last row 6 high, the last column 4 wide


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def to_maps(masks, dev):
    return torch.from_numpy(np.ascontiguousarray(masks, dtype=np.float32)).to(dev)


@functools.lru_cache(maxsize=None)
def hand_made():
    """[3,70,100]: the hand-made cases of test_box_split_ref.py, placed so that necks, cores and ties lie across the tile borders at 32
    and 64 and on rows and columns 0 and H-1 / W-1 (the one-pixel frame of sp.two_squares cut off where a blob touches the edge)."""
    b, h, w = SHAPE
    m = np.zeros(SHAPE, dtype=bool)

    def put(i, small, y0, x0):
        ys, xs = small.shape
        m[i, y0:y0 + ys, x0:x0 + xs] |= small[:h - y0, :w - x0]

    pair3, pair7 = sp.two_squares(3)[1:-1, 1:-1], sp.two_squares(7)[1:-1, 1:-1]      # 9 x 21
    put(0, pair3, 0, 0)                    # on row 0 and column 0
    put(0, pair3, 27, 21)                  # the neck (columns 30-32) across the border at 32, the squares across the border at 32 (rows)
    put(0, pair7, 61, 79)                  # on row 69 and column 99, across the border at 64
    put(0, pair3.T, 40, 60)                # upright, across the border at column 64; its neck at rows 49-51
    put(0, np.ones((3, 40), dtype=bool), 15, 50)                                   # a bar without a core over two tiles
    big = sp.two_squares(5, gap=4, size=25)[1:-1, 1:-1]                            # 25 x 54: cores even at split_px = 8
    put(1, big, 20, 23)                    # the neck at columns 48-51, the tie inside it; squares over the borders at 32 and 64
    put(1, sp.two_squares(3, gap=2, size=19)[1:-1, 1:-1], 0, 0)                    # 19 x 40 in the corner: cores at split_px <= 8 on the edge
    put(1, pair3, 50, 2)
    put(1, big.T[:, :20], 10, 80)          # cut by column 99
    put(2, np.ones((70, 100), dtype=bool), 0, 0)
    m[2, 30:34, :] = False                 # two slabs ...
    m[2, 30:34, 62:67] = True              # ... joined by a neck 5 wide across the corner (32, 64)
    m[2, 0:20, 40:43] = False
    return m


@functools.lru_cache(maxsize=None)
def reference_labels(name, r, g):
    masks = hand_made() if name == "hand" else random_mask(SHAPE, float(name), seed=int(100 * float(name)))
    return masks, np.stack([sp.split(m, r, g) for m in masks])


# ------------------------------------------------------------------------------------------------ 1. labels
@pytest.mark.parametrize("r,g", SETTINGS)
@pytest.mark.parametrize("name", ["0.3", "0.6", "0.9", "hand"])
def test_labels_equal_the_reference(dev, name, r, g):
    from driving_dirty_amd import ops
    masks, want = reference_labels(name, r, g)
    got = ops.split_components(to_maps(masks, dev), 0.5, r, g)
    assert got.dtype == torch.int32 and tuple(got.shape) == SHAPE
    got = got.cpu().numpy()
    regions = [len(np.unique(x)) - 1 for x in want]
    print(f"{name} ({r},{g}): regions per sample {regions}, components {[len(np.unique(ref.label(m))) - 1 for m in masks]}")
    assert np.array_equal(got, want)
    if name == "hand":
        cores = [int(sp.erode(m, r).sum()) for m in masks]
        assert min(cores[1:]) > 0                                                  # the erosion leaves something to grow at every setting
        if (r, g) == (2, 4):
            assert regions[0] > len(np.unique(ref.label(masks[0]))) - 1            # and blobs do come apart


def test_labels_of_a_full_size_contact_scene(dev):
    from driving_dirty_amd import ops
    cars = [sp.contact_pairs(seed) for seed in sp.CONTACT_SCENE_SEEDS[:2]]
    maps = ops.boxes_to_binary_map([torch.from_numpy(c).to(dev) for c in cars])
    assert tuple(maps.shape) == (2, 800, 800)
    masks = maps.cpu().numpy() > 0.5
    want = np.stack([sp.split(m, 4, 8) for m in masks])
    got = ops.split_components(maps, 0.5, 4, 8).cpu().numpy()
    assert np.array_equal(got, want)
    assert all(len(np.unique(w)) - 1 > len(np.unique(ref.label(m))) - 1 for w, m in zip(want, masks))
    # the default number of rounds is 2 * split_px, and the threshold reaches the kernels
    assert np.array_equal(ops.split_components(maps, 0.5, 4).cpu().numpy(), want)
    assert np.array_equal(ops.split_components(maps * 0.5, 0.25, 4, 8).cpu().numpy(), want)
    assert not ops.split_components(maps * 0.5, 0.5, 4, 8).any()


# ------------------------------------------------------------------------------------------------ 2. / 3. boxes from split labels
@pytest.mark.parametrize("r,g", [(1, 2), (2, 4), (8, 16)])
@pytest.mark.parametrize("name", ["0.6", "0.9", "hand"])
def test_boxes_from_split_labels_equal_the_reference(dev, name, r, g):
    from driving_dirty_amd import ops
    masks, labels = reference_labels(name, r, g)
    maps = to_maps(masks, dev)
    worst = 0.0
    for min_pixels, cap in ((1, 4096), (4, 16)):
        boxes, counts = ops.component_boxes(maps, 0.5, min_pixels, cap, split_px=r, grow_iters=g)
        obb, ocounts, moments = ops.component_boxes(maps, 0.5, min_pixels, cap, fit="oriented", pad_px=0.0, want_moments=True, split_px=r,
                                                    grow_iters=g)
        assert torch.equal(counts, ocounts)
        boxes, obb, moments = boxes.cpu().numpy(), obb.cpu().numpy(), moments.cpu().numpy()
        for i, lab in enumerate(labels):
            want = sp.region_boxes(lab, min_pixels)
            want_obb, want_moments = sp.fit_regions(lab, min_pixels, 0.0)
            assert int(counts[i]) == len(want) == len(want_obb)                    # uncapped
            n = min(len(want), cap)
            assert np.array_equal(boxes[i, :n], want[:n]) and not boxes[i, n:].any()      # bit-identical, order included
            assert np.array_equal(moments[i, :n], want_moments[:n]) and not moments[i, n:].any()
            worst = max(worst, fit.ulp_distance(obb[i, :n], want_obb[:n]))
            assert not obb[i, n:].any()
    print(f"{name} ({r},{g}): worst corner difference {worst:.2f} fp32 ulp (bound {ULP_BOUND})")
    assert worst <= ULP_BOUND


def test_labelled_fits_of_plain_components_are_the_component_fits(dev):
    """On dd_label_components' own output the label-image entry points return the bytes of dd_component_boxes / dd_component_obb; a label
    that names no region (out of range, or whose pixel does not carry it) is ignored."""
    from driving_dirty_amd import ops
    maps = to_maps(np.concatenate([random_mask((2, 70, 100), 0.55, seed=4), hand_made()[:1]]), dev)
    labels = ops.label_components(maps, 0.5)
    for min_pixels, cap in ((1, 2048), (3, 8)):
        assert all(torch.equal(a, b) for a, b in zip(ops.labelled_boxes(labels, min_pixels, cap), ops.component_boxes(maps, 0.5, min_pixels, cap)))
        got = ops.labelled_boxes(labels, min_pixels, cap, fit="oriented", pad_px=0.5, want_moments=True)
        want = ops.component_boxes(maps, 0.5, min_pixels, cap, fit="oriented", pad_px=0.5, want_moments=True)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    stray = labels.clone()
    background = (labels[0] == 0).nonzero()
    (y0, x0), (y1, x1), (y2, x2) = background[0].tolist(), background[1].tolist(), background[-1].tolist()
    # too large, negative, and the name of a pixel that does not carry it (pixel (y1, x1) now holds -5)
    stray[0, y0, x0], stray[0, y1, x1], stray[0, y2, x2] = 70 * 100 + 1, -5, y1 * 100 + x1 + 1
    for kw in ({}, {"fit": "oriented", "want_moments": True}):
        assert all(torch.equal(a, b) for a, b in zip(ops.labelled_boxes(labels, 1, 2048, **kw), ops.labelled_boxes(stray, 1, 2048, **kw)))


# ------------------------------------------------------------------------------------------------ 4. / 5. determinism, independence
def test_two_launches_are_bit_identical_and_samples_are_independent(dev):
    from driving_dirty_amd import ops
    masks = np.concatenate([hand_made()[1:2], random_mask((1, 70, 100), 0.9, seed=2), hand_made()[2:3]])
    maps = to_maps(masks, dev)
    for r, g in ((2, 4), (8, 16)):
        first, again = ops.split_components(maps, 0.5, r, g), ops.split_components(maps, 0.5, r, g)
        assert torch.equal(first, again)
        boxes = ops.component_boxes(maps, 0.5, 1, 512, fit="oriented", want_moments=True, split_px=r, grow_iters=g)
        assert all(torch.equal(a, b) for a, b in zip(boxes, ops.component_boxes(maps, 0.5, 1, 512, fit="oriented", want_moments=True, split_px=r,
                                                                                 grow_iters=g)))
        for i in range(3):
            assert torch.equal(ops.split_components(maps[i:i + 1].contiguous(), 0.5, r, g)[0], first[i])
        assert torch.equal(ops.split_components(maps.flip(0).contiguous(), 0.5, r, g).flip(0), first)


def test_split_px_zero_changes_nothing(dev):
    from driving_dirty_amd import ops
    maps = to_maps(np.concatenate([hand_made()[:2], random_mask((1, 70, 100), 0.6, seed=6)]), dev)
    assert all(torch.equal(a, b) for a, b in zip(ops.component_boxes(maps, 0.5, 2, 64, split_px=0), ops.component_boxes(maps, 0.5, 2, 64)))
    assert all(torch.equal(a, b) for a, b in zip(ops.component_boxes(maps, 0.5, 2, 64, split_px=0, grow_iters=5), ops.component_boxes(maps, 0.5, 2, 64)))
    want = ops.component_boxes(maps, 0.5, 2, 64, fit="oriented", pad_px=0.25, want_moments=True)
    got = ops.component_boxes(maps, 0.5, 2, 64, fit="oriented", pad_px=0.25, want_moments=True, split_px=0)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    from driving_dirty_amd import _lib
    for split_px, grow_iters in ((9, None), (4, 17), (-1, 2)):
        with pytest.raises(_lib.HotpathError):
            ops.component_boxes(maps, split_px=split_px, grow_iters=grow_iters)


# ------------------------------------------------------------------------------------------------ 6. round trip
def test_round_trip_of_cars_in_contact(dev):
    """Cars in contact -> ops.boxes_to_binary_map -> split (4, 8) -> oriented fit -> ops.ats_bounding_boxes against the painting boxes, on
    the device at full size, beside the reference chain on the same maps.  IoU within IOU_BOUND; ATS within 1e-6 for every scene whose
    reference IoU matrix keeps 1e-4 from the thresholds (the rule of test_gpu_box_fit.py); and splitting pays on the device as well."""
    from driving_dirty_amd import ops
    scenes = [sp.contact_pairs(seed) for seed in sp.CONTACT_SCENE_SEEDS]
    targets = [torch.from_numpy(s).to(dev) for s in scenes]
    maps = ops.boxes_to_binary_map(targets)
    masks = maps.cpu().numpy() > 0.5
    boxes, counts = ops.component_boxes(maps, 0.5, 1, 64, fit="oriented", pad_px=0.0, split_px=4, grow_iters=8)
    plain, plain_counts = ops.component_boxes(maps, 0.5, 1, 64, fit="oriented", pad_px=0.0)
    counts, plain_counts = counts.cpu().tolist(), plain_counts.cpu().tolist()
    preds = [boxes[i, :c] for i, c in enumerate(counts)]
    got_ats = ops.ats_bounding_boxes(preds, targets).cpu().double().numpy()
    plain_ats = ops.ats_bounding_boxes([plain[i, :c] for i, c in enumerate(plain_counts)], targets).cpu().double().numpy()
    qualifying, worst_iou, worst_ats, worst_ulp = 0, 0.0, 0.0, 0.0
    for i, s in enumerate(scenes):
        want_boxes, _ = sp.fit_regions(sp.split(masks[i], 4, 8), 1, 0.0)
        assert counts[i] == len(want_boxes) <= 64 and counts[i] > plain_counts[i]
        worst_ulp = max(worst_ulp, fit.ulp_distance(preds[i].cpu().numpy(), want_boxes))
        want = ref.iou_matrix(want_boxes, s)
        got = ops.box_iou(preds[i], targets[i]).cpu().double().numpy()
        worst_iou = max(worst_iou, float(np.abs(got - want).max()))
        if ref.threshold_margin(want) >= 1e-4:
            qualifying += 1
            worst_ats = max(worst_ats, abs(got_ats[i] - ref.ats_from_iou(want)))
    print(f"contact round trip: corners {worst_ulp:.2f} ulp, IoU {worst_iou:.3e} (bound {IOU_BOUND:.3e}), ATS {worst_ats:.3e} over {qualifying} of "
          f"{len(scenes)} scenes; ATS split {np.round(got_ats, 4)}, unsplit {np.round(plain_ats, 4)}")
    assert worst_ulp <= ULP_BOUND
    assert worst_iou <= IOU_BOUND
    assert 4 * qualifying >= 3 * len(scenes), qualifying
    assert worst_ats <= 1e-6
    assert plain_ats.max() < got_ats.min()


# ------------------------------------------------------------------------------------------------ 7. module surface
def test_module_surface(dev):
    from argparse import Namespace
    from driving_dirty_amd import ops
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.spatial import boxes_from_map
    b = 2
    plain = build_model(dev, box_metrics=True)
    views, road = synth.camera_batch(b, seed=17).to(dev), synth.road_maps(b, seed=17).to(dev)
    targets = [synth.car_boxes(n, seed=3 + n) for n in (12, 5)]
    batch = (tuple(views), tuple({"bounding_box": t} for t in targets), tuple(road))
    rm = road.float().unsqueeze(1)
    with torch.no_grad():
        pred = plain(views, rm)
    thr = float(pred.median())          # an untrained head's output is no use at 0.5, and the extraction is what is under test
    cap = 8192
    got = plain.predict_boxes(views, rm, threshold=thr, min_pixels=6, max_boxes=cap, split_px=4)
    raw, counts = ops.component_boxes(pred.contiguous(), thr, 6, cap, split_px=4, grow_iters=8)
    assert isinstance(got, tuple) and len(got) == b and int(counts.min()) > 0
    for i in range(b):
        n = min(int(counts[i]), cap)
        assert tuple(got[i].shape) == (n, 2, 4) and torch.equal(got[i], raw[i, :n]) and not got[i].requires_grad
    unsplit = plain.predict_boxes(views, rm, threshold=thr, min_pixels=6, max_boxes=cap)
    assert any(a.shape != b_.shape or not torch.equal(a, b_) for a, b_ in zip(got, unsplit))
    oriented = plain.predict_boxes(views, rm, threshold=thr, min_pixels=6, max_boxes=cap, fit="oriented", split_px=4, grow_iters=2)
    want = boxes_from_map(pred, thr, 6, cap, fit="oriented", split_px=4, grow_iters=2)
    assert all(tuple(a.shape[1:]) == (2, 4) and torch.equal(a, w) for a, w in zip(oriented, want))

    joint = JointRoadMapBBox(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=16, latent_dim=8)), unfreeze_epoch_no=0, learning_rate=1e-3,
                                       output_img_freq=500))
    synth.fill_module(joint, seed=29)
    joint = joint.to(dev)
    joint.ae.encoder.fc1.drop_p = joint.ae.encoder.fc2.drop_p = 0.0
    with torch.no_grad():
        jmap = joint(views, rm)[1]
    jthr = float(jmap.median())
    jgot = joint.predict_boxes(views, rm, threshold=jthr, min_pixels=6, max_boxes=cap, split_px=4)
    jwant = boxes_from_map(jmap, jthr, 6, cap, split_px=4)
    assert len(jgot) == b and all(g.dim() == 3 and tuple(g.shape[1:]) == (2, 4) and g.shape[0] > 0 and torch.equal(g, w) for g, w in zip(jgot, jwant))

    # validation_step: box_split_px absent == 0, bit for bit; 4 == the ops by hand on the step's own maps
    assert not hasattr(plain.hparams, "box_split_px") and not hasattr(plain.hparams, "box_grow_iters")
    out_plain = plain.validation_step(batch, 0)
    plain.hparams.box_split_px = 0
    out_zero = plain.validation_step(batch, 0)
    plain.hparams.box_split_px = 4
    out_split = plain.validation_step(batch, 0)
    assert set(out_plain) == set(out_zero) == set(out_split) == {"val_loss", "val_ats", "val_ts"}
    for k in out_plain:
        assert torch.equal(out_plain[k], out_zero[k])
    assert torch.equal(out_plain["val_loss"], out_split["val_loss"]) and torch.equal(out_plain["val_ts"], out_split["val_ts"])
    with torch.no_grad():
        _, _, pred_flat = plain._run_step(batch, 0, step_name="valid")
        hand_boxes, hand_counts = ops.component_boxes(pred_flat.reshape(b, 800, 800).contiguous(), 0.5, 1, 256, split_px=4, grow_iters=8)
        hand_ats = ops.ats_bounding_boxes([hand_boxes[i, :min(int(hand_counts[i]), 256)] for i in range(b)], targets).mean()
    assert out_split["val_ats"].dim() == 0 and torch.equal(out_split["val_ats"], hand_ats)
    plain.hparams.box_grow_iters = 17
    from driving_dirty_amd import _lib
    with pytest.raises(_lib.HotpathError):
        plain.validation_step(batch, 0)
