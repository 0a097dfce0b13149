"""The oriented box fit on the device (csrc/boxeval.hip: dd_component_obb, ops.component_boxes(fit="oriented")) against the fp64 CPU
reference of tests/_box_fit_ref.py, and the module surface built on it (predict_boxes(fit=...), hparams.box_fit / box_pad_px).

Moments, counts and order are compared exactly.  Corners: the device and the host evaluate the same fp64 expression on identical
integers, so they differ only by the last bits of atan2 / sin / cos (about 1e-13 px) and then by the single rounding to fp32: the bound
is ONE fp32 ulp of the coordinate (np.spacing of the larger magnitude; 3.8e-6 m at 40 m), derived, not tuned."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import _box_eval_ref as ref
import _box_fit_ref as fit

from driving_dirty_amd import synth
from test_gpu_box_eval import IOU_BOUND, build_model, random_mask, spiral

pytestmark = pytest.mark.gpu

# Worst corner difference from the reference over every comparison of this file, in fp32 ulps of the coordinate, measured on an MI355X
# (each test prints its own): ULP_MEASURED = 0, every one of the 3.4 million coordinates bit-identical -- a difference needs the fp64
# value to lie within ~1e-13 px of an fp32 rounding boundary.  The asserted bound is ULP_BOUND = 1, whatever was measured.
ULP_MEASURED = 0.0
ULP_BOUND = 1.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def ref_fit(masks, min_pixels, max_boxes, pad_px):
    b = masks.shape[0]
    boxes = np.zeros((b, max_boxes, 2, 4), dtype=np.float32)
    moments = np.zeros((b, max_boxes, 6), dtype=np.int64)
    counts = np.zeros(b, dtype=np.int32)
    for i, m in enumerate(masks):
        bx, mo, _ = fit.fit_components(m, min_pixels, pad_px)
        counts[i] = len(bx)
        n = min(len(bx), max_boxes)
        boxes[i, :n], moments[i, :n] = bx[:n], mo[:n]
    return boxes, counts, moments


def gpu_fit(masks, dev, min_pixels, max_boxes, pad_px, threshold=0.5):
    from driving_dirty_amd import ops
    maps = torch.from_numpy(np.ascontiguousarray(masks, dtype=np.float32)).to(dev)
    boxes, counts, moments = ops.component_boxes(maps, threshold, min_pixels, max_boxes, fit="oriented", pad_px=pad_px, want_moments=True)
    assert boxes.dtype == torch.float32 and tuple(boxes.shape) == (masks.shape[0], max_boxes, 2, 4)
    assert counts.dtype == torch.int32 and moments.dtype == torch.int64 and tuple(moments.shape) == (masks.shape[0], max_boxes, 6)
    extent_boxes, extent_counts = ops.component_boxes(maps, threshold, min_pixels, max_boxes)
    assert torch.equal(counts, extent_counts)                                      # the same survivors as the extent path
    return boxes.cpu().numpy(), counts.cpu().numpy(), moments.cpu().numpy(), extent_boxes.cpu().numpy()


def check_against_reference(masks, dev, min_pixels, max_boxes, pad_px, what):
    boxes, counts, moments, extent_boxes = gpu_fit(masks, dev, min_pixels, max_boxes, pad_px)
    want_boxes, want_counts, want_moments = ref_fit(masks, min_pixels, max_boxes, pad_px)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(moments, want_moments)                                   # exact int64, order included; zero past the count
    h, w = masks.shape[1:]
    for i in range(masks.shape[0]):
        n = min(int(counts[i]), max_boxes)
        # the same order as the extent path: the centroid of box k lies inside the extent path's box k
        e = extent_boxes[i, :n].astype(np.float64)
        c0, c1 = np.round(e[:, 0].min(axis=1) * 10 + w / 2), np.round(e[:, 0].max(axis=1) * 10 + w / 2) - 1
        r0, r1 = np.round(h / 2 - e[:, 1].max(axis=1) * 10), np.round(h / 2 - e[:, 1].min(axis=1) * 10) - 1
        cnt, sx, sy = moments[i, :n, 0], moments[i, :n, 1], moments[i, :n, 2]
        assert np.all(cnt * c0 <= sx) and np.all(sx <= cnt * c1) and np.all(cnt * r0 <= sy) and np.all(sy <= cnt * r1)
        assert not boxes[i, n:].any()
    worst = fit.ulp_distance(boxes, want_boxes)
    same = float((boxes == want_boxes).mean())
    print(f"{what}: {int(np.minimum(counts, max_boxes).sum())} boxes, worst corner difference {worst:.2f} fp32 ulp, {same:.6f} of the coordinates "
          f"bit-identical (bound {ULP_BOUND} ulp)")
    assert worst <= ULP_BOUND
    return boxes, counts, moments


# ------------------------------------------------------------------------------------------------ 4. / 5. moments, counts, order, corners
@pytest.mark.parametrize("shape,density,min_pixels,max_boxes", [((1, 5, 7), 0.4, 1, 16), ((2, 130, 257), 0.5, 4, 2048), ((2, 130, 257), 0.3, 1, 8192),
                                                                 ((2, 130, 257), 0.62, 1, 4096), ((4, 800, 800), 0.55, 12, 8192),
                                                                 ((4, 800, 800), 0.02, 1, 16384), ((4, 800, 800), 0.4, 2, 65536)])
@pytest.mark.parametrize("pad_px", [0.5, 0.0])
def test_oriented_boxes_equal_the_reference(dev, shape, density, min_pixels, max_boxes, pad_px):
    masks = random_mask(shape, density, seed=shape[2] + min_pixels)
    _, counts, _ = check_against_reference(masks, dev, min_pixels, max_boxes, pad_px, f"random {shape} density {density}")
    assert counts.max() <= max_boxes and counts.min() > 0


def straddling_masks():
    """Components across 32 x 32 tile corners and across the ends of the 64-pixel row segments the run kernels work on."""
    h, w = 130, 257
    m = np.zeros((4, h, w), dtype=bool)
    for y in range(32, h, 32):
        for x in range(32, w, 32):
            m[0, y - 1:y + 1, x - 1:x + 1] = True                                  # 2 x 2 block, one pixel in each of four tiles
            m[1, y - 2:y + 2, x] = m[1, y, x - 2:x + 2] = True                       # a cross through the corner
    m[1, 0, :] = m[1, :, 0] = True                                                 # a frame that joins nothing to them
    for k, (x0, x1) in enumerate([(60, 70), (63, 64), (0, 256), (64, 127), (1, 191), (127, 129), (192, 256), (63, 63), (64, 64), (100, 230)]):
        m[2, 3 * k + 1, x0:x1 + 1] = True                                          # single-row runs that end on, before and after a segment end
    m[2, 40:44, 30:200] = True                                                     # a block of runs over three segments
    for i in range(80):                                                            # slanted bars, two pixels thick, over tile and segment borders
        m[3, 5 + i, 20 + 2 * i:24 + 2 * i] = True
        m[3, 120 - i, 150 + i:153 + i] = True
    m[3, 20:110, 250] = True                                                       # a vertical line: every run has one pixel
    return m


@pytest.mark.parametrize("pad_px", [0.5, 0.0])
def test_components_that_straddle_tiles_and_segments(dev, pad_px):
    m = straddling_masks()
    _, counts, moments = check_against_reference(m, dev, 1, 256, pad_px, "straddling")
    assert counts.tolist() == [4 * 8, 4 * 8 + 1, 11, 3]
    assert moments[2, 2, 0] == 257 and moments[3, :3, 0].tolist() == [320, 90, 240]
    check_against_reference(m, dev, 5, 256, pad_px, "straddling, min_pixels 5")


def test_overflow_is_reported_and_nothing_is_written_past_the_cap(dev):
    from driving_dirty_amd import _lib, ops
    from driving_dirty_amd.ops import _p, _stream
    b, h, w, max_boxes, guard = 3, 64, 64, 5, 4096
    masks = random_mask((b, h, w), 0.3, seed=9)
    masks[1] = False
    masks[1, 10:12, 10:20] = True                                                  # sample 1: one component, no overflow
    want_boxes, want_counts, want_moments = ref_fit(masks, 1, max_boxes, 0.5)
    assert want_counts[0] > max_boxes and want_counts[2] > max_boxes and want_counts[1] == 1
    maps = torch.from_numpy(masks.astype(np.float32)).to(dev)
    buf = torch.full((b * max_boxes * 8 + guard,), -7.0, device=dev)
    mom = torch.full((b * max_boxes * 6 + guard,), -7, device=dev, dtype=torch.int64)
    counts = torch.full((b + 64,), -7, device=dev, dtype=torch.int32)
    nbytes = _lib.lib().dd_component_obb_workspace_bytes(b, h, w, max_boxes)
    ws = torch.empty(nbytes + guard, device=dev, dtype=torch.uint8)
    ws[nbytes:] = 0x5a
    _lib.check(_lib.lib().dd_component_obb(_p(maps), 0.5, 1, max_boxes, 0.5, _p(buf), _p(counts), _p(mom), b, h, w, _p(ws), nbytes, _stream()),
               "dd_component_obb")
    got, got_m = buf.cpu(), mom.cpu()
    assert torch.all(got[b * max_boxes * 8:] == -7.0) and torch.all(got_m[b * max_boxes * 6:] == -7) and torch.all(counts[b:].cpu() == -7)
    assert torch.all(ws[nbytes:].cpu() == 0x5a)                                    # nor past the workspace
    assert np.array_equal(counts[:b].cpu().numpy(), want_counts)                  # uncapped
    got = got[:b * max_boxes * 8].reshape(b, max_boxes, 2, 4).numpy()
    got_m = got_m[:b * max_boxes * 6].reshape(b, max_boxes, 6).numpy()
    for i in (0, 2):
        assert fit.ulp_distance(got[i], want_boxes[i]) <= ULP_BOUND and np.array_equal(got_m[i], want_moments[i])
    assert fit.ulp_distance(got[1, :1], want_boxes[1, :1]) <= ULP_BOUND and np.array_equal(got_m[1, :1], want_moments[1, :1])
    assert np.all(got[1, 1:] == -7.0) and np.all(got_m[1, 1:] == -7)               # the slots beyond the count: left as they were
    # moments = NULL is allowed, and the Python op gives zero rows past the count
    buf2 = torch.full_like(buf, -7.0)
    _lib.check(_lib.lib().dd_component_obb(_p(maps), 0.5, 1, max_boxes, 0.5, _p(buf2), _p(counts), None, b, h, w, _p(ws), nbytes, _stream()),
               "dd_component_obb")
    assert torch.equal(buf2, buf)
    boxes, counts2 = ops.component_boxes(maps, 0.5, 1, max_boxes, fit="oriented")
    assert np.array_equal(counts2.cpu().numpy(), want_counts) and not boxes[1, 1:].any()
    assert np.array_equal(boxes.cpu().numpy()[0], got[0])


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_two_launches_are_bit_identical_and_samples_are_independent(dev):
    from driving_dirty_amd import ops
    masks = np.concatenate([random_mask((2, 800, 800), 0.58, seed=1), spiral(800)[None]])
    maps = torch.from_numpy(masks.astype(np.float32)).to(dev)
    first = ops.component_boxes(maps, 0.5, 2, 8192, fit="oriented", want_moments=True)
    again = ops.component_boxes(maps, 0.5, 2, 8192, fit="oriented", want_moments=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert int(first[1][2]) == 1 and int(first[2][2, 0, 0]) == int(masks[2].sum())      # the spiral: one component of ~320000 pixels
    for i in (0, 2):
        alone = ops.component_boxes(maps[i:i + 1], 0.5, 2, 8192, fit="oriented", want_moments=True)
        assert all(torch.equal(a[0], w[i]) for a, w in zip(alone, first))
    flipped = ops.component_boxes(maps.flip(0).contiguous(), 0.5, 2, 8192, fit="oriented", want_moments=True)
    assert all(torch.equal(a.flip(0), w) for a, w in zip(flipped, first))


# ------------------------------------------------------------------------------------------------ 7. edge cases
def test_background_foreground_one_pixel_and_nan(dev):
    from driving_dirty_amd import ops
    for shape in [(2, 5, 7), (2, 130, 257), (1, 800, 800)]:
        b, h, w = shape
        boxes, counts, moments = ops.component_boxes(torch.zeros(shape, device=dev), 0.5, 1, 8, fit="oriented", want_moments=True)
        assert counts.cpu().tolist() == [0] * b and not boxes.any() and not moments.any()
        boxes, counts, moments = check_against_reference(np.ones(shape, dtype=bool), dev, 1, 8, 0.5, f"all foreground {shape}")
        assert counts.tolist() == [1] * b
        n = h * w
        assert moments[0, 0].tolist() == [n, h * (w - 1) * w // 2, w * (h - 1) * h // 2, h * (w - 1) * w * (2 * w - 1) // 6,
                                          ((w - 1) * w // 2) * ((h - 1) * h // 2), w * (h - 1) * h * (2 * h - 1) // 6]
        # the whole map: theta = 0 (wide or square), the box is the map's outline, as a corner set
        assert fit.ulp_distance(np.array(fit.corner_set(boxes[0, 0])), np.array(fit.corner_set(ref.extent_to_box(0, w - 1, 0, h - 1, h, w)))) <= ULP_BOUND
    # one pixel: theta = 0, the pixel's square at pad_px = 0.5 and a point at 0
    m = np.zeros((1, 800, 800), dtype=bool)
    m[0, 123, 677] = True
    boxes, counts, moments = check_against_reference(m, dev, 1, 4, 0.5, "one pixel")
    assert counts.tolist() == [1] and moments[0, 0].tolist() == [1, 677, 123, 677 * 677, 677 * 123, 123 * 123]
    assert fit.ulp_distance(np.array(fit.corner_set(boxes[0, 0])), np.array(fit.corner_set(ref.extent_to_box(677, 677, 123, 123, 800, 800)))) <= ULP_BOUND
    boxes, _, _ = check_against_reference(m, dev, 1, 4, 0.0, "one pixel, pad 0")
    assert np.all(boxes[0, 0, 0] == boxes[0, 0, 0, 0]) and np.all(boxes[0, 0, 1] == boxes[0, 0, 1, 0])
    # foreground is map > threshold, strictly; NaN is background
    vals = torch.tensor([[[0.2, 0.5, 0.7, float("nan"), 0.9, 0.8]]], device=dev)
    _, counts, moments = ops.component_boxes(vals, 0.5, 1, 4, fit="oriented", want_moments=True)
    assert counts.cpu().tolist() == [2] and moments[0, :2, :2].cpu().tolist() == [[1, 2], [2, 9]]
    _, counts, moments = ops.component_boxes(vals, 0.1, 1, 4, fit="oriented", want_moments=True)
    assert counts.cpu().tolist() == [2] and moments[0, :2, :2].cpu().tolist() == [[3, 3], [2, 9]]
    with pytest.raises(ValueError):
        ops.component_boxes(vals, fit="calipers")


# ------------------------------------------------------------------------------------------------ 8. round trip
@pytest.mark.parametrize("pad_px", [0.5, 0.0])
def test_round_trip_of_rotated_cars(dev, pad_px):
    """Rotated cars -> ops.boxes_to_binary_map -> component_boxes(fit="oriented") -> ops.ats_bounding_boxes against the painting boxes,
    on the device at full size.  The IoU matrices agree with the reference's within IOU_BOUND; the ATS within 1e-6 for every scene
    whose reference IoU matrix keeps 1e-4 from the thresholds -- and at least three quarters of the scenes must be such scenes
    (test_box_fit_ref.py checks, on the reference alone, that these seeds meet that)."""
    from driving_dirty_amd import ops
    scenes = [fit.car_scene(seed) for seed in fit.CAR_SCENE_SEEDS]
    targets = [torch.from_numpy(s).to(dev) for s in scenes]
    maps = ops.boxes_to_binary_map(targets)
    boxes, counts = ops.component_boxes(maps, 0.5, 1, 64, fit="oriented", pad_px=pad_px)
    assert counts.cpu().tolist() == [len(s) for s in scenes]                       # nothing merged, nothing lost
    masks = maps.cpu().numpy() > 0.5
    want_boxes, _, _ = ref_fit(masks, 1, 64, pad_px)
    worst_ulp = fit.ulp_distance(boxes.cpu().numpy(), want_boxes)
    preds = [boxes[i, :len(s)] for i, s in enumerate(scenes)]
    got_ats = ops.ats_bounding_boxes(preds, targets).cpu().double().numpy()
    extent_boxes, _ = ops.component_boxes(maps, 0.5, 1, 64)
    extent_ats = ops.ats_bounding_boxes([extent_boxes[i, :len(s)] for i, s in enumerate(scenes)], targets).cpu().double().numpy()
    qualifying, worst_iou, worst_ats = 0, 0.0, 0.0
    for i, s in enumerate(scenes):
        want = ref.iou_matrix(want_boxes[i, :len(s)], s)
        got = ops.box_iou(preds[i], targets[i]).cpu().double().numpy()
        worst_iou = max(worst_iou, float(np.abs(got - want).max()))
        assert float(want.max(axis=0).min()) > 0.5
        if ref.threshold_margin(want) >= 1e-4:
            qualifying += 1
            worst_ats = max(worst_ats, abs(got_ats[i] - ref.ats_from_iou(want)))
    print(f"round trip pad_px {pad_px}: corners {worst_ulp:.2f} ulp, IoU {worst_iou:.3e} (bound {IOU_BOUND:.3e}), ATS {worst_ats:.3e} over {qualifying} of "
          f"{len(scenes)} scenes; ATS oriented {got_ats.mean():.4f}, extent {extent_ats.mean():.4f}")
    assert worst_ulp <= ULP_BOUND
    assert worst_iou <= IOU_BOUND
    assert 4 * qualifying >= 3 * len(scenes), qualifying
    assert worst_ats <= 1e-6
    assert np.all(got_ats >= 2.0 * extent_ats)                                     # what the fit is for, on the device too


# ------------------------------------------------------------------------------------------------ 9. module surface
def test_module_surface(dev):
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
    cap = 4096
    got = plain.predict_boxes(views, rm, threshold=thr, min_pixels=6, max_boxes=cap, fit="oriented")
    want = boxes_from_map(pred, thr, 6, cap, fit="oriented")
    raw, counts = ops.component_boxes(pred.contiguous(), thr, 6, cap, fit="oriented")
    assert isinstance(got, tuple) and len(got) == b and int(counts.min()) > 0
    for i in range(b):
        n = min(int(counts[i]), cap)
        assert tuple(got[i].shape) == (n, 2, 4) and torch.equal(got[i], want[i]) and torch.equal(got[i], raw[i, :n])
        assert not got[i].requires_grad
    # the default is the extent fit, and pad_px reaches the kernel
    default = plain.predict_boxes(views, rm, threshold=thr, min_pixels=6, max_boxes=cap)
    assert all(torch.equal(a, b_) for a, b_ in zip(default, plain.predict_boxes(views, rm, threshold=thr, min_pixels=6, max_boxes=cap, fit="extent")))
    assert not torch.equal(default[0], got[0])
    tight = plain.predict_boxes(views, rm, threshold=thr, min_pixels=6, max_boxes=cap, fit="oriented", pad_px=0.0)
    assert tight[0].shape == got[0].shape and not torch.equal(tight[0], got[0])
    with pytest.raises(ValueError):
        plain.predict_boxes(views, rm, fit="calipers")

    # the joint model: its box head's map
    joint = JointRoadMapBBox(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=16, latent_dim=8)), unfreeze_epoch_no=0, learning_rate=1e-3,
                                       output_img_freq=500))
    synth.fill_module(joint, seed=29)
    joint = joint.to(dev)
    joint.ae.encoder.fc1.drop_p = joint.ae.encoder.fc2.drop_p = 0.0
    with torch.no_grad():
        jmap = joint(views, rm)[1]
    jthr = float(jmap.median())
    jgot = joint.predict_boxes(views, rm, threshold=jthr, min_pixels=6, max_boxes=cap, fit="oriented")
    jwant = boxes_from_map(jmap, jthr, 6, cap, fit="oriented")
    assert len(jgot) == b and all(g.dim() == 3 and tuple(g.shape[1:]) == (2, 4) and g.shape[0] > 0 and torch.equal(g, w) for g, w in zip(jgot, jwant))
    with pytest.raises(ValueError):
        joint.predict_boxes(views, rm, fit="calipers")

    # validation_step: box_fit absent == "extent", bit for bit; "oriented" == the ops by hand on the step's own maps
    assert not hasattr(plain.hparams, "box_fit") and not hasattr(plain.hparams, "box_pad_px")
    out_plain = plain.validation_step(batch, 0)
    plain.hparams.box_fit = "extent"
    out_extent = plain.validation_step(batch, 0)
    plain.hparams.box_fit, plain.hparams.box_pad_px = "oriented", 0.0
    out_oriented = plain.validation_step(batch, 0)
    assert set(out_plain) == set(out_extent) == set(out_oriented) == {"val_loss", "val_ats", "val_ts"}
    for k in out_plain:
        assert torch.equal(out_plain[k], out_extent[k])
    assert torch.equal(out_plain["val_loss"], out_oriented["val_loss"]) and torch.equal(out_plain["val_ts"], out_oriented["val_ts"])
    with torch.no_grad():
        _, _, pred_flat = plain._run_step(batch, 0, step_name="valid")
        hand_boxes, hand_counts = ops.component_boxes(pred_flat.reshape(b, 800, 800).contiguous(), 0.5, 1, 256, fit="oriented", pad_px=0.0)
        hand_sets = [hand_boxes[i, :min(int(hand_counts[i]), 256)] for i in range(b)]
        hand_ats = ops.ats_bounding_boxes(hand_sets, targets).mean()
    assert out_oriented["val_ats"].dim() == 0 and torch.equal(out_oriented["val_ats"], hand_ats)
    plain.hparams.box_fit = "calipers"
    with pytest.raises(ValueError):
        plain.validation_step(batch, 0)
