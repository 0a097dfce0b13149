"""Box-level validation on the device (csrc/boxeval.hip: dd_label_components, dd_component_boxes, dd_box_iou_ats) against the
independent fp64 CPU reference of tests/_box_eval_ref.py (scipy labelling; hull -> clip -> shoelace IoU; transcribed ATS), and the
module surface built on them (BBSpatialRoadMap.predict_boxes, hparams.box_metrics)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import _box_eval_ref as ref

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

# Worst |IoU - fp64 reference| over the sets of test_iou_matrix_against_reference, measured on an MI355X: 2.451e-8 -- the kernel works
# in fp64 and stores fp32, so this is the one rounding of the stored result (half an ulp just below 1 is 2^-25 = 2.98e-8).  The bound is
# four times the measured value, far inside the 1e-4 that would let a threshold decision flip in test_ats_against_reference.
IOU_MEASURED = 2.451e-8
IOU_BOUND = 4 * IOU_MEASURED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def random_mask(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def ref_labels(masks):
    return np.stack([ref.label(m) for m in masks])


def gpu_labels(masks, dev, threshold=0.5):
    from driving_dirty_amd import ops
    out = ops.label_components(torch.from_numpy(np.ascontiguousarray(masks, dtype=np.float32)).to(dev), threshold)
    assert out.dtype == torch.int32 and tuple(out.shape) == tuple(masks.shape)
    return out.cpu().numpy()


def spiral(n):
    """One 4-connected path that winds inwards with a one-pixel gap: a single component with a path of ~n*n/2 pixels."""
    m = np.zeros((n, n), dtype=bool)
    r = c = 0
    dr, dc = 0, 1
    m[0, 0] = True
    while True:
        moved = False
        while True:
            nr, nc, fr, fc = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if not (0 <= nr < n and 0 <= nc < n) or m[nr, nc] or (0 <= fr < n and 0 <= fc < n and m[fr, fc]):
                break
            r, c = nr, nc
            m[r, c] = True
            moved = True
        if not moved:
            return m
        dr, dc = dc, -dr


# ------------------------------------------------------------------------------------------------ 1. labels
@pytest.mark.parametrize("density", [0.1, 0.45, 0.6, 0.9])
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 64, 64), (2, 130, 257), (4, 800, 800)])
def test_labels_equal_the_reference(dev, shape, density):
    masks = random_mask(shape, density, seed=int(density * 100) + shape[1])
    got = gpu_labels(masks, dev)
    assert np.array_equal(got, ref_labels(masks))


def test_labels_all_background_all_foreground_and_threshold(dev):
    for shape in [(2, 5, 7), (2, 130, 257), (1, 800, 800)]:
        assert not gpu_labels(np.zeros(shape, dtype=bool), dev).any()
        assert np.array_equal(gpu_labels(np.ones(shape, dtype=bool), dev), np.ones(shape, dtype=np.int32))
    # foreground is map > threshold, strictly; NaN is background
    from driving_dirty_amd import ops
    vals = torch.tensor([[[0.2, 0.5, 0.7, float("nan"), 0.9]]], device=dev)
    assert ops.label_components(vals, 0.5).cpu().tolist() == [[[0, 0, 3, 0, 5]]]
    assert ops.label_components(vals, 0.1).cpu().tolist() == [[[1, 1, 1, 0, 5]]]


def test_labels_of_a_spiral(dev):
    m = spiral(800)
    assert m.sum() > 300000 and ref.components(m)[0][1] == m.sum()          # one component
    masks = np.stack([m, m[::-1].copy(), m.T.copy()[:, ::-1]])
    got = gpu_labels(masks, dev)
    assert np.array_equal(got, ref_labels(masks))
    assert np.array_equal(np.unique(got[0]), [0, 1])


def test_labels_of_components_that_straddle_tile_corners(dev):
    h, w = 130, 257
    m = np.zeros((2, h, w), dtype=bool)
    for y in range(32, h, 32):
        for x in range(32, w, 32):
            m[0, y - 1:y + 1, x - 1:x + 1] = True                                  # 2 x 2 block, one pixel in each of four tiles
            m[1, y - 2:y + 2, x] = m[1, y, x - 2:x + 2] = True                       # a cross through the corner
    m[1, 0, :] = m[1, :, 0] = True                                                 # and a frame that joins nothing to them
    got = gpu_labels(m, dev)
    assert np.array_equal(got, ref_labels(m))
    assert len(np.unique(got[0])) == 1 + 4 * 8


def test_labels_do_not_depend_on_the_rest_of_the_batch(dev):
    masks = random_mask((5, 130, 257), 0.55, seed=77)
    whole = gpu_labels(masks, dev)
    for i in (0, 3):
        assert np.array_equal(gpu_labels(masks[i:i + 1], dev)[0], whole[i])
    assert np.array_equal(gpu_labels(masks[::-1].copy(), dev)[::-1], whole)


# ------------------------------------------------------------------------------------------------ 2. component boxes
def ref_boxes(masks, min_pixels, max_boxes):
    b = masks.shape[0]
    boxes = np.zeros((b, max_boxes, 2, 4), dtype=np.float32)
    counts = np.zeros(b, dtype=np.int32)
    for i, m in enumerate(masks):
        bx, n = ref.component_boxes(m, min_pixels)
        counts[i] = n
        boxes[i, :min(n, max_boxes)] = bx[:max_boxes]
    return boxes, counts


@pytest.mark.parametrize("shape,density,min_pixels,max_boxes", [((1, 5, 7), 0.4, 1, 16), ((3, 64, 64), 0.3, 1, 1024), ((3, 64, 64), 0.45, 3, 256),
                                                                 ((2, 130, 257), 0.5, 4, 2048), ((2, 800, 800), 0.55, 12, 8192),
                                                                 ((2, 800, 800), 0.02, 1, 16384)])
def test_component_boxes_equal_the_reference(dev, shape, density, min_pixels, max_boxes):
    from driving_dirty_amd import ops
    masks = random_mask(shape, density, seed=shape[2] + min_pixels)
    boxes, counts = ops.component_boxes(torch.from_numpy(masks.astype(np.float32)).to(dev), 0.5, min_pixels, max_boxes)
    want_boxes, want_counts = ref_boxes(masks, min_pixels, max_boxes)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), want_counts)
    assert want_counts.max() <= max_boxes and want_counts.min() > 0
    assert boxes.dtype == torch.float32 and torch.equal(boxes.cpu(), torch.from_numpy(want_boxes))      # counts, order and extents, bit for bit


def test_component_boxes_overflow_is_reported_and_nothing_is_written_past_the_buffer(dev):
    from driving_dirty_amd import _lib, ops
    from driving_dirty_amd.ops import _p, _stream
    b, h, w, max_boxes, guard = 3, 64, 64, 5, 4096
    masks = random_mask((b, h, w), 0.3, seed=9)
    masks[1] = False
    masks[1, 10:12, 10:20] = True                                                  # sample 1: one component, no overflow
    want_boxes, want_counts = ref_boxes(masks, 1, max_boxes)
    assert want_counts[0] > max_boxes and want_counts[2] > max_boxes and want_counts[1] == 1
    maps = torch.from_numpy(masks.astype(np.float32)).to(dev)
    # the C entry point on a buffer with a guard region behind it (and a sentinel in the rows it must leave alone)
    buf = torch.full((b * max_boxes * 8 + guard,), -7.0, device=dev)
    counts = torch.full((b + 64,), -7, device=dev, dtype=torch.int32)
    nbytes = _lib.lib().dd_component_boxes_workspace_bytes(b, h, w)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    _lib.check(_lib.lib().dd_component_boxes(_p(maps), 0.5, 1, max_boxes, _p(buf), _p(counts), b, h, w, _p(ws), nbytes, _stream()), "dd_component_boxes")
    got = buf.cpu()
    assert torch.all(got[b * max_boxes * 8:] == -7.0) and torch.all(counts[b:].cpu() == -7)
    assert np.array_equal(counts[:b].cpu().numpy(), want_counts)                  # uncapped
    got = got[:b * max_boxes * 8].reshape(b, max_boxes, 2, 4)
    assert torch.equal(got[0], torch.from_numpy(want_boxes[0])) and torch.equal(got[2], torch.from_numpy(want_boxes[2]))
    assert torch.equal(got[1, :1], torch.from_numpy(want_boxes[1, :1])) and torch.all(got[1, 1:] == -7.0)
    # the Python op: zero rows past the count, the same counts
    boxes, counts2 = ops.component_boxes(maps, 0.5, 1, max_boxes)
    assert torch.equal(boxes.cpu(), torch.from_numpy(want_boxes)) and np.array_equal(counts2.cpu().numpy(), want_counts)


# ------------------------------------------------------------------------------------------------ 3. IoU
def clustered(rng, n, maker):
    out = []
    while len(out) < n:
        centre = rng.uniform(-27, 27, 2)
        out.extend(maker(rng, min(8, n - len(out)), centre))
    return np.array(out)


def iou_sets():
    rng = np.random.default_rng(31)
    sets = []
    for k in range(2):
        a = np.concatenate([clustered(rng, 64, ref.random_rects), clustered(rng, 64, ref.random_convex_quads)])
        sets.append(a[rng.permutation(128)])
    # the same cluster centres on both sides, or nothing would overlap: redraw set 2 around set 1's boxes
    rng = np.random.default_rng(32)
    near = []
    for i in range(128):
        c = sets[0][i].mean(axis=1) + rng.uniform(-1.5, 1.5, 2)
        near.append((ref.random_rects if i % 2 else ref.random_convex_quads)(rng, 1, c)[0])
    return sets[0], np.array(near), sets[1]


def test_iou_matrix_against_reference(dev):
    """Up to 128 x 128 rotated rectangles and general convex quadrilaterals, coordinates within +-40, sides 0.5-6, both orientations,
    f64 and f32 inputs, plus the cases with known answers.  Measured on an MI355X: worst |difference| from the fp64 reference
    IOU_MEASURED = 2.451e-8 (the fp32 rounding of the stored result); asserted: IOU_BOUND = 4 x that = 9.8e-8 (cap: 1e-4)."""
    from driving_dirty_amd import ops
    assert IOU_BOUND <= 1e-4
    a, near, other = iou_sets()
    assert np.abs(np.concatenate([a, near, other])).max() <= 40.0
    worst = 0.0
    overlapping = 0
    for s1, s2 in ((a, near), (near[:77], a[:128]), (a[:50], other[:33])):
        for dtype in (torch.float64, torch.float32):
            t1, t2 = torch.from_numpy(s1).to(dtype), torch.from_numpy(s2).to(dtype)
            got = ops.box_iou(t1.to(dev), t2.to(dev))
            assert got.dtype == torch.float32 and tuple(got.shape) == (len(s1), len(s2))
            want = ref.iou_matrix(t1.double().numpy(), t2.double().numpy())        # the reference sees the inputs the kernel saw
            overlapping += int((want > 0.05).sum())
            worst = max(worst, float(np.abs(got.cpu().double().numpy() - want).max()))
    assert overlapping > 500
    exact = ref.exact_cases()
    e1, e2 = np.array([c[0] for c in exact]), np.array([c[1] for c in exact])
    got = ops.box_iou(torch.from_numpy(e1).to(dev), torch.from_numpy(e2).to(dev)).cpu().double().numpy()
    for k, (_, _, expected) in enumerate(exact):
        worst = max(worst, abs(got[k, k] - expected))
    assert got[0, 0] == 1.0 and got[3, 3] == 0.0 and got[4, 4] == 0.0
    worst = max(worst, float(np.abs(got - ref.iou_matrix(e1, e2)).max()))
    print(f"box_iou: worst |difference| from the fp64 reference {worst:.3e} (bound {IOU_BOUND:.3e})")
    assert worst <= IOU_BOUND


# ------------------------------------------------------------------------------------------------ 4. ATS
def ats_cases():
    rng = np.random.default_rng(404)
    cases, generated = [], 0
    while len(cases) < 24:
        generated += 1
        s1, s2 = ref.ats_pair(rng, int(rng.integers(1, 50)), int(rng.integers(0, 12)), int(rng.integers(0, 3)), int(rng.integers(0, 8)),
                              int(rng.integers(0, 8)))
        m = ref.iou_matrix(s1, s2)
        if ref.threshold_margin(m) < 1e-3:
            continue                                                               # discarded: an IoU too close to a threshold
        cases.append((s1, s2, m))
    return cases, generated


def test_ats_against_reference(dev):
    from driving_dirty_amd import ops
    from driving_dirty_amd.spatial import compute_ats_bounding_boxes
    cases, generated = ats_cases()
    assert (generated - len(cases)) * 20 <= generated, f"{generated - len(cases)} of {generated} pairs discarded"
    for _, _, m in cases:                                                          # with the reference alone: no decision can flip
        assert ref.threshold_margin(m) >= 1e-3
    assert len({len(s1) for s1, _, _ in cases}) > 5 and max(len(s2) for _, s2, _ in cases) >= 30
    empty = np.zeros((0, 2, 4))
    sets1 = [c[0] for c in cases] + [empty, cases[0][0], empty]
    sets2 = [c[1] for c in cases] + [cases[0][1], empty, empty]
    want = np.array([ref.ats_from_iou(c[2]) for c in cases] + [0.0, 0.0, 0.0])
    assert want.max() > 0.3 and len(np.unique(np.round(want, 6))) > 10
    for dtype in (torch.float64, torch.float32):
        got = ops.ats_bounding_boxes([torch.from_numpy(s).to(dtype).to(dev) for s in sets1], [torch.from_numpy(s).to(dtype).to(dev) for s in sets2])
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(sets1),)
        assert np.abs(got.cpu().double().numpy() - want).max() <= 1e-6
        assert got[-3:].cpu().tolist() == [0.0, 0.0, 0.0]                          # an empty set on either side scores 0
    # predictions on the device, targets on the host in f64, as a validation batch has them; and one sample at a time
    mixed = ops.ats_bounding_boxes([torch.from_numpy(s).float().to(dev) for s in sets1[:5]], [torch.from_numpy(s) for s in sets2[:5]])
    want5 = [ref.ats(torch.from_numpy(s).float().double().numpy(), t) for s, t in zip(sets1[:5], sets2[:5])]
    assert np.abs(mixed.cpu().double().numpy() - np.array(want5)).max() <= 1e-6
    one = compute_ats_bounding_boxes(torch.from_numpy(sets1[3]).to(dev), torch.from_numpy(sets2[3]).to(dev))
    assert one.dim() == 0 and one.is_cuda and abs(float(one) - want[3]) <= 1e-6


# ------------------------------------------------------------------------------------------------ 5. round trip
def separated_boxes(rng, n):
    """n axis-aligned boxes on a 10 m grid, 1.5-6 m sides, corners 0.02-0.08 m inside their pixels (never on a pixel boundary)."""
    cells = rng.permutation(49)[:n]
    out = np.zeros((n, 2, 4))
    for i, c in enumerate(cells):
        x0 = -33.0 + 10.0 * (c % 7) + rng.integers(0, 20) / 10 + rng.uniform(0.02, 0.08)
        y0 = -33.0 + 10.0 * (c // 7) + rng.integers(0, 20) / 10 + rng.uniform(0.02, 0.08)
        x1 = x0 + rng.integers(15, 60) / 10 + rng.uniform(0.0, 0.01)
        y1 = y0 + rng.integers(15, 60) / 10 + rng.uniform(0.0, 0.01)
        out[i] = [[x1, x1, x0, x0], [y1, y0, y1, y0]]
    return out


def test_round_trip_through_the_rasteriser(dev):
    from driving_dirty_amd import ops
    rng = np.random.default_rng(55)
    sources = [separated_boxes(rng, n) for n in (1, 7, 30, 49)]
    maps = ops.boxes_to_binary_map([torch.from_numpy(s).to(dev) for s in sources])
    boxes, counts = ops.component_boxes(maps, 0.5, 1, 64)
    assert counts.cpu().tolist() == [len(s) for s in sources]
    extracted = [boxes[i, :len(s)].cpu().numpy() for i, s in enumerate(sources)]
    for src, ext in zip(sources, extracted):
        # match each source to the extracted box that holds its centre; every extracted box is used once
        centres = src.mean(axis=2)
        owner = [int(np.flatnonzero((ext[:, 0].min(axis=1) <= cx) & (cx <= ext[:, 0].max(axis=1)) & (ext[:, 1].min(axis=1) <= cy)
                                    & (cy <= ext[:, 1].max(axis=1)))[0]) for cx, cy in centres]
        assert sorted(owner) == list(range(len(src)))
        for s, e in zip(src, ext[owner].astype(np.float64)):
            for axis in (0, 1):
                lo, hi, elo, ehi = s[axis].min(), s[axis].max(), e[axis].min(), e[axis].max()
                assert elo <= lo and ehi >= hi, (s, e)                             # contains its source ...
                assert lo - elo <= 0.1 + 1e-6 and ehi - hi <= 0.1 + 1e-6, (s, e)   # ... and exceeds it by at most one pixel per side
    got = ops.ats_bounding_boxes([boxes[i, :len(s)] for i, s in enumerate(sources)], [torch.from_numpy(s).to(dev) for s in sources])
    want = [ref.ats(e, s) for e, s in zip(extracted, sources)]
    assert np.abs(got.cpu().double().numpy() - np.array(want)).max() <= 1e-6
    assert min(want) > 0.2


# ------------------------------------------------------------------------------------------------ 6. module surface
def build_model(dev, **extra):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8))
    model = BBSpatialRoadMap(Namespace(pretrained_ae=ae, unfreeze_epoch_no=5, learning_rate=1e-3, output_img_freq=500, **extra))
    synth.fill_module(model, seed=17)
    return model.to(dev)


def test_module_surface(dev):
    from driving_dirty_amd import ops
    b = 2
    plain, flagged = build_model(dev), build_model(dev, box_metrics=True)
    views, road = synth.camera_batch(b, seed=17).to(dev), synth.road_maps(b, seed=17).to(dev)
    targets = [synth.car_boxes(n, seed=3 + n) for n in (12, 5)]
    batch = (tuple(views), tuple({"bounding_box": t} for t in targets), tuple(road))
    rm = road.float().unsqueeze(1)

    with torch.no_grad():
        pred = plain(views, rm)
    assert tuple(pred.shape) == (b, 800, 800)
    # a threshold at the map's median: an untrained head's output is no use at 0.5, and the extraction is what is under test
    thr = float(pred.median())
    cap = 4096
    boxes, counts = ops.component_boxes(pred.contiguous(), thr, 6, cap)
    assert int(counts.min()) > 0
    got = plain.predict_boxes(views, rm, threshold=thr, min_pixels=6, max_boxes=cap)
    assert isinstance(got, tuple) and len(got) == b
    for i in range(b):
        n = min(int(counts[i]), cap)
        assert tuple(got[i].shape) == (n, 2, 4) and torch.equal(got[i], boxes[i, :n])
        assert not got[i].requires_grad

    out_plain = plain.validation_step(batch, 0)
    out_flag = flagged.validation_step(batch, 0)
    assert set(out_plain) == {"val_loss"}                                          # the flag off: what the method always returned
    assert set(out_flag) == {"val_loss", "val_ats", "val_ts"}
    assert torch.equal(out_plain["val_loss"], out_flag["val_loss"])                # the same bits
    with torch.no_grad():                                                          # the ops by hand, on the step's own maps
        _, target_flat, pred_flat = plain._run_step(batch, 0, step_name="valid")
        hand_boxes, hand_counts = ops.component_boxes(pred_flat.reshape(b, 800, 800).contiguous(), 0.5, 1, 256)
        hand_sets = [hand_boxes[i, :min(int(hand_counts[i]), 256)] for i in range(b)]
        hand_ats = ops.ats_bounding_boxes(hand_sets, targets).mean()
        hand_ts = ops.threat_score(target_flat.contiguous(), pred_flat.contiguous(), round_b=True)
    assert torch.equal(target_flat.reshape(b, 800, 800), ops.boxes_to_binary_map(targets, dev))
    assert out_flag["val_ats"].dim() == 0 and torch.equal(out_flag["val_ats"], hand_ats)
    assert torch.equal(out_flag["val_ts"], hand_ts)
    end_plain = plain.validation_epoch_end([out_plain, out_plain])
    end_flag = flagged.validation_epoch_end([out_flag, out_flag])
    assert set(end_plain["log"]) == {"avg_val_loss"} and torch.equal(end_plain["val_loss"], end_flag["val_loss"])
    assert set(end_flag["log"]) == {"avg_val_loss", "avg_val_ats", "avg_val_ts"}
    assert torch.equal(end_flag["log"]["avg_val_ats"], out_flag["val_ats"]) and torch.equal(end_flag["log"]["avg_val_ts"], out_flag["val_ts"])


# ------------------------------------------------------------------------------------------------ 7. determinism
def test_two_launches_are_bit_identical(dev):
    from driving_dirty_amd import ops
    masks = np.concatenate([random_mask((2, 800, 800), 0.58, seed=1), spiral(800)[None]])
    maps = torch.from_numpy(masks.astype(np.float32)).to(dev)
    assert torch.equal(ops.label_components(maps), ops.label_components(maps))
    b1, c1 = ops.component_boxes(maps, 0.5, 2, 8192)
    b2, c2 = ops.component_boxes(maps, 0.5, 2, 8192)
    assert torch.equal(b1, b2) and torch.equal(c1, c2)
    a, near, _ = iou_sets()
    t1, t2 = torch.from_numpy(a).to(dev), torch.from_numpy(near).to(dev)
    assert torch.equal(ops.box_iou(t1, t2), ops.box_iou(t1, t2))
    s1, s2 = [t1[:40], t1[40:]], [t2[:50], t2[50:]]
    assert torch.equal(ops.ats_bounding_boxes(s1, s2), ops.ats_bounding_boxes(s1, s2))
