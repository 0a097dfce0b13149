"""CPU reference for the box-level validation ops (csrc/boxeval.hip): an independent fp64 restatement, numpy / scipy / plain Python.

* labelling: ``scipy.ndimage.label`` (default structure = 4-connectivity), relabelled to the canonical labels
  ``1 + raster index of the component's first pixel``; extents from ``scipy.ndimage.find_objects``.
* IoU of two [2,4] corner sets: convex hull (monotone chain) -> Sutherland-Hodgman clipping -> shoelace formula.  This is what
  reference src/utils/helper.py:79-83 asks shapely for (``Polygon(...).convex_hull``, ``intersection``, ``union``).
* ATS: helper.py:59-70 transcribed; an empty set on either side scores 0 (the reference raises there).

Also the seeded generators the GPU tests draw their boxes from.  Nothing here imports the package under test.
"""
import functools
import math

import numpy as np
from scipy import ndimage

THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)


# ------------------------------------------------------------------------------------------------ components
def label(mask):
    """bool [H,W] -> int32 [H,W]: 0 = background, else 1 + raster index of the first pixel of the pixel's 4-connected component."""
    mask = np.asarray(mask, dtype=bool)
    lab, n = ndimage.label(mask)
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    first = np.full(n + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat[idx], idx)
    out = np.zeros(flat.size, dtype=np.int32)
    out[idx] = first[flat[idx]] + 1
    return out.reshape(mask.shape)


def components(mask, min_pixels=1):
    """[(canonical label, pixels, c0, c1, r0, r1)] of the components with at least min_pixels pixels, ordered by label."""
    mask = np.asarray(mask, dtype=bool)
    lab, n = ndimage.label(mask)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    out = []
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        rows, cols = sl
        r0, r1, c0, c1 = rows.start, rows.stop - 1, cols.start, cols.stop - 1
        first_col = c0 + int(np.flatnonzero(lab[r0, c0:c1 + 1] == k)[0])
        if sizes[k] >= min_pixels:
            out.append((r0 * mask.shape[1] + first_col + 1, int(sizes[k]), c0, c1, r0, r1))
    return sorted(out)


def extent_to_box(c0, c1, r0, r1, h, w):
    """The [2,4] fp32 box of a pixel extent: each coordinate is ONE fp32 division of an exact multiple of 0.5 by 10."""
    f = np.float32
    xmin, xmax = f(c0 - w / 2) / f(10), f(c1 + 1 - w / 2) / f(10)
    ymin, ymax = f(h / 2 - 1 - r1) / f(10), f(h / 2 - r0) / f(10)
    return np.array([[xmax, xmax, xmin, xmin], [ymax, ymin, ymax, ymin]], dtype=np.float32)


def component_boxes(mask, min_pixels=1):
    """(boxes fp32 [n,2,4], n) for one map."""
    h, w = np.asarray(mask).shape
    comps = components(mask, min_pixels)
    boxes = np.zeros((len(comps), 2, 4), dtype=np.float32)
    for i, (_, _, c0, c1, r0, r1) in enumerate(comps):
        boxes[i] = extent_to_box(c0, c1, r0, r1, h, w)
    return boxes, len(comps)


# ------------------------------------------------------------------------------------------------ polygons
def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(points):
    """Andrew's monotone chain; counter-clockwise, collinear points dropped."""
    pts = sorted(set((float(x), float(y)) for x, y in points))
    if len(pts) <= 2:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def polygon_area(poly):
    if len(poly) < 3:
        return 0.0
    return 0.5 * sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1] for i in range(len(poly)))


def clip(subject, clipper):
    """Sutherland-Hodgman: the part of `subject` inside the convex counter-clockwise `clipper`."""
    out = list(subject)
    for i in range(len(clipper)):
        a, b = clipper[i], clipper[(i + 1) % len(clipper)]
        src, out = out, []
        if not src:
            break
        for j in range(len(src)):
            p, q = src[j], src[(j + 1) % len(src)]
            sp, sq = _cross(a, b, p), _cross(a, b, q)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def iou(box1, box2):
    """compute_iou (helper.py:79-83) of two [2,4] corner sets."""
    box1, box2 = np.asarray(box1, dtype=np.float64), np.asarray(box2, dtype=np.float64)
    # translate to box1's centroid: the fp64 reference itself should not spend digits on the +-40 m offset
    c = box1.mean(axis=1, keepdims=True)
    a, b = convex_hull((box1 - c).T), convex_hull((box2 - c).T)
    area_a, area_b = polygon_area(a), polygon_area(b)
    if area_a <= 0 or area_b <= 0:
        return 0.0
    inter = max(0.0, polygon_area(clip(a, b)))
    return inter / (area_a + area_b - inter)


def iou_matrix(boxes1, boxes2):
    boxes1, boxes2 = np.asarray(boxes1, dtype=np.float64).reshape(-1, 2, 4), np.asarray(boxes2, dtype=np.float64).reshape(-1, 2, 4)
    out = np.zeros((len(boxes1), len(boxes2)))
    lo1, hi1, lo2, hi2 = boxes1.min(axis=2), boxes1.max(axis=2), boxes2.min(axis=2), boxes2.max(axis=2)
    for i in range(len(boxes1)):
        for j in range(len(boxes2)):
            if (hi1[i] > lo2[j]).all() and (lo1[i] < hi2[j]).all():      # helper.py:47-51
                out[i, j] = iou(boxes1[i], boxes2[j])
    return out


def ats_from_iou(m):
    n1, n2 = m.shape
    if n1 == 0 or n2 == 0:
        return 0.0
    iou_max = m.max(axis=0)
    total = weight = 0.0
    for t in THRESHOLDS:
        tp = int((iou_max > t).sum())
        total += 1.0 / t * (tp / (n1 + n2 - tp))
        weight += 1.0 / t
    return total / weight


def ats(boxes1, boxes2):
    """compute_ats_bounding_boxes (helper.py:33-72); 0 when either set is empty."""
    return ats_from_iou(iou_matrix(boxes1, boxes2))


def threshold_margin(m):
    """Smallest distance of any entry of an IoU matrix to one of the five thresholds (inf for an empty matrix)."""
    if m.size == 0:
        return math.inf
    return float(min(np.abs(m - t).min() for t in THRESHOLDS))


# ------------------------------------------------------------------------------------------------ generators
def ring_to_box(ring, reverse=False):
    """4 ring points (outline order) -> [2,4] corner columns with outline 0,1,3,2; reverse = the other orientation."""
    r = list(ring)[::-1] if reverse else list(ring)
    return np.array([r[0], r[1], r[3], r[2]], dtype=np.float64).T


def rotated_rect(cx, cy, length, width, angle, reverse=False):
    c, s = math.cos(angle), math.sin(angle)
    ring = [(cx + c * dx - s * dy, cy + s * dx + c * dy) for dx, dy in
            ((length / 2, width / 2), (length / 2, -width / 2), (-length / 2, -width / 2), (-length / 2, width / 2))]
    return ring_to_box(ring, reverse)


def random_rects(rng, n, centre=None, spread=37.0):
    """n rotated rectangles, sides 0.5-6, coordinates within +-40, both orientations."""
    out = np.zeros((n, 2, 4))
    for i in range(n):
        cx, cy = rng.uniform(-spread, spread, 2) if centre is None else np.asarray(centre) + rng.uniform(-3, 3, 2)
        out[i] = rotated_rect(cx, cy, rng.uniform(0.5, 6), rng.uniform(0.5, 6), rng.uniform(0, 2 * math.pi), bool(rng.integers(2)))
    return out


def random_convex_quads(rng, n, centre=None, spread=36.0):
    """n general convex quadrilaterals: four points on an ellipse (always in convex position), sides kept within 0.5-6."""
    out = np.zeros((n, 2, 4))
    i = 0
    while i < n:
        cx, cy = rng.uniform(-spread, spread, 2) if centre is None else np.asarray(centre) + rng.uniform(-3, 3, 2)
        a, b, rot = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 2 * math.pi)
        th = rng.uniform(0, 2 * math.pi) + np.arange(4) * (math.pi / 2) + rng.uniform(-0.5, 0.5, 4)
        px, py = a * np.cos(th), b * np.sin(th)
        ring = [(cx + math.cos(rot) * x - math.sin(rot) * y, cy + math.sin(rot) * x + math.cos(rot) * y) for x, y in zip(px, py)]
        sides = [math.dist(ring[k], ring[(k + 1) % 4]) for k in range(4)]
        if min(sides) < 0.5 or max(sides) > 6.0:
            continue
        out[i] = ring_to_box(ring, bool(rng.integers(2)))
        i += 1
    return out


def exact_cases():
    """(box1, box2, expected IoU): the cases with known answers."""
    sq = rotated_rect(0.0, 0.0, 1.0, 1.0, 0.0)
    inter = 2.0 * (math.sqrt(2.0) - 1.0)
    far = rotated_rect(31.25, -17.5, 4.5, 2.0, 0.0)
    return [
        (sq, sq.copy(), 1.0),                                                     # identical
        (far, far.copy(), 1.0),
        (sq, rotated_rect(0.0, 0.0, 1.0, 1.0, 0.0, reverse=True), 1.0),           # identical, other orientation
        (sq, rotated_rect(1.0, 0.0, 1.0, 1.0, 0.0), 0.0),                         # share only an edge
        (sq, rotated_rect(0.0, -1.0, 1.0, 1.0, 0.0, reverse=True), 0.0),
        (sq, rotated_rect(0.5, 0.0, 1.0, 1.0, 0.0), 1.0 / 3.0),                   # shifted by half a side
        (sq, rotated_rect(0.0, 0.0, 1.0, 1.0, math.pi / 4), inter / (2.0 - inter)),   # regular octagon
        (sq, rotated_rect(5.0, 5.0, 1.0, 1.0, 0.3), 0.0),                         # disjoint
        (rotated_rect(0.0, 0.0, 4.0, 2.0, 0.0), rotated_rect(0.5, 0.25, 1.0, 0.5, 0.0), 0.5 / 8.0),   # contained
    ]


def ats_pair(rng, n_targets, n_exact, n_mid, n_off, n_stray):
    """One pair of sets for the ATS test.  Targets sit on a jittered grid, far enough apart that only intended pairs overlap;
    set 1 = exact copies (IoU 1), a few moderately perturbed copies (IoU somewhere in 0.3-0.95), badly shifted copies (IoU well
    below 0.5) and strays.  Few entries lie anywhere near a threshold, which keeps the discard rate of the 1e-3 margin small."""
    cells = rng.permutation(64)[:n_targets + n_stray]
    centres = [(-35.0 + 10.0 * (c % 8) + rng.uniform(-1, 1), -35.0 + 10.0 * (c // 8) + rng.uniform(-1, 1)) for c in cells]
    spec = [(rng.uniform(2, 6), rng.uniform(1, 3), rng.uniform(0, 2 * math.pi)) for _ in centres]
    targets = np.array([rotated_rect(x, y, l, w, a, bool(rng.integers(2))) for (x, y), (l, w, a) in zip(centres[:n_targets], spec[:n_targets])]
                       ).reshape(-1, 2, 4)
    preds = []
    order = rng.permutation(n_targets)
    for k, t in enumerate(order[:n_exact + n_mid + n_off]):
        (x, y), (l, w, a) = centres[t], spec[t]
        if k < n_exact:
            preds.append(targets[t].copy())
        elif k < n_exact + n_mid:
            preds.append(rotated_rect(x + rng.uniform(-0.4, 0.4), y + rng.uniform(-0.4, 0.4), l * rng.uniform(0.85, 1.15), w * rng.uniform(0.85, 1.15),
                                      a + rng.uniform(-0.15, 0.15), bool(rng.integers(2))))
        else:
            preds.append(rotated_rect(x + 0.8 * l * math.cos(a), y + 0.8 * l * math.sin(a), l, w, a, bool(rng.integers(2))))
    for (x, y), (l, w, a) in zip(centres[n_targets:], spec[n_targets:]):
        preds.append(rotated_rect(x, y, l, w, a))
    preds = np.array(preds).reshape(-1, 2, 4)
    return preds[rng.permutation(len(preds))], targets


def ats_batch():
    """130 (set 1, set 2, IoU matrix) samples from ats_pair for tests/test_gpu_batch_boundaries.py, under the rule of
    tests/test_gpu_box_eval.py: a pair with an IoU within 1e-3 of a threshold is discarded and drawn again.
    -> (cases, number generated)."""
    rng = np.random.default_rng(6465)
    cases, generated = [], 0
    while len(cases) < 130:
        generated += 1
        s1, s2 = ats_pair(rng, int(rng.integers(1, 14)), int(rng.integers(0, 5)), int(rng.integers(0, 3)), int(rng.integers(0, 3)),
                          int(rng.integers(0, 4)))
        m = iou_matrix(s1, s2)
        if threshold_margin(m) < 1e-3:
            continue
        cases.append((s1, s2, m))
    return cases, generated


EMPTY = np.zeros((0, 2, 4))


@functools.lru_cache(maxsize=None)
def ats_arrangements():
    """Two placements of empty sets over the same 130 samples.  "edges": an empty side at samples 0, 63, 64 and 129.  "middle": every
    sample of the second table (64-127) has an empty side, so that launch has no pair and the third must still start at the right
    place of the flat IoU buffer."""
    cases, generated = ats_batch()
    out = {}
    for name in ("edges", "middle"):
        sets1, sets2 = [c[0] for c in cases], [c[1] for c in cases]
        holes = {0: 1, 63: 2, 64: 1, 129: 2} if name == "edges" else {i: 1 + i % 2 for i in range(64, 128)}
        for i, side in holes.items():
            if side == 1:
                sets1[i] = EMPTY
            else:
                sets2[i] = EMPTY
        mats = [np.zeros((len(a), len(b))) if i in holes else cases[i][2] for i, (a, b) in enumerate(zip(sets1, sets2))]
        out[name] = (sets1, sets2, mats)
    return out, cases, generated
