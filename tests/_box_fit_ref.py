"""CPU reference for the oriented box fit (csrc/boxeval.hip, dd_component_obb): the fit of include/dd_hotpath.h restated in numpy /
plain Python fp64.  Labelling, IoU and ATS come from _box_eval_ref; nothing here imports the package under test.

For one 4-connected component (pixel = column X, row Y):
  1. N, Sx, Sy, Sxx, Sxy, Syy = sums of 1, X, Y, X*X, X*Y, Y*Y (exact integers);
  2. mxx = N*Sxx - Sx*Sx, myy = N*Syy - Sy*Sy, mxy = N*Sxy - Sx*Sy, theta = 0.5 * atan2(2.0*mxy, float(mxx - myy));
  3. c, s = cos / sin(theta); u = (X+0.5)*c + (Y+0.5)*s, v = -(X+0.5)*s + (Y+0.5)*c; min / max, moved outwards by pad_px*(|c|+|s|);
  4. ring (u1,v1), (u1,v0), (u0,v0), (u0,v1) -> X = u*c - v*s, Y = u*s + v*c -> x = (X - W/2)/10, y = (H/2 - Y)/10 -> one rounding to
     fp32, ring stored in columns 0, 1, 3, 2.

``fit_pixels`` is that, one component at a time, in plain Python (the pinned cases use it); ``fit_components`` is the same arithmetic
vectorised over a whole map (the GPU tests' 800 x 800 random masks have 10^5 components), and a CPU test holds the two together.
"""
import math

import numpy as np

import _box_eval_ref as ref


def moments_of(cols, rows):
    """Exact integer (N, Sx, Sy, Sxx, Sxy, Syy) of a pixel list, by brute force in Python integers."""
    cols, rows = [int(c) for c in cols], [int(r) for r in rows]
    return (len(cols), sum(cols), sum(rows), sum(c * c for c in cols), sum(c * r for c, r in zip(cols, rows)), sum(r * r for r in rows))


def heading(m):
    n, sx, sy, sxx, sxy, syy = (int(v) for v in m)
    mxx, myy, mxy = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy
    assert max(abs(mxx), abs(myy), abs(mxy)) < 2 ** 62                             # what the kernel's int64 holds
    return 0.5 * math.atan2(2.0 * float(mxy), float(mxx - myy))


def ring_to_box32(ring_x, ring_y, h, w):
    """Ring in pixel coordinates (fp64) -> fp32 [2,4], ring in columns 0, 1, 3, 2."""
    box = np.zeros((2, 4), dtype=np.float64)
    for k, col in enumerate((0, 1, 3, 2)):
        box[0, col] = (ring_x[k] - w / 2) / 10.0
        box[1, col] = (h / 2 - ring_y[k]) / 10.0
    return box.astype(np.float32)


def fit_pixels(cols, rows, h, w, pad_px=0.5):
    """(box fp32 [2,4], theta, moments) of one component given as pixel lists."""
    pad_px = float(np.float32(pad_px))                                             # the entry point takes pad_px as fp32
    m = moments_of(cols, rows)
    theta = heading(m)
    c, s = math.cos(theta), math.sin(theta)
    us = [(x + 0.5) * c + (y + 0.5) * s for x, y in zip(cols, rows)]
    vs = [-(x + 0.5) * s + (y + 0.5) * c for x, y in zip(cols, rows)]
    pad = pad_px * (abs(c) + abs(s))
    u0, u1, v0, v1 = min(us) - pad, max(us) + pad, min(vs) - pad, max(vs) + pad
    ring = ((u1, v1), (u1, v0), (u0, v0), (u0, v1))
    return ring_to_box32([u * c - v * s for u, v in ring], [u * s + v * c for u, v in ring], h, w), theta, m


def fit_components(mask, min_pixels=1, pad_px=0.5):
    """bool [H,W] -> (boxes fp32 [n,2,4], moments int64 [n,6], theta fp64 [n]) of the components with at least min_pixels pixels,
    ordered by canonical label.  The arithmetic of fit_pixels, vectorised: int64 sums by reduceat over the pixels sorted by label."""
    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    assert h <= 1024 and w <= 1024                                                  # N * Sxx < 2^60
    pad_px = float(np.float32(pad_px))
    lab = ref.label(mask).ravel()
    idx = np.flatnonzero(lab)
    if idx.size == 0:
        return np.zeros((0, 2, 4), dtype=np.float32), np.zeros((0, 6), dtype=np.int64), np.zeros(0)
    order = np.argsort(lab[idx], kind="stable")
    idx = idx[order]
    labels, start, size = np.unique(lab[idx], return_index=True, return_counts=True)
    x, y = (idx % w).astype(np.int64), (idx // w).astype(np.int64)
    sums = [np.add.reduceat(t, start) for t in (np.ones_like(x), x, y, x * x, x * y, y * y)]
    n, sx, sy, sxx, sxy, syy = sums
    mxx, myy, mxy = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy
    theta = 0.5 * np.arctan2(2.0 * mxy.astype(np.float64), (mxx - myy).astype(np.float64))
    c, s = np.cos(theta), np.sin(theta)
    which = np.repeat(np.arange(len(labels)), size)
    cp, sp = c[which], s[which]
    xc, yc = x + 0.5, y + 0.5
    u, v = xc * cp + yc * sp, -xc * sp + yc * cp
    pad = pad_px * (np.abs(c) + np.abs(s))
    u0, u1 = np.minimum.reduceat(u, start) - pad, np.maximum.reduceat(u, start) + pad
    v0, v1 = np.minimum.reduceat(v, start) - pad, np.maximum.reduceat(v, start) + pad
    ring_u, ring_v = (u1, u1, u0, u0), (v1, v0, v0, v1)
    boxes = np.zeros((len(labels), 2, 4), dtype=np.float64)
    for k, col in enumerate((0, 1, 3, 2)):
        boxes[:, 0, col] = (ring_u[k] * c - ring_v[k] * s - w / 2) / 10.0
        boxes[:, 1, col] = (h / 2 - (ring_u[k] * s + ring_v[k] * c)) / 10.0
    keep = size >= min_pixels
    return boxes.astype(np.float32)[keep], np.stack(sums, axis=1)[keep], theta[keep]


def ulp_distance(got, want):
    """Worst |got - want| in units of one fp32 ulp of the larger magnitude (np.spacing), over two fp32 arrays of one shape."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.size == 0:
        return 0.0
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp).max())


def corner_set(box):
    """The four corners of a [2,4] box as a sorted list, for comparisons that do not care where the ring starts."""
    return sorted((float(box[0, k]), float(box[1, k])) for k in range(4))


# ------------------------------------------------------------------------------------------------ generators
def separated_cars(rng, n):
    """n car-sized rectangles (3.5-6 m x 1.6-2.4 m), uniformly random heading, either orientation, on a jittered 10 m grid: centres at
    least 8 m apart, half-diagonal at most 3.3 m, so no two touch and everything stays inside +-40 m."""
    assert n <= 64
    cells = rng.permutation(64)[:n]
    out = np.zeros((n, 2, 4))
    for i, cell in enumerate(cells):
        x, y = -35.0 + 10.0 * (cell % 8) + rng.uniform(-1, 1), -35.0 + 10.0 * (cell // 8) + rng.uniform(-1, 1)
        out[i] = ref.rotated_rect(x, y, rng.uniform(3.5, 6.0), rng.uniform(1.6, 2.4), rng.uniform(0, 2 * math.pi), bool(rng.integers(2)))
    return out


CAR_SCENE_SEEDS = (11, 12, 13, 14, 15, 16, 17, 18)      # the scenes of the value test and of the device round trip; 40 cars each


def car_scene(seed, n=40):
    return separated_cars(np.random.default_rng(seed), n)
