"""CPU reference for marker-based splitting (csrc/boxeval.hip: dd_split_components, dd_labelled_boxes, dd_labelled_obb): the rule of
include/dd_hotpath.h restated in numpy.  Labelling, the fit of one pixel list, IoU and ATS come from _box_eval_ref / _box_fit_ref;
nothing here imports the package under test.

For one mask, r = split_px >= 1, g = grow_iters >= 0:
  1. erode: core[p] = every pixel of the (2r+1) x (2r+1) square round p is in the mask (outside the image = background);
  2. label the cores: canonical labels, 1 + raster index of the component's first pixel (4-connected);
  3. grow: g synchronous rounds; a mask pixel with label 0 and a labelled pixel among its 8 neighbours takes the smallest such label;
  4. leftovers: mask pixels still 0 are labelled as 4-connected components of the leftover set, canonically.

``split`` is that on the whole image.  ``split_tiled`` computes steps 1 and 3 one 32 x 32 tile at a time from the tile plus a halo of
r / g pixels -- what the kernels do -- and a CPU test holds the two together.  ``region_boxes`` / ``fit_regions`` are the extent and the
oriented fit of _box_eval_ref / _box_fit_ref for regions given as a label image.
"""
import math

import numpy as np

import _box_eval_ref as ref

MAX_SPLIT_PX, MAX_GROW_ITERS = 8, 16
TILE = 32
_BIG = np.iinfo(np.int64).max


# ------------------------------------------------------------------------------------------------ the rule
def erode(mask, r):
    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    pad = np.pad(mask, r, constant_values=False)
    core = np.ones_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            core &= pad[dy:dy + h, dx:dx + w]
    return core


def grow_round(lab, mask):
    """One synchronous round: reads `lab` only, returns the next image."""
    h, w = lab.shape
    p = np.pad(np.where(lab > 0, lab, _BIG), 1, constant_values=_BIG)
    m = np.full(lab.shape, _BIG, dtype=np.int64)
    for dy in range(3):
        for dx in range(3):
            if dy != 1 or dx != 1:
                m = np.minimum(m, p[dy:dy + h, dx:dx + w])
    return np.where((lab == 0) & mask & (m < _BIG), m, lab)


def grow(lab, mask, g):
    lab = np.asarray(lab, dtype=np.int64)
    for _ in range(g):
        lab = grow_round(lab, mask)
    return lab


def with_leftovers(lab, mask):
    left = mask & (lab == 0)
    return np.where(left, ref.label(left), lab).astype(np.int32)


def split(mask, split_px, grow_iters):
    """bool [H,W] -> int32 [H,W] label image of the rule above."""
    assert 1 <= split_px <= MAX_SPLIT_PX and 0 <= grow_iters <= MAX_GROW_ITERS
    mask = np.asarray(mask, dtype=bool)
    return with_leftovers(grow(ref.label(erode(mask, split_px)), mask, grow_iters), mask)


def _window(a, y0, x0, halo, fill):
    """a[y0 - halo : y0 + TILE + halo, x0 - halo : x0 + TILE + halo] with `fill` outside the image."""
    h, w = a.shape
    out = np.full((TILE + 2 * halo, TILE + 2 * halo), fill, dtype=a.dtype)
    ya, yb, xa, xb = max(y0 - halo, 0), min(y0 + TILE + halo, h), max(x0 - halo, 0), min(x0 + TILE + halo, w)
    out[ya - (y0 - halo):yb - (y0 - halo), xa - (x0 - halo):xb - (x0 - halo)] = a[ya:yb, xa:xb]
    return out


def split_tiled(mask, split_px, grow_iters):
    """The same labels, with the erosion and the growth done tile by tile from the tile and its halo alone."""
    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    r, g = split_px, grow_iters
    core = np.zeros_like(mask)
    for y0 in range(0, h, TILE):
        for x0 in range(0, w, TILE):
            win = _window(mask, y0, x0, r, False)
            t = np.ones((TILE, TILE), dtype=bool)
            for dy in range(2 * r + 1):
                for dx in range(2 * r + 1):
                    t &= win[dy:dy + TILE, dx:dx + TILE]
            core[y0:y0 + TILE, x0:x0 + TILE] = t[:h - y0, :w - x0]
    seeds = ref.label(core).astype(np.int64)
    lab = np.zeros((h, w), dtype=np.int64)
    for y0 in range(0, h, TILE):
        for x0 in range(0, w, TILE):
            wl, wm = _window(seeds, y0, x0, g, 0), _window(mask, y0, x0, g, False)
            for _ in range(g):                                                      # every round over the whole window; the edge goes stale
                wl = grow_round(wl, wm)
            lab[y0:y0 + TILE, x0:x0 + TILE] = wl[g:g + TILE, g:g + TILE][:h - y0, :w - x0]
    return with_leftovers(lab, mask)


# ------------------------------------------------------------------------------------------------ fits of a label image
def _regions(lab):
    """(labels, start, size, x, y): the pixels of a label image sorted by label (stable: raster order inside a region)."""
    lab = np.asarray(lab)
    w = lab.shape[1]
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    idx = idx[np.argsort(flat[idx], kind="stable")]
    labels, start, size = np.unique(flat[idx], return_index=True, return_counts=True)
    return labels, start, size, (idx % w).astype(np.int64), (idx // w).astype(np.int64)


def region_boxes(lab, min_pixels=1):
    """Extent boxes fp32 [n,2,4] of the regions with at least min_pixels pixels, ordered by label (_box_eval_ref.component_boxes)."""
    h, w = np.asarray(lab).shape
    labels, start, size, x, y = _regions(lab)
    if len(labels) == 0:
        return np.zeros((0, 2, 4), dtype=np.float32)
    c0, c1 = np.minimum.reduceat(x, start), np.maximum.reduceat(x, start)
    r0, r1 = np.minimum.reduceat(y, start), np.maximum.reduceat(y, start)
    out = [ref.extent_to_box(int(c0[k]), int(c1[k]), int(r0[k]), int(r1[k]), h, w) for k in range(len(labels)) if size[k] >= min_pixels]
    return np.stack(out) if out else np.zeros((0, 2, 4), dtype=np.float32)


def fit_regions(lab, min_pixels=1, pad_px=0.5):
    """Oriented boxes of a label image: (boxes fp32 [n,2,4], moments int64 [n,6]) ordered by label -- the arithmetic of
    _box_fit_ref.fit_components, expression for expression, on regions instead of components."""
    lab = np.asarray(lab)
    h, w = lab.shape
    assert h <= 1024 and w <= 1024
    pad_px = float(np.float32(pad_px))
    labels, start, size, x, y = _regions(lab)
    if len(labels) == 0:
        return np.zeros((0, 2, 4), dtype=np.float32), np.zeros((0, 6), dtype=np.int64)
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
    return boxes.astype(np.float32)[keep], np.stack(sums, axis=1)[keep]


# ------------------------------------------------------------------------------------------------ hand-made masks
def two_squares(neck, gap=3, size=9):
    """Two size x size squares side by side, `gap` columns apart, joined by a bar `neck` rows high through their middle, with a
    background frame of one pixel: bool [size + 2, 2 * size + gap + 2] (size 9, gap 3: [11, 23])."""
    m = np.zeros((size + 2, 2 * size + gap + 2), dtype=bool)
    m[1:size + 1, 1:size + 1] = True
    m[1:size + 1, size + 1 + gap:2 * size + 1 + gap] = True
    lo = 1 + size // 2 - neck // 2
    m[lo:lo + neck, size + 1:size + 1 + gap] = True
    return m


def place(small, shape, y0, x0):
    out = np.zeros(shape, dtype=bool)
    out[y0:y0 + small.shape[0], x0:x0 + small.shape[1]] = small
    return out


# ------------------------------------------------------------------------------------------------ the value scenes
CONTACT_SCENE_SEEDS = (21, 22, 23, 24, 25, 26)


def contact_pairs(seed, n_pairs=20):
    """2 * n_pairs car-sized rectangles (3.5-6 m x 1.6-2.4 m) as [n,2,4] fp64: pairs IN CONTACT on a jittered 13 m grid, each pair
    either side by side (gap 0-0.15 m, the second car shifted lengthwise by up to +-1.5 m) or nose to tail (gap 0-0.15 m).  At 10
    pixels per metre and with an inclusive rasteriser every pair is one blob."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(36)[:n_pairs]
    cars = []
    for cell in cells:
        x, y = -32.0 + 13.0 * (cell % 6) + rng.uniform(-1, 1), -32.0 + 13.0 * (cell // 6) + rng.uniform(-1, 1)
        a, length, width = rng.uniform(0, 2 * math.pi), rng.uniform(3.5, 6.0), rng.uniform(1.6, 2.4)
        kind = rng.integers(2)
        cars.append(ref.rotated_rect(x, y, length, width, a))
        if kind == 0:
            gap, shift, width2 = rng.uniform(0.0, 0.15), rng.uniform(-1.5, 1.5), rng.uniform(1.6, 2.4)
            d = (width + width2) / 2 + gap
            cars.append(ref.rotated_rect(x - math.sin(a) * d + math.cos(a) * shift, y + math.cos(a) * d + math.sin(a) * shift,
                                         rng.uniform(3.5, 6.0), width2, a))
        else:
            gap, length2 = rng.uniform(0.0, 0.15), rng.uniform(3.5, 6.0)
            d = (length + length2) / 2 + gap
            cars.append(ref.rotated_rect(x + math.cos(a) * d, y + math.sin(a) * d, length2, rng.uniform(1.6, 2.4), a))
    return np.stack(cars)


def contact_scene_mask(seed):
    """(cars [40,2,4], bool [800,800]): a contact-pair scene and its rasterised map (the repository's own CPU rasteriser)."""
    from oracle import raster
    cars = contact_pairs(seed)
    return cars, np.asarray(raster.boxes_to_binary_map(cars)) > 0.5
