"""numpy restatement of the threshold calibration: the binning of ``dd_ts_hist``, the curve and the argmax of ``ops.ts_curve``, and
the reference's own threat score.  Written from the definitions, shares no code with the package."""
import numpy as np


def ts_hist_ref(prob, target, bins):
    """int64 [2, bins + 1]: slot ceil(p * bins) clamped to [0, bins] (NaN -> 0), row 1 where the target is non-zero."""
    p = np.asarray(prob, dtype=np.float32).reshape(-1)
    t = np.asarray(target).reshape(-1) != 0
    with np.errstate(invalid="ignore"):
        c = np.ceil(p * np.float32(bins))          # a power of two: exact
        slot = np.where(c >= bins, bins, np.where(c > 0, c, 0))      # comparisons with NaN are false -> 0
    slot = slot.astype(np.int64)
    hist = np.zeros((2, bins + 1), dtype=np.int64)
    np.add.at(hist, (t.astype(np.int64), slot), 1)
    return hist


def ts_curve_ref(hist):
    """(ts float64 [bins], best_k).  ts[k] scores the prediction p > k / bins, i.e. the elements in slots above k."""
    hist = np.asarray(hist, dtype=np.int64)
    bins = hist.shape[1] - 1
    total_pos = int(hist[1].sum())
    ts = np.zeros(bins, dtype=np.float64)
    for k in range(bins):
        tp = int(hist[1, k + 1:].sum())
        pred = int(hist[:, k + 1:].sum())
        den = pred + total_pos - tp
        ts[k] = tp / den if den else 0.0
    best, top = None, ts.max()
    for k in range(bins):      # ties: nearest bins / 2, then the lower k
        if ts[k] == top and (best is None or abs(k - bins // 2) < abs(best - bins // 2)):
            best = k
    return ts, best


def reference_ts(target, pred):
    """compute_ts_road_map of the reference (helper.py): tp / (sum(a) + sum(b) - tp) with tp = sum(a * b), on 0/1 maps."""
    a = np.asarray(target, dtype=np.float64).reshape(-1)
    b = np.asarray(pred, dtype=np.float64).reshape(-1)
    tp = (a * b).sum()
    return tp / (a.sum() + b.sum() - tp)
