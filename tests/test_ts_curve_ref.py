"""CPU checks of the threshold calibration's reference (tests/_ts_curve_ref.py) and of ``ops.ts_curve`` against it, and of the
inputs the GPU test of dd_linear_sigmoid_gt relies on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _predict_cases as pc  # noqa: E402
from _ts_curve_ref import reference_ts, ts_curve_ref, ts_hist_ref  # noqa: E402


@pytest.mark.parametrize("bins", [2, 256, 1024])
def test_curve_at_half_is_the_reference_threat_score_of_the_rounded_map(bins):
    from driving_dirty_amd import ops
    rs = np.random.RandomState(bins)
    prob = rs.random_sample(20000).astype(np.float32)
    prob[:4] = (0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.0, 1.0)
    target = rs.random_sample(20000) < 0.3
    hist = ts_hist_ref(prob, target, bins)
    assert hist.sum() == prob.size
    want = reference_ts(target, np.round(prob))
    ts, _ = ts_curve_ref(hist)
    assert abs(ts[bins // 2] - want) < 1e-12
    got, best = ops.ts_curve(torch.from_numpy(hist))
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), ts) and best == ts_curve_ref(hist)[1]
    # every threshold, from the definition
    for k in (0, 1, bins // 2, bins - 1):
        assert abs(ts[k] - reference_ts(target, prob > np.float32(k / bins))) < 1e-12


def _hist(bins, entries):
    h = np.zeros((2, bins + 1), dtype=np.int64)
    for row, slot, count in entries:
        h[row, slot] = count
    return h


@pytest.mark.parametrize("name,bins,entries,best", [
    ("all empty: every threshold scores 0, the tie goes to bins / 2", 8, [], 4),
    ("positives only in one bin: thresholds 0..2 score 1, 2 is nearest to 4", 8, [(1, 3, 5)], 2),
    ("one bin above the middle: 0..5 tie, 4 itself is among them", 8, [(1, 6, 7)], 4),
    # T = 4.  k = 1..3: tp 4 of 8 predicted -> 4/8; k = 4 drops two hits: 2/(6 + 4 - 2); k >= 5 drops four false alarms: 2/(2 + 4 - 2)
    ("equal maxima 0.5 at 3 and 5 with 0.25 between them, either side of the middle: the lower k", 8, [(1, 8, 2), (1, 4, 2), (0, 5, 4), (0, 1, 3)], 3),
    ("negatives only: 0 everywhere", 4, [(0, 1, 9), (0, 4, 2)], 2),
])
def test_argmax_and_its_tie_rule(name, bins, entries, best):
    from driving_dirty_amd import ops
    h = _hist(bins, entries)
    ts, ref_best = ts_curve_ref(h)
    got, got_best = ops.ts_curve(torch.from_numpy(h))
    assert np.array_equal(got.numpy(), ts), name
    assert got_best == ref_best, name
    if best is not None:
        assert ref_best == best, name


@pytest.mark.parametrize("m,n,k", pc.CASES)
def test_head_test_inputs_keep_clear_of_the_threshold(m, n, k):
    """The GPU test of dd_linear_sigmoid_gt compares with fp64 outside a band around the threshold's logit and lets the band cover at
    most 1e-3 of the elements.  That the inputs satisfy this is a property of the inputs alone: shown here, from fp64 logits, for
    the very seeds, shapes and thresholds the GPU test uses."""
    x, w, b = pc.head_inputs(m, n, k)
    plain = x.astype(np.float64) @ w.astype(np.float64).T
    for logit in (plain, plain + b.astype(np.float64)):
        for tau in pc.TAUS:
            share = pc.band_mask(logit, tau).mean()
            assert share <= pc.BAND_CAP, (m, n, k, tau, share)
