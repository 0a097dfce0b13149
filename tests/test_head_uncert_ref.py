"""The reference of the sampled head's uncertainty (tests/_head_uncert_ref.py) against itself, without a GPU, on the GPU test's own
inputs (tests/_head_uncert_cases.py): the fp32 model of the header's formulas -- correctly rounded primitives -- stays inside the TIGHT
bounds of the fp64 reference, so the bounds are met by the formulas alone; the properties the statistics have in real arithmetic hold
in the model; and the pure-fp64 reference from the operands agrees with the one from the logits within the LOOSE bounds."""
import numpy as np
import pytest

import _head_uncert_cases as cases
import _head_uncert_ref as ref

LN2 = np.float32(np.log(2.0))
MAPS = ("mean", "entropy", "expected", "mi", "var", "scores")


def logits(scenes, samples, n, k, bias, spread):
    x, w, b = cases.operands("cpu", scenes, samples, n, k, bias, spread)
    return cases.logits32_cpu(x, w, b), cases.numpy_operands(x, w, b)


@pytest.mark.parametrize("scenes,samples", cases.GROUPS, ids=[f"{b}x{s}" for b, s in cases.GROUPS])
def test_the_fp32_model_stays_inside_the_tight_bounds(scenes, samples):
    worst = dict.fromkeys(MAPS, 0.0)
    reach = {s: 0.0 for s in cases.SPREADS}
    for n, k, bias, spread in cases.shapes():
        z32, (x, w, b) = logits(scenes, samples, n, k, bias, spread)
        reach[spread] = max(reach[spread], float(np.abs(z32).max()))
        want, bound = ref.stats_from_logits(z32, samples)
        got = ref.model32(z32, samples)
        for name in MAPS:
            used = ref.fraction(getattr(got, name), getattr(want, name), getattr(bound, name))
            worst[name] = max(worst[name], used)
            assert used <= 1.0, (scenes, samples, n, k, bias, spread, name, used)
        # what holds in real arithmetic holds in the model
        assert np.all(got.mi >= 0) and np.all(got.mi <= got.entropy) and np.all(got.entropy <= LN2 * (1 + 2.0 ** -22))
        assert np.all(got.mean >= 0) and np.all(got.mean <= 1), "1 - m never goes negative"
        m = got.mean.astype(np.float64)
        assert np.all(got.var <= m * (1 - m) + bound.var)
        if samples == 1:
            assert np.all(got.mi == 0) and np.all(got.var == 0) and np.array_equal(got.scores[:, 1:], np.zeros((scenes, 2)))
        # ... and the two references agree within the loose bound, which is the wider one
        want64, loose = ref.stats64(x, w, b, samples)
        for name in MAPS:
            assert ref.fraction(getattr(want, name), getattr(want64, name), getattr(loose, name)) <= 1.0, (n, k, bias, spread, name)
    print(f"({scenes},{samples}): the fp32 model uses of the tight bounds: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; |z| reaches {reach[cases.NARROW]:.1f} / {reach[cases.WIDE]:.1f}")
    assert reach[cases.WIDE] >= 30.0, "the wide spread carries both tails"


def test_the_tight_bounds_are_a_few_1e_6_and_the_loose_ones_wider():
    for scenes, samples in cases.GROUPS:
        z32, (x, w, b) = logits(scenes, samples, 272, 68, True, cases.NARROW)
        _, tight = ref.stats_from_logits(z32, samples)
        _, loose = ref.stats64(x, w, b, samples)
        for name in MAPS:
            t, l = getattr(tight, name), getattr(loose, name)
            assert 0 < t.min() and t.max() < (samples + 40) * 2 * ref.U < 2e-5, (samples, name, t.max())
            assert np.all(l >= t) and l.max() < 2e-3, (samples, name)


@pytest.mark.parametrize("samples", [1, 2, 5, 16, 64])
def test_identical_draws_have_no_spread(samples):
    """Every draw of a scene the same logit: the mutual information is within its bound of 0; the variance is EXACTLY 0 where the mean is
    the draw itself -- S = 1 and S = 2, whose sum p + p and halving are exact -- and within its bound of 0 otherwise: from the third add
    on p + p + p is rounded, so the pinned draw-order mean of identical fp32 values need not be that value."""
    z32, _ = logits(3, samples, 130, 68, True, cases.WIDE)
    same = cases.identical_draws(z32, samples)
    want, bound = ref.stats_from_logits(same, samples)
    got = ref.model32(same, samples)
    assert np.all(want.mi <= 1e-12) and np.all(want.var <= 1e-28)      # the fp64 reference's own rounding
    assert np.all(got.mi <= bound.mi) and np.all(got.var <= bound.var)
    if samples <= 2:
        assert np.all(got.var == 0)


def test_the_draw_entropy_from_the_logit_is_the_binary_entropy_of_the_probability():
    z = np.concatenate([np.linspace(-30, 30, 2001), [0.0, -0.0, 200.0, -200.0, 87.4, -103.0]])
    h = ref.draw_entropy64(z)
    assert np.all(np.isfinite(h)) and h[2001] == np.log(2.0) and 0 < h[2003] < 1e-80 and h[2004] == h[2003]
    mid = np.abs(z) <= 20      # beyond, 1 - p cancels in the probability form: the reason the header takes it from the logit
    assert np.max(np.abs(h[mid] - ref.entropy64(ref.er.sigmoid64(z[mid])))) < 1e-14
    z32 = np.array([[0.0, -0.0, 200.0, -200.0, 87.4, -103.0, 16.7, -17.4]], dtype=np.float32)
    got = ref.model32(z32, 1)
    assert np.all(np.isfinite(got.entropy)) and got.entropy[0, 0] == LN2 and np.all(got.entropy[0, 2:4] == 0)


def test_a_nan_logit_poisons_its_pixel_and_its_scene_only():
    z32, _ = logits(3, 4, 16, 4, True, cases.NARROW)
    z32[1 * 4 + 2, 5] = np.nan
    got = ref.model32(z32, 4)
    for name in ("mean", "entropy", "mi", "var"):
        bad = np.isnan(getattr(got, name))
        assert bad[1, 5] and bad.sum() == 1, name
    assert np.all(np.isnan(got.scores[1])) and np.all(np.isfinite(got.scores[[0, 2]]))


def test_the_mean_never_exceeds_one():
    """(S * 1.0f) * (float)(1 / S) <= 1 for every S the kernel takes: 1 - m is never negative, and logf never sees a negative number."""
    for s in range(1, 65):
        assert np.float32(np.float32(s) * np.float32(1.0 / s)) <= np.float32(1.0), s


def test_the_ranking_case_cannot_pass_by_rounding():
    """tests/_head_uncert_cases.ranking_inputs, with the fp64 oracle alone: the scene whose draws share one mask has no mutual
    information, the scene with independent masks has, and the gap between the two scores exceeds TWICE the bound a model is held to --
    so tests/test_gpu_head_uncert_models.py's ranking cannot come out right by rounding."""
    import _head_mean_cases as hc
    from driving_dirty_amd.roadmap import RoadMapBCE
    x, masks = cases.ranking_inputs()
    want, bound = cases.model_reference(hc.build(RoadMapBCE), x, cases.RANK_DRAWS, masks)
    same, free, tol = want.scores[0, 1], want.scores[1, 1], bound.scores[:, 1].max()
    print(f"mutual-information score: shared mask {same:.3g}, independent masks {free:.3g}, bound {tol:.3g}")
    assert same <= 1e-12 and free - same > 2 * tol
    assert want.scores[0, 2] <= 1e-28 and want.scores[1, 2] > 2 * bound.scores[:, 2].max(), "the variance score tells them apart too"
