"""tests/_rankb_ref.py without a GPU: the class of every case (which kernel form, how many tiles, workgroups and tiles per workgroup,
whether a piece changes its dY tile and whether a workgroup comes up empty), the margin that fp32 references leave inside the derived
bounds, and that the checker rejects the wrong results it is there to catch."""
import pytest
import torch

import _rankb_ref as ref

IDS = [f"rows{c[0]}-{c[1]}x{c[2]}-blocks{c[3]}-spare{c[4]}" for c, _ in ref.CASES]


def test_the_table_holds_what_the_issue_lists():
    assert len(ref.CASES) == len(set(c for c, _ in ref.CASES)) == 16
    assert {cls[0] for _, cls in ref.CASES} == {"short", "lds<1,2>", "lds<2,1>", "wide"}
    assert all(c[0] <= 64 and c[1] % 4 == 0 and c[2] % 4 == 0 for c, _ in ref.CASES)
    assert max(c[1] * c[2] * 4 for c, _ in ref.CASES) < 9 << 20      # the largest tensor: 9 MB


@pytest.mark.parametrize("case,cls", ref.CASES, ids=IDS)
def test_every_case_is_of_the_class_it_is_listed_under(case, cls):
    assert ref.plan(*case) == cls


def test_plan_on_shapes_whose_launch_is_known():
    """The launches tests/test_gpu_round5.py describes in words."""
    assert ref.plan(32, 16 * 70, 64 * 20) == ("lds<1,2>", 360, 256, 2, False, True)      # 18 n-groups x 20 k-tiles: more group-tiles than workgroups
    assert ref.plan(32, 640000, 64)[:4] == ("short", 10000, 256, 40)                     # the head: 10 000 n-groups, 40 per workgroup
    assert ref.plan(64, 640000, 64)[0] == ref.plan(48, 640000, 64)[0] == "lds<2,1>"
    assert ref.plan(16, 136, 64 * 70 + 12, 4)[0] == "wide" and ref.plan(16, 136, 64 * 70 + 12, 1)[0] == "lds<1,2>"
    assert ref.plan(32, 1024, 2052, 1, 128)[1:5] == (16 * 33, 128, 5, True)           # the spare-CU test: pieces that straddle


@pytest.fixture(scope="module")
def drawn():
    """One draw per (case, signed): the factors and the fp32 candidate of the first step."""
    out = {}
    for case, _ in ref.CASES:
        rows, n, k = case[:3]
        for signed in (True, False):
            gen = torch.Generator().manual_seed(n * 7 + k + rows)
            x, dy = ref.factors(rows, n, k, signed, 1, gen)
            out[case, signed] = (x, dy)
    return out


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("case", [c for c, _ in ref.CASES], ids=IDS)
def test_fp32_references_stay_inside_the_bounds(drawn, case, signed):
    """``dy.T @ x`` in fp32 and a row-by-row sequential sum, through the element's three multiplies: the derived bounds hold for any
    order of summation, so both must pass, with room (they used at most 0.36 of the gradient's bound over rows 1 .. 64)."""
    x, dy = drawn[case, signed]
    for sequential in (False, True):
        frac = ref.check_first_step(dy, x, *ref.model_first_step(dy, x, sequential))
        print(case, signed, "sequential" if sequential else "matmul", {k: round(f, 3) for k, f in frac.items()})
        assert set(frac) == {"m", "v", "bias_m", "bias_v"}
        assert max(frac["m"], frac["bias_m"]) <= 0.5      # the sums by themselves leave half of their bound (v: two roundings of its four units are m's)


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("case", [(9, 19220, 64, 1, 128), (40, 260, 2052, 1, 128), (20, 52, 132, 1, 0)], ids=["short", "two-chunks", "ragged"])
def test_the_checker_rejects_wrong_results(drawn, case, signed):
    x, dy = drawn[case, signed]
    rows, n, k = case[:3]
    good = ref.model_first_step(dy, x)
    ref.check_first_step(dy, x, *good)

    def rejected(m, v, bm, bv, where):
        frac = ref.first_step_fractions(dy, x, m, v, bm, bv)
        with pytest.raises(AssertionError):
            ref.check_first_step(dy, x, m, v, bm, bv)
        assert not frac[where] <= 1.0, (where, frac)
        return frac

    # the last batch row dropped (a contraction that stops one row early)
    m, v, bm, bv = ref.model_first_step(dy[:-1], x[:-1])
    frac = rejected(m, v, bm, bv, "m")
    assert not frac["bias_m"] <= 1.0
    # one 16 x 64 tile zeroed (a tile nobody owned)
    m, v = good[0].clone(), good[1].clone()
    m[16:32, :64] = 0
    v[16:32, :64] = 0
    rejected(m, v, good[2], good[3], "m")
    # one tile's v scaled by 1 + 2^-18 (3.8e-6 of the element: under 2e-6 of the tensor's peak wherever the element is below half of it)
    v = good[1].clone()
    v[:16, -4:] *= 1 + 2.0 ** -18
    frac = rejected(good[0], v, good[2], good[3], "v")
    assert frac["m"] <= 1.0
    # rows >= M taken from whatever lies behind x (0xFF bytes: NaN) and multiplied by dY's zeros
    pad = 32 * ((rows + 31) // 32) - rows
    xp = torch.cat([x, torch.full((pad, k), float("nan"))])
    yp = torch.cat([dy, torch.zeros(pad, n)])
    rejected(*ref.model_first_step(yp, xp)[:2], good[2], good[3], "m")
    # ... and from a finite neighbour: the same numbers, nothing to reject (why the guard arena is filled with NaN)
    xp = torch.cat([x, torch.ones(pad, k)])
    ref.check_first_step(dy, x, *ref.model_first_step(yp, xp)[:2], good[2], good[3])
    # bias_v left at zero
    rejected(good[0], good[1], good[2], torch.zeros(n), "bias_v")
