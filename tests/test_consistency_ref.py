"""The mirror consistency loss without a GPU: the fp64 reference of tests/_consistency_ref.py against a case worked by hand, and the
ramp of the loss's weight."""
import math

import pytest
import torch

import _consistency_ref as ref


def test_the_reference_on_a_hand_computed_case():
    """(1,2,2).  sigmoid(ln 3) = 3/4, sigmoid(-ln 3) = 1/4, sigmoid(0) = 1/2.
    a = [[0, ln3], [-ln3, 0]], m = [[ln3, 0], [0, 0]], so m' = [[0, 0], [ln3, 0]];
    P(a) = [[1/2, 3/4], [1/4, 1/2]], P(m') = [[1/2, 1/2], [3/4, 1/2]], d = [[0, 1/4], [-1/2, 0]];
    Q = 1/16 + 1/4 = 5/16, L = 5/64; a > 0 at (0,1) only, m' > 0 at (1,0) only: D = 2;
    dL/da = 2 d p (1 - p) / 4: (0,1) -> 2 (1/4)(3/16) / 4 = 3/128, (1,0) -> 2 (-1/2)(3/16) / 4 = -3/64;
    dL/dm at the reversed row, -2 d p' (1 - p') / 4: a's (0,1) is m's (1,1) -> -2 (1/4)(1/4) / 4 = -1/32, a's (1,0) is m's (0,0) ->
    -2 (-1/2)(3/16) / 4 = 3/64."""
    ln3 = math.log(3.0)
    a = torch.tensor([[[0.0, ln3], [-ln3, 0.0]]])
    m = torch.tensor([[[ln3, 0.0], [0.0, 0.0]]])
    loss, stats, da, dm = ref.loss_and_grad(a, m)
    tol = 1e-7      # ln 3 rounded to fp32
    assert abs(float(loss) - 5 / 64) < tol
    assert abs(float(stats[0, 0]) - 5 / 16) < tol and float(stats[0, 1]) == 2.0
    assert torch.allclose(da, torch.tensor([[[0.0, 3 / 128], [-3 / 64, 0.0]]], dtype=torch.float64), rtol=0, atol=tol)
    assert torch.allclose(dm, torch.tensor([[[3 / 64, 0.0], [0.0, -1 / 32]]], dtype=torch.float64), rtol=0, atol=tol)
    _, _, da4, dm4 = ref.loss_and_grad(a, m, grad_scale=0.25)
    assert torch.equal(da4, da * 0.25) and torch.equal(dm4, dm * 0.25)


def test_the_reference_is_zero_on_a_map_and_its_own_reversal():
    a, _ = ref.inputs((2, 3, 8), salt=1)
    loss, stats, da, dm = ref.loss_and_grad(a, torch.flip(a, dims=(1,)))
    assert float(loss) == 0.0 and bool((stats == 0).all()) and bool((da == 0).all()) and bool((dm == 0).all())


def test_the_edge_inputs_pair_every_logit_with_every_other():
    a, m = ref.edge_inputs()
    assert tuple(a.shape) == tuple(m.shape) == (1, 14, 16) and a.dtype == torch.float32
    pairs = {(float(x), float(y)) for x, y in zip(a.reshape(-1), torch.flip(m, dims=(1,)).reshape(-1))}
    values = {float(torch.tensor(s * v, dtype=torch.float32)) for v in ref.EDGE_LOGITS for s in (1.0, -1.0)}      # 1e-3 as fp32
    assert pairs == {(x, y) for x in values for y in values}
    _, stats, da, dm = ref.loss_and_grad(a, m)
    assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(dm).all()) and float(stats[0, 1]) > 0


def test_the_shapes_cover_the_paths():
    assert ref.CHUNK % 1024 == 0
    assert any(w % 4 for _, _, w in ref.SHAPES) and any(h % 2 and h > 1 for _, h, _ in ref.SHAPES)
    assert any(h * w > ref.CHUNK and (h * w) % ref.CHUNK for _, h, w in ref.SHAPES)
    assert (2, 1, ref.CHUNK + 4) in ref.SHAPES and (2, 2, ref.CHUNK // 2 + 4) in ref.SHAPES and (2, 800, 800) in ref.SHAPES


def test_ramp():
    from driving_dirty_amd import consistency
    T = 40
    assert consistency.ramp(0, T) == math.exp(-5.0)
    assert consistency.ramp(T // 2, T) == math.exp(-1.25)
    assert consistency.ramp(T, T) == 1.0 and consistency.ramp(3 * T, T) == 1.0
    assert consistency.ramp(0, 0) == 1.0 and consistency.ramp(7, 0) == 1.0 and consistency.ramp(7, -1) == 1.0
    steps = [consistency.ramp(t, T) for t in range(T + 1)]
    assert all(x < y for x, y in zip(steps, steps[1:]))


def test_workspace_bytes_is_the_headers_formula():
    from driving_dirty_amd import consistency
    assert consistency.CHUNK == ref.CHUNK
    assert consistency.workspace_bytes(1, 4) == 16 and consistency.workspace_bytes(3, ref.CHUNK) == 48
    assert consistency.workspace_bytes(2, ref.CHUNK + 4) == 2 * 2 * 16
    assert consistency.workspace_bytes(32, 640000) == 2 * 8 * 32 * -(-640000 // ref.CHUNK)


@pytest.mark.parametrize("bad", [dict(cons_weight=-0.5), dict(cons_weight=float("nan")), dict(cons_weight=float("inf")), dict(cons_weight="much"),
                                 dict(cons_weight=1.0, cons_rampup_steps=-1), dict(cons_rampup_steps=-3), dict(cons_rampup_steps="soon")])
def test_check_hparams_refuses(bad):
    from argparse import Namespace
    from driving_dirty_amd import consistency
    with pytest.raises(ValueError, match="cons_"):
        consistency.check_hparams(Namespace(**bad))


def test_check_hparams_and_the_flags():
    from argparse import ArgumentParser, Namespace
    from driving_dirty_amd import consistency
    assert consistency.check_hparams(None) == (0.0, 0) and consistency.check_hparams(Namespace()) == (0.0, 0)
    assert consistency.check_hparams(Namespace(cons_weight=2, cons_rampup_steps=100)) == (2.0, 100)
    p = consistency.add_consistency_args(ArgumentParser(add_help=False))
    args = p.parse_args([])
    assert (args.cons_weight, args.cons_rampup_steps) == (0.0, 0) and consistency.check_hparams(args) == (0.0, 0)
    args = p.parse_args(["--cons_weight", "0.5", "--cons_rampup_steps", "4000"])
    assert consistency.check_hparams(args) == (0.5, 4000)
