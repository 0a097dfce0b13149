"""The reference of the bootstrapped road-map loss (tests/_topk_loss_ref.py) held to hand-worked cases, and ``topk_loss.keep_now`` pinned:
no GPU needed."""
import math

import pytest
import torch
from torch.nn import functional as F

import _topk_loss_ref as ref


def sp(x):
    return math.log1p(math.exp(-abs(x))) + max(x, 0.0)


def sig(x):
    return 1.0 / (1.0 + math.exp(-x))


Z = torch.tensor([[2.0, -1.0, 0.5, -3.0]])
T = torch.tensor([[0, 1, 1, 0]], dtype=torch.uint8)
U = [2.0, 1.0, -0.5, -3.0]      # the margins: -z where t is set


@pytest.mark.parametrize("keep", [1, 2, 3, 4])
def test_one_sample_of_four_by_hand(keep):
    loss, l_all, stats, dz, mask = ref.loss_and_grad(Z, T, keep)
    assert ref.margins(Z, T).tolist() == [U]
    assert mask.tolist() == [[i < keep for i in range(4)]], "the margins above are in descending order"
    want = sum(sp(u) for u in U[:keep]) / keep
    assert abs(float(loss) - want) < 1e-14
    assert abs(float(l_all) - sum(sp(u) for u in U) / 4) < 1e-14
    assert stats[0].tolist() == pytest.approx([keep, want * keep, U[keep - 1], sum(sp(u) for u in U)], abs=1e-13)
    assert float(stats[0, 0]) == keep and float(stats[0, 2]) == U[keep - 1]
    for i in range(4):
        g = (sig(float(Z[0, i])) - float(T[0, i])) / keep if i < keep else 0.0
        assert abs(float(dz[0, i]) - g) < 1e-14
        assert (float(dz[0, i]) == 0.0) == (i >= keep)


def test_a_tie_at_the_kth_value_keeps_every_tied_pixel():
    z = torch.tensor([[1.0, 1.0, -1.0, 0.0], [0.0, -0.0, 0.0, -0.0]])
    t = torch.tensor([[0, 0, 1, 0], [0, 0, 1, 1]], dtype=torch.uint8)
    tau, mask, n = ref.selection(z, t, 2)
    assert tau.tolist() == [1.0, 0.0] and n.tolist() == [3, 4], "n_b > K; -0 and +0 margins tie"
    assert mask.tolist() == [[True, True, True, False], [True] * 4]
    assert not bool(torch.signbit(ref.margins(z, t)[1]).any()), "-0 is canonicalised to +0"
    loss, _, stats, dz, _ = ref.loss_and_grad(z, t, 2, grad_scale=3.0)
    assert abs(float(loss) - 0.5 * (sp(1.0) + math.log(2.0))) < 1e-14
    assert stats[:, 0].tolist() == [3.0, 4.0]
    assert abs(float(dz[0, 2]) - 3.0 * (sig(-1.0) - 1.0) / (2 * 3)) < 1e-14 and float(dz[0, 3]) == 0.0
    assert abs(float(dz[1, 2]) - 3.0 * (0.5 - 1.0) / (2 * 4)) < 1e-14


def test_keep_all_is_binary_cross_entropy_with_logits():
    z, t = ref.logits_and_target((3, 40), salt=1)
    loss, l_all, stats, dz, mask = ref.loss_and_grad(z, t, 40)
    zd = z.double().requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(zd, t.double())
    (gw,) = torch.autograd.grad(want, zd)
    want = want.detach()
    assert bool(mask.all()) and stats[:, 0].tolist() == [40.0] * 3
    assert abs(float(loss) - float(want)) < 1e-14 and abs(float(l_all) - float(want)) < 1e-14
    assert float((dz - gw).abs().max()) < 1e-16
    assert torch.equal(stats[:, 2].float(), ref.margins(z, t).min(1).values), "tau_b is the sample's minimum"


def test_keys_and_floats_are_inverse_and_ordered():
    xs = [float(torch.tensor(x, dtype=torch.float32)) for x in (-float("inf"), -3.0, -1e-40, 0.0, 1e-40, 1.0, float("inf"))]
    assert xs[2] < 0.0 < xs[4] < 1e-38, "denormals"
    keys = [ref.key_of_float(x) for x in xs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert ref.floats_of_keys(keys).tolist() == xs
    assert ref.key_of_float(0.0) == 0x80000000 and ref.key_of_float(-0.0) == 0x7fffffff, "why -0 is canonicalised first"
    assert sum(ref.DIGIT_BITS) == 32 and ref.BINS == sum(1 << b for b in ref.DIGIT_BITS)


def test_keep_now_is_pinned():
    from driving_dirty_amd.topk_loss import keep_now
    per, frac, T = 640000, 0.25, 100
    assert [keep_now(frac, T, t, per) for t in (0, T // 2, T, 2 * T)] == [640000, 400000, 160000, 160000]
    assert keep_now(frac, 0, 0, per) == keep_now(frac, 0, 7, per) == keep_now(frac, -3, 7, per) == 160000
    assert keep_now(0.25, 0, 0, 10) == 3, "ceil(2.5)"
    assert keep_now(1e-9, 0, 0, 640000) == 1 and keep_now(1.0, 5, 3, 640000) == 640000
    assert keep_now(0.1, 4, 1, 1000) == math.ceil((1.0 - 0.9 * 0.25) * 1000)
