"""GPU tests of the bootstrapped road-map loss (csrc/topk_loss.hip, include/dd_topk_loss.h) against tests/_topk_loss_ref.py.

The bounds are the reference module's, stated before any kernel ran: ``n_b``, ``tau_b`` and the SET of non-zero gradient positions exact
(the selection is defined on bits: zero mismatches, no case left out); the loss, ``L_all`` and the per-sample sums within 2e-5 of
themselves; the gradient within 2e-5 of its peak; ``probs`` the bits of ``ops.sigmoid``.

The key cases are built from integer keys mapped back to floats: margins that differ only in the lowest key bit, only in the top
digit, and at every boundary of the 11 / 11 / 10-bit digit plan.

Observed on an MI355X: every n_b, tau_b and selected set exact; the loss, L_all and the sums within 3.3e-7 of themselves, the gradient
within 1.7e-7 of its peak (at (2, 640000), K = P/4: 1.5e-9 and 1.5e-7)."""
import numpy as np
import pytest
import torch

import _topk_loss_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import topk_loss
    topk_loss.lib()
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def check(dev, z, t, keep, grad_scale=1.0, label=""):
    """One call held to the reference; returns the call's outputs on the CPU."""
    from driving_dirty_amd import ops, topk_loss
    zg, tg = z.to(dev).contiguous(), t.to(dev).contiguous()
    losses, probs, stats, dz = topk_loss.fwd(zg, tg, keep, grad=True, grad_scale=grad_scale)
    torch.cuda.synchronize()
    w_loss, w_all, w_stats, w_dz, w_mask = ref.loss_and_grad(z, t, keep, grad_scale)
    losses, probs, stats, dz = losses.cpu(), probs.cpu(), stats.cpu(), dz.cpu()
    assert torch.equal(stats[:, 0], w_stats[:, 0]), (label, "n_b", stats[:, 0].tolist(), w_stats[:, 0].tolist())
    assert torch.equal(stats[:, 2], w_stats[:, 2]), (label, "tau_b", stats[:, 2].tolist(), w_stats[:, 2].tolist())
    assert bool((stats[:, 0] >= keep).all())
    # the selected set: outside it the gradient is exactly zero, inside it non-zero -- read wherever sig - t cannot round to zero in
    # fp32 (the kernel's sigmoid is within 3 x 2^-24 absolute: past |z| = 17 under the matching label 1 - p is 0, a magnitude
    # question the gradient bound below answers; n_b and tau_b above pin the set there)
    live = (torch.sigmoid(z.double()) - t.double()).abs() > 1e-6
    mism = int(((dz != 0) != w_mask)[live].sum()) + int((dz[~w_mask] != 0).sum())
    assert mism == 0, (label, f"{mism} positions of the selected set differ")
    e_loss = abs(float(losses[0]) - float(w_loss)) / abs(float(w_loss))
    e_all = abs(float(losses[1]) - float(w_all)) / abs(float(w_all))
    e_sel = float(((stats[:, 1] - w_stats[:, 1]).abs() / w_stats[:, 1].abs()).max())
    e_tot = float(((stats[:, 3] - w_stats[:, 3]).abs() / w_stats[:, 3].abs()).max())
    e_grad = ref.peak_error(dz, w_dz)
    print(f"{label} {tuple(z.shape)} K={keep}: loss {e_loss:.2e} L_all {e_all:.2e} sums {e_sel:.2e} {e_tot:.2e} (bound {ref.LOSS_REL}); "
          f"grad {e_grad:.2e} of peak (bound {ref.GRAD_OF_PEAK}); n_b {stats[:, 0].tolist()[:4]}")
    assert max(e_loss, e_all, e_sel, e_tot) <= ref.LOSS_REL and e_grad <= ref.GRAD_OF_PEAK
    assert torch.equal(bits(probs), bits(ops.sigmoid(zg))), (label, "probs are ops.sigmoid's bits")
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(stats).all())
    return losses, probs, stats, dz


def test_one_sample_of_four_for_every_keep(dev):
    z = torch.tensor([[2.0, -1.0, 0.5, -3.0]])
    t = torch.tensor([[0, 1, 1, 0]], dtype=torch.uint8)
    for keep in (1, 2, 3, 4):
        _, _, stats, _ = check(dev, z, t, keep, label="by hand")
        assert stats[0, 0] == keep and stats[0, 2] == [2.0, 1.0, -0.5, -3.0][keep - 1]


def test_three_samples_with_a_threshold_each(dev):
    z = torch.tensor([[0.5, -1.5, 2.5, -3.5, 4.5, -5.5, 6.5, -7.5]]).repeat(3, 1)
    t = torch.tensor([[0] * 8, [1] * 8, [0, 1, 1, 0, 0, 1, 1, 0]], dtype=torch.uint8)
    for keep in (1, 3, 5, 8):
        _, _, stats, _ = check(dev, z, t, keep, label="3 x 8")
        if keep < 8:
            assert len(set(stats[:, 2].tolist())) == 3, "a different tau_b per sample"


def test_a_constant_map_keeps_every_pixel(dev):
    """Every pixel ties: n_b = P at K = 1; every element falls into one bin of every digit -- the worst case of the histogram."""
    for per in (8, ref.CHUNK + 4):
        z = torch.full((2, per), -1.25)
        t = torch.zeros((2, per), dtype=torch.uint8)
        _, _, stats, _ = check(dev, z, t, 1, label="constant")
        assert stats[:, 0].tolist() == [per, per] and stats[:, 2].tolist() == [-1.25, -1.25]


def key_cases():
    """(label, int64 keys [B, P]): margins built from their keys."""
    base = ref.key_of_float(1.5)
    low = [base + i for i in range(8)]                                       # differ in the lowest key bits only
    # differ in the top digit only; exponents up to 2^92, so that a thread's fp32 sum of eight such margins stays far from overflow
    top = [(d << 21) | 0x12345 for d in (150, 200, 1023, 1024, 1500, 1900, 1700, 300)]
    edges = []
    for boundary in (0x5a4 << 21, (0x5a3 << 21) | (0x156 << 10)):           # both sides of a top-digit and of a middle-digit boundary
        edges += [boundary - 1, boundary, boundary + 1, boundary - 2]
    mid = [(0x5a3 << 21) | (m << 10) | 0x3ff for m in (0, 1, 2046, 2047, 1024, 1023, 7, 8)]      # differ in the middle digit only
    last = [(0x5a3 << 21) | (0x2aa << 10) | l for l in (0, 1, 1022, 1023, 512, 511, 3, 4)]       # differ in the last digit only
    return [("lowest bits", [low]), ("top digit", [top]), ("digit boundaries", [edges]), ("middle digit", [mid]), ("last digit", [last]),
            ("all at once", [low, top, edges, mid, last])]


@pytest.mark.parametrize("label,keys", key_cases(), ids=[c[0].replace(" ", "_") for c in key_cases()])
def test_margins_built_from_keys(dev, label, keys):
    u = torch.stack([ref.floats_of_keys(k) for k in keys])
    assert bool(torch.isfinite(u).all()) and u.shape[1] == 8
    g = torch.Generator().manual_seed(5)
    t = (torch.rand(u.shape, generator=g) < 0.5).to(torch.uint8)
    z = torch.where(t.bool(), -u, u)      # so that the margins are u
    assert torch.equal(ref.margins(z, t), u)
    for keep in range(1, 9):
        check(dev, z, t, keep, label=label)


def test_mixed_signs_with_the_kth_value_negative_zero_and_positive(dev):
    z = torch.tensor([[3.0, 1.0, 0.0, -0.0, -1.0, -2.0, 0.5, -0.5]])
    t = torch.zeros((1, 8), dtype=torch.uint8)
    for keep, tau in ((2, 1.0), (3, 0.5), (4, 0.0), (5, 0.0), (6, -0.5), (8, -2.0)):
        _, _, stats, _ = check(dev, z, t, keep, label="signs")
        assert float(stats[0, 2]) == tau
    _, _, stats, _ = check(dev, z, t, 4, label="signs")
    assert float(stats[0, 0]) == 5, "+0 and -0 tie"


def test_signed_zero_logits_under_both_labels(dev):
    z = torch.tensor([[0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0]])
    t = torch.tensor([[0, 0, 1, 1, 0, 0, 1, 0]], dtype=torch.uint8)
    for keep in (1, 2, 7, 8):
        _, _, stats, _ = check(dev, z, t, keep, label="zeros")
    assert float(stats[0, 2]) == -1.0
    _, _, stats, _ = check(dev, z, t, 2, label="zeros")
    assert float(stats[0, 0]) == 7 and float(stats[0, 2]) == 0.0 and not np.signbit(float(stats[0, 2]))


def test_denormal_margins(dev):
    d = float(torch.tensor(1e-40, dtype=torch.float32))
    z = torch.tensor([[1e-40, -1e-40, 2e-40, -2e-40, 0.0, 1e-38, -1e-38, 3e-40]])
    t = torch.tensor([[0, 0, 1, 1, 0, 0, 0, 1]], dtype=torch.uint8)
    assert 0 < d < 1.2e-38
    for keep in range(1, 9):
        check(dev, z, t, keep, label="denormals")
    _, _, stats, _ = check(dev, z, t, 3, label="denormals")
    assert float(stats[0, 2]) == d and float(stats[0, 0]) == 3, "1e-38 > 2e-40 > 1e-40: ordered as keys, not flushed"


@pytest.mark.parametrize("shape", [(2, ref.CHUNK + 4), (2, 2 * ref.CHUNK - 4)], ids=["chunk+4", "2chunk-4"])
def test_a_piece_boundary_inside_a_sample(dev, shape):
    z, t = ref.logits_and_target(shape, salt=2)
    for keep in (1, 5, shape[1] // 4, shape[1] - 1, shape[1]):
        check(dev, z, t, keep, label="pieces")


@pytest.mark.parametrize("batch", [33, 65])
def test_more_samples_than_the_small_launches_have_waves(dev, batch):
    z, t = ref.logits_and_target((batch, 8), salt=3)
    for keep in (1, 3, 8):
        check(dev, z, t, keep, label="batch")


def test_the_pointer_table_gives_the_stacked_bits(dev):
    from driving_dirty_amd import topk_loss
    z, t = ref.logits_and_target((64, 8), salt=4)
    want = check(dev, z, t, 3, label="stacked 64 x 8")
    zg = z.to(dev)
    masks = tuple(row.clone() for row in t.to(dev))
    for target in (masks, tuple(m.bool() for m in masks)):
        got = topk_loss.fwd(zg, target, 3)
        for a, b in zip(got, want):
            assert torch.equal(bits(a), bits(b))
    # 65 masks: past the table's size the tuple is stacked
    z, t = ref.logits_and_target((65, 8), salt=4)
    got = topk_loss.fwd(z.to(dev), tuple(row.clone() for row in t.to(dev)), 3)
    want = topk_loss.fwd(z.to(dev), t.to(dev), 3)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want))
    z2, t2 = ref.logits_and_target((2, ref.CHUNK + 4), salt=6)
    got = topk_loss.fwd(z2.to(dev), tuple(row.clone() for row in t2.to(dev)), 100)
    want = topk_loss.fwd(z2.to(dev), t2.to(dev), 100)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want))


@pytest.fixture(scope="module")
def road_map(dev):
    z, t = ref.logits_and_target((2, 640000), salt=5)
    return z, t, check(dev, z, t, 160000, grad_scale=2.0, label="road map")


def test_the_road_map_at_a_quarter(dev, road_map):
    _, _, (losses, probs, stats, dz) = road_map
    assert bool((stats[:, 0] >= 160000).all()) and float(losses[0]) > float(losses[1]), "the hardest quarter's mean exceeds the mean"


def test_call_properties_on_the_road_map(dev, road_map):
    from driving_dirty_amd import topk_loss
    z, t, (losses, probs, stats, dz) = road_map
    zg, tg = z.to(dev), t.to(dev)
    again = topk_loss.fwd(zg, tg, 160000, grad_scale=2.0)
    for a, b in zip(again, (losses, probs, stats, dz)):
        assert torch.equal(bits(a), bits(b)), "two runs give the same bits"
    l1, _, s1, d1 = topk_loss.fwd(zg, tg, 160000, grad_scale=1.0)
    assert torch.equal(bits(d1 * 2.0), bits(dz)), "grad_scale scales the gradient"
    l0, p0, s0, d0 = topk_loss.fwd(zg, tg, 160000, grad=False, want_probs=False)
    assert d0 is None and p0 is None
    assert torch.equal(bits(l0), bits(losses)) and torch.equal(bits(s0), bits(stats)), "dlogits = NULL gives the same bits of loss and stats"
    table = topk_loss.fwd(zg, tuple(row.clone() for row in tg), 160000, grad_scale=2.0)
    for a, b in zip(table, (losses, probs, stats, dz)):
        assert torch.equal(bits(a), bits(b)), "the table form gives the stacked form's bits"


def test_keep_all_is_the_mean_bce(dev):
    from driving_dirty_amd import ops
    z, t = ref.logits_and_target((2, ref.CHUNK + 4), salt=7)
    per = z.shape[1]
    losses, _, stats, dz = check(dev, z, t, per, label="K = P")
    zg = z.to(dev).requires_grad_(True)
    loss, _ = ops.BceWithLogitsProbs.apply(zg, t.to(dev))
    loss.backward()
    loss = loss.detach()
    assert abs(float(losses[0]) - float(loss)) <= ref.LOSS_REL * float(loss) and abs(float(losses[0]) - float(losses[1])) <= 1e-6 * float(loss)
    assert ref.peak_error(dz, zg.grad.cpu().double()) <= ref.GRAD_OF_PEAK
    assert torch.equal(stats[:, 2].float(), ref.margins(z, t).min(1).values)


def test_edge_logits_under_both_labels_stay_finite(dev):
    v = torch.tensor([s * x for x in ref.EDGE_LOGITS for s in (1.0, -1.0)], dtype=torch.float32)      # 14 values
    z = torch.cat([v, v, v[:4]]).reshape(1, 32).repeat(2, 1)
    t = torch.cat([torch.zeros(14), torch.ones(14), torch.tensor([0.0, 1.0, 1.0, 0.0])]).to(torch.uint8).reshape(1, 32).repeat(2, 1)
    t[1] = 1 - t[1]
    for keep in (1, 4, 16, 31, 32):
        check(dev, z, t, keep, label="edges")


def test_nan_logits_finish_inside_the_buffers(dev):
    from driving_dirty_amd import topk_loss
    z, t = ref.logits_and_target((2, 16), salt=8)
    z[0, 3] = float("nan")
    z[1, 0] = -float("nan")
    losses, probs, stats, dz = topk_loss.fwd(z.to(dev), t.to(dev), 4)
    torch.cuda.synchronize()
    assert bool((stats[:, 0] >= 4).all()) and bool((stats[:, 0] <= 16).all())


def test_autograd_through_the_function(dev):
    from driving_dirty_amd import topk_loss
    z, t = ref.logits_and_target((3, 40), salt=9)
    w_loss, _, w_stats, w_dz, _ = ref.loss_and_grad(z, t, 10, grad_scale=0.5)
    zg = z.to(dev).requires_grad_(True)
    loss, probs, stats = topk_loss.topk_bce(zg, t.to(dev), 10)
    assert not probs.requires_grad and not stats.requires_grad and loss.dim() == 0
    (0.5 * loss).backward()
    assert abs(float(loss) - float(w_loss)) <= ref.LOSS_REL * float(w_loss)
    assert ref.peak_error(zg.grad, w_dz) <= ref.GRAD_OF_PEAK and torch.equal(stats.cpu()[:, 0], w_stats[:, 0])
    with torch.no_grad():
        loss2, _, _ = topk_loss.topk_bce(zg, tuple(row.clone() for row in t.to(dev)), 10)
    assert torch.equal(bits(loss2), bits(loss))
    with pytest.raises(topk_loss.HotpathError, match="floating-point target"):
        topk_loss.topk_bce(zg, t.to(dev).float(), 10)
    with pytest.raises(topk_loss.HotpathError, match="keep = 41"):
        topk_loss.topk_bce(zg, t.to(dev), 41)
