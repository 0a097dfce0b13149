"""The class-balanced box-map loss on the device (csrc/box_loss.hip: dd_box_loss_fwd, dd_box_loss_bwd; ops.box_loss) against the fp64
reference of tests/_box_loss_ref.py, and the module surface built on it (hparams box_pos_weight / box_bce_weight / box_ts_weight /
box_ts_eps of BBSpatialRoadMap and JointRoadMapBBox).

Bounds, the project's own: the loss and its two components 1e-6 relative against fp64; a gradient 2e-5 of THAT SAMPLE's peak |dL/dp| (the
automatic weights differ by orders of magnitude between samples: a bound from the batch's peak would not see the lightly weighted ones); the
per-sample statistics 1e-6 relative; parameter gradients of a model 2e-4 of each tensor's peak."""
import functools
from argparse import Namespace

import pytest
import torch

import _box_loss_ref as ref

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_OF_PEAK, STATS_RTOL, MODEL_GRAD_OF_PEAK = 1e-6, 2e-5, 1e-6, 2e-4
SHAPES = [(1, 4), (3, 1028), (65, 260), (2, 640000)]
POS_WEIGHTS = [None, 7.5, "auto"]
MIXES = [(1.0, 0.0), (0.0, 1.0), (0.7, 1.3)]
EPSILONS = [1.0, 0.0]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(shape, dev):
    """(p, t) on the device for one of SHAPES; built once, never written to."""
    from driving_dirty_amd import ops
    b, per = shape
    if shape == (3, 1028):          # a ragged last run; sample 1 has an empty target, sample 2 is all ones
        p, t = ref.inputs(b, per, salt=1, empty=(1,), full=(2,))
    elif shape == (2, 640000):      # the product shape: rasterised cars
        p, _ = ref.inputs(b, per, salt=4)
        return p.to(dev), ops.boxes_to_binary_map([synth.car_boxes(60, seed=100 + i) for i in range(b)], dev).reshape(b, per)
    else:
        p, t = ref.inputs(b, per, salt=b)
    return p.to(dev), t.to(dev)


@functools.lru_cache(maxsize=None)
def reference(shape, dev):
    """fp64 pieces of every setting for one shape, computed once: {("bce", pos_weight): (L_bce, dL_bce/dp), ("ts", eps): (L_ts, dL_ts/dp)}.
    The loss is linear in them: L = alpha L_bce + beta L_ts."""
    p, t = case(shape, dev)
    out = {}
    for w in POS_WEIGHTS:
        _, l_bce, _, g = ref.loss_and_grad(p, t, w, 1.0, 0.0)
        out["bce", w] = (l_bce, g)
    for eps in EPSILONS:
        _, _, l_ts, g = ref.loss_and_grad(p, t, None, 0.0, 1.0, eps)
        out["ts", eps] = (l_ts, g)
    return out


def close(got, want, rtol):
    return abs(float(got) - float(want)) <= rtol * abs(float(want))


def grad_excess(got, want):
    """max over the samples of |got - want| / that sample's peak |want| (fp64, on the CPU).  A sample whose gradient is identically zero
    (an empty target under the soft threat score alone with eps = 0: I = 0 and t = 0 everywhere) must come out as exact zeros."""
    got, want = got.detach().double().cpu(), want.double().cpu()
    err, peak = (got - want).abs().amax(dim=1), want.abs().amax(dim=1)
    assert bool((err[peak == 0] == 0).all()), "a zero gradient must be exact"
    return float((err / peak.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------------------ 6. every setting on every shape
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_gradient_and_statistics_against_fp64(dev, shape):
    from driving_dirty_amd import ops
    p, t = case(shape, dev)
    pieces = reference(shape, dev)
    want_stats = ref.stats(p.cpu(), t.cpu())
    assert bool((want_stats[:, 1] + want_stats[:, 0] - want_stats[:, 2] > 0).all())      # U_b > 0: eps = 0 is defined on every sample
    worst = {"loss": 0.0, "grad": 0.0}
    for w in POS_WEIGHTS:
        for alpha, beta in MIXES:
            for eps in EPSILONS:
                (l_bce, g_bce), (l_ts, g_ts) = pieces["bce", w], pieces["ts", eps]
                losses, stats, coef = ops.box_loss_fwd(p, t, w, alpha, beta, eps)
                grad = ops.box_loss_bwd(p, t, coef)
                what = (shape, w, alpha, beta, eps)
                for got, want in zip(losses.tolist(), (alpha * l_bce + beta * l_ts, l_bce, l_ts)):
                    worst["loss"] = max(worst["loss"], abs(got - float(want)) / abs(float(want)))
                    assert close(got, want, LOSS_RTOL), (what, got, float(want))
                assert bool(((stats.cpu() - want_stats).abs() <= STATS_RTOL * want_stats.abs()).all()), (what, stats, want_stats)
                excess = grad_excess(grad, alpha * g_bce + beta * g_ts)
                worst["grad"] = max(worst["grad"], excess)
                assert excess <= GRAD_OF_PEAK, (what, excess)
    print(f"box_loss {shape}: worst relative loss error {worst['loss']:.3e}, worst gradient error {worst['grad']:.3e} of the sample's peak")


# ------------------------------------------------------------------------------------------------ 7. byte targets
@pytest.mark.parametrize("shape", [(3, 1028), (2, 640000)])
def test_byte_targets_give_the_bits_of_the_fp32_target(dev, shape):
    from driving_dirty_amd import ops
    p, t = case(shape, dev)
    losses, stats, coef = ops.box_loss_fwd(p, t, "auto", 0.7, 1.3)
    grad = ops.box_loss_bwd(p, t, coef)
    for tb in (t.to(torch.uint8), t.bool()):
        l2, s2, c2 = ops.box_loss_fwd(p, tb, "auto", 0.7, 1.3)
        assert torch.equal(l2, losses) and torch.equal(s2, stats) and torch.equal(c2, coef)
        assert torch.equal(ops.box_loss_bwd(p, tb, c2), grad)


# ------------------------------------------------------------------------------------------------ 8. determinism
@pytest.mark.parametrize("shape", [(65, 260), (2, 640000)])
def test_two_launches_are_bit_identical(dev, shape):
    from driving_dirty_amd import ops
    p, t = case(shape, dev)
    first = ops.box_loss_fwd(p, t, "auto", 1.0, 1.0)
    second = ops.box_loss_fwd(p, t, "auto", 1.0, 1.0)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert torch.equal(ops.box_loss_bwd(p, t, first[2]), ops.box_loss_bwd(p, t, second[2]))


# ------------------------------------------------------------------------------------------------ 9. the clamps
def test_exact_zero_and_one_probabilities(dev):
    from driving_dirty_amd import ops
    p, t = ref.inputs(2, 1028, salt=2)
    where = [(0, 0), (0, 1), (0, 1026), (0, 1027), (1, 5), (1, 6), (1, 514), (1, 515)]
    for k, (i, j) in enumerate(where):
        p[i, j], t[i, j] = float(k % 2), float((k // 2) % 2)      # p = 0 and p = 1 at both target values, in both samples
    pd, td = p.to(dev), t.to(dev)
    for w, alpha, beta in ((7.5, 1.0, 0.0), ("auto", 0.7, 1.3)):
        want, w_bce, w_ts, g = ref.loss_and_grad(p, t, w, alpha, beta)
        losses, _, coef = ops.box_loss_fwd(pd, td, w, alpha, beta)
        assert bool(torch.isfinite(losses).all())
        assert all(close(a, b, LOSS_RTOL) for a, b in zip(losses.tolist(), (want, w_bce, w_ts)))
        assert float(w_bce) > 100.0 * 4 / (2 * 1028)      # the four clamped elements of weight >= 1 are in it at 100 each
        grad = ops.box_loss_bwd(pd, td, coef)
        assert bool(torch.isfinite(grad).all()) and grad_excess(grad, g) <= GRAD_OF_PEAK
        # the clamped term's slope is zero: what is left at those elements is the other BCE term and the soft threat score's, both finite
        pure_ts = ref.closed_form_grad(p, t, w, 0.0, beta)
        for k, (i, j) in enumerate(where):
            if (k % 2 == 0) == bool(t[i, j]):      # p = 0 with t = 1, p = 1 with t = 0: the whole BCE part is the clamped term
                assert abs(float(grad[i, j]) - float(pure_ts[i, j])) <= 1e-6 * abs(float(pure_ts[i, j])), (w, i, j)


# ------------------------------------------------------------------------------------------------ 10. the existing kernel
def test_unit_weight_is_bce_probs(dev):
    from driving_dirty_amd import ops
    for shape in [(3, 1028), (2, 640000)]:
        p, t = case(shape, dev)
        pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
        old = ops.BceProbs.apply(pa, t)
        new = ops.box_loss(pb, t, pos_weight=1.0, bce_weight=1.0, ts_weight=0.0)
        old.backward()
        new.backward()
        assert close(new.detach(), old.detach(), LOSS_RTOL)
        assert grad_excess(pb.grad, pa.grad) <= GRAD_OF_PEAK


# ------------------------------------------------------------------------------------------------ 11. a sample does not see the batch
def test_a_batch_is_the_mean_of_its_samples(dev):
    from driving_dirty_amd import ops
    p, t = case((3, 1028), dev)
    whole = ops.box_loss_fwd(p, t, "auto", 1.0, 1.0)
    singles = [ops.box_loss_fwd(p[i:i + 1].contiguous(), t[i:i + 1].contiguous(), "auto", 1.0, 1.0) for i in range(3)]
    for k in range(3):
        assert close(whole[0][k], sum(float(s[0][k]) for s in singles) / 3, LOSS_RTOL), k
    assert torch.equal(whole[1], torch.cat([s[1] for s in singles]))      # the statistics of a sample: the same bits alone and in the batch


# ------------------------------------------------------------------------------------------------ 12. autograd
def test_autograd_surface(dev):
    from driving_dirty_amd import ops
    p, t = case((3, 1028), dev)
    _, _, _, g = ref.loss_and_grad(p, t, "auto", 0.7, 1.3)
    kw = dict(pos_weight="auto", bce_weight=0.7, ts_weight=1.3)
    pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
    loss = ops.box_loss(pa, t, **kw)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    (2.5 * ops.box_loss(pb, t, **kw)).backward()
    assert grad_excess(pa.grad, g) <= GRAD_OF_PEAK and grad_excess(pb.grad, 2.5 * g) <= GRAD_OF_PEAK
    assert float((pb.grad - 2.5 * pa.grad).abs().max()) <= 2.0 ** -22 * float(pb.grad.abs().max())      # one more fp32 rounding per element
    total, bce, ts = ops.box_loss(pa, t, return_parts=True, **kw)
    assert torch.equal(total, loss.detach()) and not bce.requires_grad and not ts.requires_grad and bce.dim() == ts.dim() == 0
    assert close(total, 0.7 * float(bce) + 1.3 * float(ts), LOSS_RTOL)
    with torch.no_grad():
        quiet = ops.box_loss(pa, t, **kw)
    assert torch.equal(quiet, loss.detach()) and not quiet.requires_grad
    assert torch.equal(ops.box_loss(p, t.bool(), **kw), quiet)      # no gradient asked for: the forward alone


# ------------------------------------------------------------------------------------------------ 13. refusals
def test_refusals_name_the_entry_point(dev):
    from driving_dirty_amd import _lib, ops
    with pytest.raises(_lib.HotpathError, match="dd_box_loss_fwd.*multiple of 4"):
        ops.box_loss(torch.full((2, 6), 0.5, device=dev), torch.zeros(2, 6, device=dev))
    p, t = case((3, 1028), dev)
    with pytest.raises(_lib.HotpathError, match="dd_box_loss_fwd.*pos_weight"):
        ops.box_loss(p, t, pos_weight=0)
    with pytest.raises(_lib.HotpathError, match="dd_box_loss_fwd"):
        ops.box_loss(p, t, ts_eps=-1.0)
    with pytest.raises(_lib.HotpathError, match="pos_weight"):
        ops.box_loss(p, t, pos_weight="car")
    with pytest.raises(_lib.HotpathError, match="target"):
        ops.box_loss(p, t[:, :1024].contiguous())
    with pytest.raises(_lib.HotpathError, match="target"):
        ops.box_loss(p, t.double())


# ------------------------------------------------------------------------------------------------ 14. / 15. the modules
HP = dict(unfreeze_epoch_no=5, learning_rate=1e-3, output_img_freq=500)
ON = dict(box_pos_weight="auto", box_ts_weight=1.0)


def build_model(dev, **extra):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    model = BBSpatialRoadMap(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=16, latent_dim=8)), **HP, **extra))
    synth.fill_module(model, seed=17)
    return model.to(dev)


def build_joint(dev, **extra):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.joint import JointRoadMapBBox
    model = JointRoadMapBBox(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=16, latent_dim=8)), **HP, **extra))
    synth.fill_module(model, seed=29)
    model = model.to(dev)
    model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0
    return model


def module_batch(dev, b=2):
    views, road = synth.camera_batch(b, seed=17).to(dev), synth.road_maps(b, seed=17).to(dev)
    targets = [synth.car_boxes(n, seed=3 + n) for n in (12, 5)]
    return (tuple(views), tuple({"bounding_box": t} for t in targets), tuple(road))


def test_box_model_trains_on_the_loss(dev):
    model, batch = build_model(dev, **ON), module_batch(dev)
    out = model.training_step(batch, 0)
    assert set(out) == {"loss", "log"} and set(out["log"]) == {"train_loss", "bbox_bce", "bbox_soft_ts"}
    out["loss"].backward()
    params = [(k, q) for k, q in model.named_parameters() if q.requires_grad]
    got = {k: q.grad for k, q in params}
    # the fp64 reference on the step's own probabilities and rasterised target
    _, target, pred = model._run_step(batch, 0, step_name="train")
    want, w_bce, w_ts, dprobs = ref.loss_and_grad(pred, target, "auto", 1.0, 1.0)
    assert close(out["loss"].detach(), want, LOSS_RTOL), (float(out["loss"].detach()), float(want))
    assert close(out["log"]["bbox_bce"], w_bce, LOSS_RTOL) and close(out["log"]["bbox_soft_ts"], w_ts, LOSS_RTOL)
    assert not out["log"]["bbox_bce"].requires_grad and not out["log"]["bbox_soft_ts"].requires_grad
    through = torch.autograd.grad(pred, [q for _, q in params], grad_outputs=dprobs.float().to(dev), allow_unused=True)
    assert any(g is not None for g in through)
    for (k, _), w in zip(params, through):
        assert (got[k] is None) == (w is None), k
        if w is not None:
            err, peak = float((got[k] - w).abs().max()), float(w.abs().max())
            assert err <= MODEL_GRAD_OF_PEAK * peak, (k, err, peak)
    val = model.validation_step(batch, 0)
    assert set(val) == {"val_loss", "val_bce", "val_soft_ts"} and torch.equal(val["val_loss"], out["loss"].detach())
    end = model.validation_epoch_end([val, val])
    assert set(end["log"]) == {"avg_val_loss", "avg_val_bce", "avg_val_soft_ts"}


def test_joint_model_takes_the_same_switch(dev):
    from driving_dirty_amd.spatial import bb_coord_to_map
    model, batch = build_joint(dev, **ON), module_batch(dev)
    out = model.training_step(batch, 0)
    assert set(out["log"]) == {"train_loss", "roadmap_loss", "bbox_loss", "bbox_bce", "bbox_soft_ts"}
    with torch.no_grad():
        _, boxes = model(batch[0], batch[2])
    target = bb_coord_to_map(batch[1], dev)
    want, w_bce, w_ts, _ = ref.loss_and_grad(boxes.reshape(2, -1), target.reshape(2, -1), "auto", 1.0, 1.0)
    assert close(out["log"]["bbox_loss"].detach(), want, LOSS_RTOL), (float(out["log"]["bbox_loss"].detach()), float(want))
    assert close(out["log"]["bbox_bce"], w_bce, LOSS_RTOL) and close(out["log"]["bbox_soft_ts"], w_ts, LOSS_RTOL)
    assert torch.equal(out["loss"], out["log"]["roadmap_loss"] + out["log"]["bbox_loss"])
    out["loss"].backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in model.box_merge.parameters())


def test_off_is_unchanged(dev):
    from driving_dirty_amd import ops
    from driving_dirty_amd.spatial import bb_coord_to_map
    batch = module_batch(dev)
    model = build_model(dev)
    assert model.box_loss is None
    out = model.training_step(batch, 0)
    assert set(out) == {"loss", "log"} and set(out["log"]) == {"train_loss"}
    val = model.validation_step(batch, 0)
    assert set(val) == {"val_loss"}
    with torch.no_grad():
        _, target, pred = model._run_step(batch, 0, step_name="valid")
        assert torch.equal(out["loss"].detach(), ops.BceProbs.apply(pred, target)) and torch.equal(val["val_loss"], out["loss"].detach())
    joint = build_joint(dev)
    assert joint.box_loss is None
    out = joint.training_step(batch, 0)
    assert set(out["log"]) == {"train_loss", "roadmap_loss", "bbox_loss"}
    with torch.no_grad():
        _, boxes = joint(batch[0], batch[2])
        assert torch.equal(out["log"]["bbox_loss"].detach(), ops.BceProbs.apply(boxes.reshape(2, -1), bb_coord_to_map(batch[1], dev).reshape(2, -1)))
