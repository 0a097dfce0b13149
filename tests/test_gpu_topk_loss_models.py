"""GPU tests of the bootstrapped road-map loss inside ``RoadMapBCE``: the smoke-sized model -- hidden 16, latent 8, views
16 x 22, dropout off -- on B = 2 scenes.

The step's loss is held to the reference (tests/_topk_loss_ref.py) recomputed in fp64 from the model's own logits (2e-5 relative, the
kernel bound); the parameter gradients to those of the same HIP forward with the loss written in fp32 torch ops on the logits (2e-4 of
each tensor's peak, the project's model bound, as tests/test_gpu_consistency_models.py uses).  With the setting off the step gives the
bits of a model built without the hparams; validation under the setting gives the bits of the parent's ``validation_step``.

Observed on an MI355X: the loss within 4e-8 relative of the fp64 value, the parameter gradients within 1.4e-5 of their tensor's peak."""
from argparse import Namespace

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _topk_loss_ref as ref

pytestmark = pytest.mark.gpu

B, H, W, P = 2, 16, 22, 640000


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def tiny_model(dev, lr=1e-2, **hp):
    from driving_dirty_amd import synth
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=H, input_width=6 * W))
    model = RoadMapBCE(Namespace(**{"pretrained_ae": ae, "unfreeze_epoch_no": 0, "learning_rate": lr, "output_img_freq": 500, **hp}))
    synth.fill_module(model, seed=77)
    model = model.to(dev)
    model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0
    return model


def tiny_batch(dev, seed=100):
    """(sample, None, road_image): fp32 views and bool masks as the collate's tuples."""
    from driving_dirty_amd import synth
    views = synth.camera_batch(B, H, W, seed=seed).to(dev)
    road = synth.road_maps(B, seed=seed).to(dev)
    return (tuple(views), None, tuple(road))


def bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def train_logits(model, batch):
    """The logits of the training step's forward: the extractor unfrozen, its BatchNorms on the batch's statistics."""
    model.frozen = False
    model.ae.unfreeze()
    with torch.no_grad():
        return model._logits(batch[0])


def test_the_steps_loss_is_the_reference_on_the_models_own_logits(dev):
    from driving_dirty_amd import topk_loss
    frac = 0.25
    model = tiny_model(dev, rm_topk_frac=frac)
    batch = tiny_batch(dev)
    assert batch[2][0].dtype == torch.bool
    z = train_logits(model, batch).reshape(B, -1)
    keep = topk_loss.keep_now(frac, 0, 0, P)
    assert keep == 160000
    w_loss, w_all, w_stats, _, _ = ref.loss_and_grad(z, torch.stack(batch[2]).reshape(B, -1), keep)
    out = model.training_step(batch, 0)
    got, log = float(out["loss"].detach().double()), out["log"]
    print(f"loss {got!r}, fp64 {float(w_loss)!r}; L_all {float(log['rm_bce_all'])!r}, fp64 {float(w_all)!r}")
    assert set(log) == {"train_loss", "rm_bce_all", "rm_topk_kept", "rm_topk_tau"}
    assert abs(got - float(w_loss)) <= ref.LOSS_REL * float(w_loss)
    assert abs(float(log["rm_bce_all"]) - float(w_all)) <= ref.LOSS_REL * float(w_all)
    assert float(w_loss) > (1 + 50 * ref.LOSS_REL) * float(w_all), "the hardest quarter's mean is fifty bounds from the mean at least: a step that took the plain loss would show"
    assert abs(float(log["rm_topk_kept"]) - float(w_stats[:, 0].sum()) / (B * P)) <= 1e-7
    assert abs(float(log["rm_topk_tau"]) - float(w_stats[:, 2].mean())) <= 1e-6 * abs(float(w_stats[:, 2].mean()))
    assert not any(v.requires_grad for k, v in log.items() if k != "train_loss") and model.topk_step == 1


def test_parameter_gradients_equal_those_of_the_torch_composition(dev):
    """The same HIP forward; the loss once from the kernels and once as fp32 torch ops on the logits."""
    model = tiny_model(dev, rm_topk_frac=0.25)
    batch = tiny_batch(dev)
    params = [(k, q) for k, q in model.named_parameters() if q.requires_grad]
    out = model.training_step(batch, 0)
    params = [(k, q) for k, q in model.named_parameters() if q.requires_grad]      # the step has unfrozen the extractor
    got = torch.autograd.grad(out["loss"], [q for _, q in params], allow_unused=True)
    z = model._logits(batch[0]).reshape(B, -1)
    t = torch.stack(batch[2]).reshape(B, -1)
    u = torch.where(t, -z, z)
    tau = torch.topk(u.detach(), 160000, dim=1).values[:, -1:]
    mask = u.detach() >= tau
    total = ((F.softplus(u) * mask).sum(1) / mask.sum(1)).mean()
    assert abs(float(total.detach()) - float(out["loss"].detach())) <= 1e-5 * float(total.detach())
    want = torch.autograd.grad(total, [q for _, q in params], allow_unused=True)
    want_of = {k: w for (k, _), w in zip(params, want)}
    worst = 0.0
    for (k, _), g, w in zip(params, got, want):
        assert (g is None) == (w is None), k
        if w is None:
            continue
        err, peak = float((g - w).abs().max()), float(w.abs().max())
        if k.endswith("bias") and (k.split(".")[-2] in ("c1", "c2", "c3") or k.endswith(".fc1.bias")):
            # a bias in front of a train-mode BatchNorm: its gradient is exactly zero and either side holds the rounding noise of a
            # column sum; judged against its weight's peak, as tests/test_gpu_consistency_models.py does
            peak = max(peak, float(want_of[k[:-len("bias")] + "weight"].abs().max()))
        worst = max(worst, err / max(peak, 1e-300))
        assert err <= ref.MODEL_GRAD_OF_PEAK * peak, (k, err, peak)
    print(f"worst parameter-gradient error {worst:.3e} of its tensor's peak (bound {ref.MODEL_GRAD_OF_PEAK})")


def test_with_the_setting_off_the_step_is_the_parents(dev, monkeypatch):
    from driving_dirty_amd import topk_loss
    batch = tiny_batch(dev)
    plain = tiny_model(dev).training_step(batch, 0)
    assert set(plain["log"]) == {"train_loss"}

    def entered(*a, **k):
        raise AssertionError("a step with the setting off entered libdd_topk_loss.so")
    monkeypatch.setattr(topk_loss, "launch", entered)
    for model in (tiny_model(dev, rm_topk_frac=1.0), tiny_model(dev, rm_topk_frac=1, rm_topk_warmup_steps=9), tiny_model(dev, rm_topk_frac=None)):
        out = model.training_step(batch, 0)
        assert torch.equal(bits(out["loss"]), bits(plain["loss"])) and set(out["log"]) == {"train_loss"}
        assert model.topk is None and model.topk_step == 0


def test_validation_under_the_setting_is_the_parents(dev, monkeypatch):
    from driving_dirty_amd import topk_loss
    batch = tiny_batch(dev)
    want = tiny_model(dev).validation_step(batch, 0)

    def entered(*a, **k):
        raise AssertionError("validation entered libdd_topk_loss.so")
    monkeypatch.setattr(topk_loss, "launch", entered)
    model = tiny_model(dev, rm_topk_frac=0.25, rm_topk_warmup_steps=3)
    got = model.validation_step(batch, 0)
    assert set(got) == set(want) == {"val_loss", "val_ts", "val_ts_rounded"}
    for k in want:
        assert torch.equal(bits(got[k]), bits(want[k])), k
    assert model.topk_step == 0
    assert model.predict_road_map(batch[0]).dtype == torch.bool


def test_the_anneal_falls_from_all_pixels_to_the_fraction(dev):
    from driving_dirty_amd import topk_loss
    frac, T = 0.1, 4
    model = tiny_model(dev, rm_topk_frac=frac, rm_topk_warmup_steps=T)
    batch = tiny_batch(dev)
    seen = []
    real = topk_loss.fwd
    stats_of = []

    def spy(logits, target, keep, **kw):
        out = real(logits, target, keep, **kw)
        stats_of.append((keep, out[2]))
        return out
    topk_loss.fwd, saved = spy, topk_loss.fwd
    try:
        for t in range(T + 2):
            seen.append(float(model.training_step(batch, t)["log"]["rm_topk_kept"]))
    finally:
        topk_loss.fwd = saved
    print("kept:", seen)
    assert seen[0] == 1.0 and all(a >= b for a, b in zip(seen, seen[1:])) and seen[T] == seen[T + 1]
    assert frac <= seen[T] <= frac + 1e-3, "ties may keep a few more than K"
    for t, (keep, stats) in enumerate(stats_of):
        assert keep == topk_loss.keep_now(frac, T, t, P) and bool((stats[:, 0] >= keep).all())
    assert model.topk_step == T + 2


def test_stacked_masks_and_the_tuple_give_the_same_bits(dev):
    """The tuple takes the pointer table; a logging step (``output_img_freq``) stacks the masks first."""
    batch = tiny_batch(dev)
    a = tiny_model(dev, rm_topk_frac=0.25).training_step(batch, 0)
    model = tiny_model(dev, rm_topk_frac=0.25)
    z = train_logits(model, batch).reshape(B, -1).requires_grad_(True)
    l1, p1 = model._loss_and_probs(z, batch[2], train=True)
    l2, p2 = model._loss_and_probs(z, torch.stack(batch[2]).reshape(B, -1), train=True)
    l3, _ = model._loss_and_probs(z, torch.stack(batch[2]).reshape(B, -1).to(torch.uint8), train=True)
    assert torch.equal(bits(l1), bits(l2)) and torch.equal(bits(l1), bits(l3)) and torch.equal(bits(p1), bits(p2))
    assert torch.equal(bits(l1), bits(a["loss"]))
    g1, = torch.autograd.grad(l1, z)
    g2, = torch.autograd.grad(l2, z)
    assert torch.equal(bits(g1), bits(g2))


def test_a_checkpoint_round_trip_keeps_the_hparams(dev, tmp_path):
    from driving_dirty_amd.roadmap import RoadMapBCE
    model = tiny_model(dev, rm_topk_frac=0.25, rm_topk_warmup_steps=400)
    model.training_step(tiny_batch(dev), 0)
    path = str(tmp_path / "topk.ckpt")
    model.save_checkpoint(path)
    again = RoadMapBCE.load_from_checkpoint(path)
    assert again.topk == (0.25, 400) and again.topk_step == 0 and model.topk_step == 1


def test_one_train_step_against_a_materialised_gradient_twin(dev):
    """The parameters after one ``TrainStep`` equal those of a ``TrainStep(fuse_linear_wgrad=False)`` twin within 1e-6 of each tensor's peak:
    the bound of tests/test_gpu_round5.py, with its exception -- the Linear bias in front of a train-mode BatchNorm."""
    from driving_dirty_amd.train import TrainStep
    a, b = tiny_model(dev, rm_topk_frac=0.25), tiny_model(dev, rm_topk_frac=0.25)
    ta = TrainStep(a, lr=1e-2, big_numel=4096, scheduler=False, fuse_linear_wgrad=False)
    tb = TrainStep(b, lr=1e-2, big_numel=4096, scheduler=False)
    try:
        batch = tiny_batch(dev)
        la, lb = ta(batch, 0)["loss"], tb(batch, 0)["loss"]
        torch.cuda.synchronize()
        assert float(la.detach()) == float(lb.detach())
        assert {id(w) for w in tb.fused} == {id(b.fc1.weight), id(b.ae.encoder.fc1.fc1.weight)} and not ta.fused
        assert a.fc1.weight.grad is not None and b.fc1.weight.grad is None
        for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            if k.endswith("fc1.fc1.bias"):
                continue
            d = float((p.detach() - q.detach()).abs().max() / p.detach().abs().max().clamp_min(1e-30))
            assert d <= 1e-6, (k, d)
    finally:
        ta.close()
        tb.close()


def test_under_cons_weight_the_loss_is_the_sum_of_the_two(dev):
    """One 4-tuple step: the supervised rows of the longer forward take the bootstrapped loss, the unlabelled ones the consistency loss."""
    import _consistency_ref as cref
    from driving_dirty_amd import augment, consistency, synth, topk_loss, tta
    weight, rampup, b_u = 50.0, 2, 2
    model = tiny_model(dev, rm_topk_frac=0.25, cons_weight=weight, cons_rampup_steps=rampup)
    batch = tiny_batch(dev)
    # fp32 views as ToTensor makes them of uint8 frames (a true division on the CPU), as tests/test_gpu_consistency_models.py builds them
    u8 = (synth.camera_batch(b_u, H, W, seed=101) * 255).round().to(torch.uint8)
    unlabelled = tuple(torch.from_numpy(u8.numpy().astype("float32") / np.float32(255.0)).contiguous().to(dev))
    plain = augment.augment_views(unlabelled, [0] * b_u, torch.tensor([1.0, 0.0]).repeat(b_u, 6, 1))
    assert torch.equal(plain, torch.stack(unlabelled)), "the identity draw moves values bit for bit"
    rows = tuple(batch[0]) + tuple(plain) + tuple(tta.mirror_views(unlabelled))
    z = train_logits(model, (rows,))
    assert tuple(z.shape) == (B + 2 * b_u, 800, 800)
    l_topk, _, _, _, _ = ref.loss_and_grad(z[:B].reshape(B, -1), torch.stack(batch[2]).reshape(B, -1), 160000)
    l_cons, _, _, _ = cref.loss_and_grad(z[B:B + b_u], z[B + b_u:])
    out = model.training_step(batch + (unlabelled,), 0)
    now = weight * consistency.ramp(0, rampup)
    want = float(l_topk) + now * float(l_cons)
    got = float(out["loss"].detach().double())
    print(f"loss {got!r}, fp64 {want!r} = {float(l_topk)!r} + {now!r} * {float(l_cons)!r}")
    assert abs(got - want) <= ref.LOSS_REL * want
    assert {"rm_bce_all", "rm_topk_kept", "rm_topk_tau", "cons_loss", "cons_weight_now"} <= set(out["log"])
    assert model.topk_step == 1 and model.cons_step == 1
