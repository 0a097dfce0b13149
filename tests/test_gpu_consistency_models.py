"""GPU tests of the mirror consistency loss inside ``RoadMapBCE``: the smoke-sized model -- hidden 16, latent 8, views
16 x 22, dropout off -- on ``B_l = 2`` labelled and ``B_u = 2`` unlabelled scenes, ``N = 6`` rows in one forward.

The step's loss is held to ``L_sup + w ramp L_cons`` recomputed in fp64 from the model's own logits of the same six rows (2e-5 relative,
the kernel bound); the parameter gradients to those of the same HIP forward with the consistency term written in fp32 torch ops on
the logits (2e-4 of each tensor's peak, the project's model bound).  With the hparams off, or on a batch without an unlabelled part,
the step gives the bits of a model built without them and never enters the new library.

Observed on an MI355X: the loss within 9e-9 relative of the fp64 value, the parameter gradients within 2.3e-7 of their tensor's peak."""
from argparse import Namespace

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _consistency_ref as ref

pytestmark = pytest.mark.gpu

B_L, B_U, H, W = 2, 2, 16, 22
AUG_ON = dict(aug_mirror=0.5, aug_brightness=0.2, aug_contrast=0.2, aug_per_view=0.1, aug_view_drop=0.3, aug_seed=11)


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


def frames(dev, b, seed):
    """uint8 frames [b,6,H,W,3], and the fp32 views ToTensor makes of them: a true division, taken on the CPU (on the device torch
    multiplies by the reciprocal of a scalar divisor, which is not the same fp32 value for every byte)."""
    from driving_dirty_amd import synth
    u8 = (synth.camera_batch(b, H, W, seed=seed) * 255).round().to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous()
    f32 = torch.from_numpy(u8.permute(0, 1, 4, 2, 3).numpy().astype("float32") / np.float32(255.0)).contiguous()
    return u8.to(dev), f32.to(dev)


def tiny_batch(dev, b_u=B_U, seed=100, b_l=B_L):
    """(sample, None, road_image, unlabelled): fp32 views as the collate's tuples."""
    from driving_dirty_amd import synth
    views = synth.camera_batch(b_l, H, W, seed=seed).to(dev)
    road = synth.road_maps(b_l, seed=seed).to(dev)
    _, unlabelled = frames(dev, b_u, seed + 1)
    return (tuple(views), None, tuple(road), tuple(unlabelled))


def six_rows(batch):
    """The rows the step forwards when the augmenter is off: the labelled scenes, the unlabelled ones, their mirrors."""
    from driving_dirty_amd import augment, tta
    b_u = len(batch[3])
    plain = augment.augment_views(batch[3], [0] * b_u, torch.tensor([1.0, 0.0]).repeat(b_u, 6, 1))
    assert torch.equal(plain, torch.stack(batch[3])), "the identity draw moves values bit for bit"
    return tuple(batch[0]) + tuple(plain) + tuple(tta.mirror_views(batch[3]))


def bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def test_the_loss_is_the_supervised_loss_plus_the_weighted_consistency_term(dev):
    """Two steps on the same batch (no optimizer: the same logits): t = 0 and t = 1 of a two-step ramp."""
    from driving_dirty_amd import consistency
    weight, rampup = 50.0, 2
    model = tiny_model(dev, cons_weight=weight, cons_rampup_steps=rampup)
    batch = tiny_batch(dev)
    model.frozen = False
    model.ae.unfreeze()      # what the first training_step does: the extractor in train mode, its BatchNorms on the batch's statistics
    with torch.no_grad():
        z = model._logits(six_rows(batch))
    assert tuple(z.shape) == (B_L + 2 * B_U, 800, 800)
    target = torch.stack(batch[2]).double().cpu()
    l_sup = float(F.binary_cross_entropy_with_logits(z[:B_L].double().cpu(), target))
    l_cons, stats, _, _ = ref.loss_and_grad(z[B_L:B_L + B_U], z[B_L + B_U:])
    assert float(l_cons) > 0 and float(stats[:, 1].sum()) > 0, "the mirrored scenes' maps differ from the scenes'"
    for t in range(2):
        out = model.training_step(batch, t)
        now = weight * consistency.ramp(t, rampup)
        want = l_sup + now * float(l_cons)
        got, log = float(out["loss"].detach().double()), out["log"]
        print(f"t = {t}: loss {got!r}, fp64 {want!r} = {l_sup!r} + {now!r} * {float(l_cons)!r}")
        assert set(log) == {"train_loss", "cons_loss", "cons_disagree", "cons_weight_now"}
        assert abs(got - want) <= ref.LOSS_REL * want
        assert abs(float(log["cons_loss"]) - float(l_cons)) <= ref.LOSS_REL * float(l_cons) and not log["cons_loss"].requires_grad
        assert float(log["cons_disagree"]) == float(stats[:, 1].sum()) / (B_U * 640000)
        assert log["cons_weight_now"] == now and model.cons_step == t + 1
    assert now * float(l_cons) > 10 * ref.LOSS_REL * want, "at t = 1 the consistency term is ten times the bound at least: a wrong weight would show"


def test_parameter_gradients_equal_those_of_the_torch_composition(dev):
    """The same HIP forward and supervised loss; the consistency term once from the kernels and once as fp32 torch ops on the logits."""
    weight = 2.0
    model = tiny_model(dev, cons_weight=weight)
    batch = tiny_batch(dev)
    params = [(k, q) for k, q in model.named_parameters() if q.requires_grad]
    out = model.training_step(batch, 0)
    got = torch.autograd.grad(out["loss"], [q for _, q in params], allow_unused=True)
    z = model._logits(six_rows(batch))
    l_sup, _ = model._loss_and_probs(z[:B_L].reshape(B_L, -1), batch[2])
    d = torch.sigmoid(z[B_L:B_L + B_U]) - torch.flip(torch.sigmoid(z[B_L + B_U:]), dims=(1,))
    total = l_sup + weight * (d * d).mean()
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
            # column sum; judged against its weight's peak, as tests/test_gpu_rm_loss_models.py does
            peak = max(peak, float(want_of[k[:-len("bias")] + "weight"].abs().max()))
        worst = max(worst, err / max(peak, 1e-300))
        assert err <= ref.MODEL_GRAD_OF_PEAK * peak, (k, err, peak)
    print(f"worst parameter-gradient error {worst:.3e} of its tensor's peak (bound {ref.MODEL_GRAD_OF_PEAK})")


def test_without_an_unlabelled_part_or_with_the_weight_off_the_step_is_the_parents(dev, monkeypatch):
    from driving_dirty_amd import consistency
    batch = tiny_batch(dev)
    plain = tiny_model(dev).training_step(batch[:3], 0)
    assert set(plain["log"]) == {"train_loss"}

    def entered(*a, **k):
        raise AssertionError("a supervised-only step entered libdd_consistency.so")
    monkeypatch.setattr(consistency, "launch", entered)
    on = tiny_model(dev, cons_weight=0.5, cons_rampup_steps=3)
    for model in (on, tiny_model(dev, cons_weight=0.0, cons_rampup_steps=0), tiny_model(dev, cons_weight=0.0, cons_rampup_steps=9)):
        out = model.training_step(batch[:3], 0)
        assert torch.equal(bits(out["loss"]), bits(plain["loss"])) and set(out["log"]) == {"train_loss"}
        assert model.cons_step == 0
    for model in (tiny_model(dev), tiny_model(dev, cons_weight=0.0)):
        with pytest.raises(ValueError, match="cons_weight is 0"):
            model.training_step(batch, 0)


def test_the_ramp_advances_only_on_batches_with_an_unlabelled_part(dev):
    from driving_dirty_amd import consistency
    model = tiny_model(dev, cons_weight=0.5, cons_rampup_steps=3)
    batch = tiny_batch(dev)
    seen = []
    for i, with_unlabelled in enumerate((True, False, True, False, True, True, True)):
        out = model.training_step(batch if with_unlabelled else batch[:3], i)
        if with_unlabelled:
            seen.append(out["log"]["cons_weight_now"])
            assert {"cons_loss", "cons_disagree", "cons_weight_now"} <= set(out["log"])
        else:
            assert set(out["log"]) == {"train_loss"}
    assert seen == [0.5 * consistency.ramp(t, 3) for t in range(5)] and seen[3] == seen[4] == 0.5 and model.cons_step == 5


def test_every_form_of_the_unlabelled_scenes_gives_the_same_bits(dev):
    """uint8 frames and the fp32 views ToTensor makes of them, each as the collate's tuple and stacked; and uint8 labelled frames."""
    model = tiny_model(dev, cons_weight=1.0)
    batch = tiny_batch(dev)
    u8, f32 = frames(dev, B_U, 101)
    assert torch.equal(f32, torch.stack(batch[3]))
    outs = [model.training_step(batch[:3] + (form,), 0) for form in (tuple(f32), f32, tuple(u8), u8)]
    for out in outs[1:]:
        assert torch.equal(bits(out["loss"]), bits(outs[0]["loss"]))
        assert torch.equal(bits(out["log"]["cons_loss"]), bits(outs[0]["log"]["cons_loss"]))
        assert torch.equal(bits(out["log"]["cons_disagree"]), bits(outs[0]["log"]["cons_disagree"]))
    l8, lf = frames(dev, B_L, 55)
    a = model.training_step((tuple(l8), None, batch[2], tuple(u8)), 0)
    b = model.training_step((tuple(lf), None, batch[2], tuple(f32)), 0)
    assert torch.equal(bits(a["loss"]), bits(b["loss"])), "uint8 labelled frames are converted by the identity draw: ToTensor's values"


def test_an_enabled_augmenter_draws_from_its_own_generator(dev):
    """Two identically built models with a fixed ``aug_seed`` give the same losses step after step, torch's global generators are not
    touched, and the unlabelled part takes two draws per step."""
    batch = tiny_batch(dev)
    a, b = tiny_model(dev, cons_weight=1.0, **AUG_ON), tiny_model(dev, cons_weight=1.0, **AUG_ON)
    assert a.augment.enabled
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    la = [a.training_step(batch, i)["loss"].detach() for i in range(3)]
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), gpu_state)
    lb = [b.training_step(batch, i)["loss"].detach() for i in range(3)]
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(la, lb))
    assert not torch.equal(la[0], la[1]), "the draws differ from step to step"
    draws = []
    own = a.augment.draw
    a.augment.draw = lambda n: draws.append(n) or own(n)
    a.training_step(batch, 3)
    assert draws == [B_L, B_U, B_U]
    off = tiny_model(dev, cons_weight=1.0)
    state = off.augment._gen.get_state()
    off.training_step(batch, 0)
    assert torch.equal(off.augment._gen.get_state(), state), "a disabled augmenter draws nothing"


def test_one_train_step_keeps_the_rank_b_pass(dev):
    """``N = 6 <= 64``: ``fc1.weight.grad`` stays None, the big Linear layers' gradients are formed inside their Adam pass.  The parameters
    after the step equal those of a ``TrainStep(fuse_linear_wgrad=False)`` twin within 1e-6 of each tensor's peak: the bound at which
    tests/test_gpu_round5.py (test_trainstep_rankb_matches_the_materialised_gradient_path) holds the rank-B pass against materialised
    gradients, with the same exception -- the Linear bias in front of a train-mode BatchNorm, whose gradient is rounding noise."""
    from driving_dirty_amd.train import TrainStep
    a, b = tiny_model(dev, cons_weight=1.0), tiny_model(dev, cons_weight=1.0)
    ta = TrainStep(a, lr=1e-2, big_numel=4096, scheduler=False, fuse_linear_wgrad=False)
    tb = TrainStep(b, lr=1e-2, big_numel=4096, scheduler=False)
    try:
        batch = tiny_batch(dev)
        la, lb = ta(batch, 0)["loss"], tb(batch, 0)["loss"]
        torch.cuda.synchronize()
        assert float(la.detach()) == float(lb.detach())
        assert {id(w) for w in tb.fused} == {id(b.fc1.weight), id(b.ae.encoder.fc1.fc1.weight)} and not ta.fused
        assert a.fc1.weight.grad is not None and b.fc1.weight.grad is None and b.ae.encoder.fc1.fc1.weight.grad is None
        for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            if k.endswith("fc1.fc1.bias"):
                continue
            d = float((p.detach() - q.detach()).abs().max() / p.detach().abs().max().clamp_min(1e-30))
            assert d <= 1e-6, (k, d)
    finally:
        ta.close()
        tb.close()


def test_one_train_step_at_48_rows_keeps_the_rank_b_pass(dev):
    """``B_l = 16``, ``B_u = 16``: ``N = 16 + 2 * 16 = 48`` rows, the production batch of the consistency step.  More than 32 rows: both big
    Linear layers take the two-chunk form of the rank-B pass with a half-filled second chunk (the head on one k-tile per n-group, the
    encoder's fc1 on 17).  Same twin and same bounds as ``test_one_train_step_keeps_the_rank_b_pass``."""
    from driving_dirty_amd.train import TrainStep
    a, b = tiny_model(dev, cons_weight=1.0), tiny_model(dev, cons_weight=1.0)
    ta = TrainStep(a, lr=1e-2, big_numel=4096, scheduler=False, fuse_linear_wgrad=False)
    tb = TrainStep(b, lr=1e-2, big_numel=4096, scheduler=False)
    try:
        batch = tiny_batch(dev, b_u=16, b_l=16)
        la, lb = ta(batch, 0)["loss"], tb(batch, 0)["loss"]
        torch.cuda.synchronize()
        assert float(la.detach()) == float(lb.detach())
        assert {id(w) for w in tb.fused} == {id(b.fc1.weight), id(b.ae.encoder.fc1.fc1.weight)} and not ta.fused
        assert a.fc1.weight.grad is not None and tuple(a.fc1.weight.grad.shape) == (640000, 8)
        assert b.fc1.weight.grad is None and b.fc1.bias.grad is None and b.ae.encoder.fc1.fc1.weight.grad is None
        worst = 0.0
        for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            if k.endswith("fc1.fc1.bias"):
                continue
            d = float((p.detach() - q.detach()).abs().max() / p.detach().abs().max().clamp_min(1e-30))
            worst = max(worst, d)
            assert d <= 1e-6, (k, d)
        print(f"48 rows: worst parameter difference {worst:.3e} of its tensor's peak (bound 1e-6)")
    finally:
        ta.close()
        tb.close()


def test_one_train_step_past_64_rows_materialises_the_gradient(dev):
    """``N = 2 + 2 * 32 = 66 > 64``: ``HipAdam.linear_factors`` declines the rank-B pass by itself; the step runs."""
    from driving_dirty_amd.train import TrainStep
    model = tiny_model(dev, cons_weight=1.0)
    ts = TrainStep(model, lr=1e-2, big_numel=4096, scheduler=False)
    try:
        before = model.fc1.weight.detach().clone()
        out = ts(tiny_batch(dev, b_u=32), 0)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out["loss"])) and model.cons_step == 1
        assert model.fc1.weight.grad is not None and tuple(model.fc1.weight.grad.shape) == (640000, 8)
        assert not torch.equal(model.fc1.weight.detach(), before), "the optimizer stepped"
    finally:
        ts.close()
