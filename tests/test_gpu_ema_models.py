"""GPU tests of weight averaging in the training step: ``train.TrainStep(ema_decay=...)`` and ``ema.WeightEMA`` on
the small model of tests/test_gpu_grad_clip.py -- ``BasicAE(hidden 16, latent 8, 16 x 132)`` under ``RoadMapBCE``, ``big_numel=4096``
so that a Linear takes the rank-B pass on the side stream -- and once on the box model.  Seeded ``synth`` batches, B = 2, 6 steps.

The shadows are held to the fp64 recurrence over snapshots of the live weights taken after every step, within the k-step bound of
tests/_ema_ref.py.  That is also the stream-ordering test: an update that ran ahead of a side-stream pass would have averaged the
previous step's weights, which are a whole Adam step (lr = 1e-2) away."""
from argparse import Namespace

import pytest
import torch

import _ema_ref as ref

pytestmark = pytest.mark.gpu

B, STEPS, LR, DECAY = 2, 6, 1e-2, 0.9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import ema
    ema.lib()
    return torch.device("cuda:0")


def tiny_model(dev, **hp):
    from driving_dirty_amd import synth
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))
    model = RoadMapBCE(Namespace(**{"pretrained_ae": ae, "unfreeze_epoch_no": 0, "learning_rate": LR, "output_img_freq": 500, **hp}))
    synth.fill_module(model, seed=77)
    model = model.to(dev)
    model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0
    return model


def tiny_batch(dev, step):
    from driving_dirty_amd import synth
    views = synth.camera_batch(B, 16, 22, seed=100 + 10 * step).to(dev)
    road = synth.road_maps(B, seed=100 + 10 * step).to(dev)
    return (tuple(views), None, tuple(road))


def train_step(model, **kw):
    from driving_dirty_amd.train import TrainStep
    return TrainStep(model, **{"lr": LR, "big_numel": 4096, "scheduler": False, **kw})


def weights(model):
    torch.cuda.synchronize()
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def shadows(ema):
    torch.cuda.synchronize()
    return {k: s.detach().clone() for k, s in zip(ema.names, ema.shadows)}


def same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(ref.bits(a[k]), ref.bits(b[k])) for k in a)


class Recurrence:
    """The fp64 recurrence over snapshots of the weights, with the running maximum the k-step bound needs."""

    def __init__(self, start):
        self.e = {k: v.double().cpu() for k, v in start.items()}
        self.m = {k: v.abs() for k, v in self.e.items()}

    def update(self, snapshot, alpha):
        for k, w in snapshot.items():
            self.m[k] = torch.maximum(self.m[k], ref.magnitude(self.e[k], w))
            self.e[k] = ref.update(self.e[k], w, alpha)

    def check(self, got, alpha, what):
        for k, e in self.e.items():
            ref.assert_within(got[k], e, ref.k_step_bound(self.m[k], alpha), f"{what}: {k}")


def check_twins_and_recurrence(dev, make_model, make_batch, steps, what, **kw):
    on, off = make_model(), make_model()
    assert same_bits(weights(on), weights(off))
    step_on, step_off = train_step(on, ema_decay=DECAY, **kw), train_step(off, **kw)
    assert step_off.ema is None and step_on.ema.decay == DECAY
    assert same_bits(shadows(step_on.ema), weights(on)), "the shadows start bit-equal to the weights"
    rec, alpha = Recurrence(weights(on)), 1.0 - DECAY
    try:
        for i in range(steps):
            batch = make_batch(i)
            loss_on, loss_off = step_on(batch, i)["loss"].detach().clone(), step_off(batch, i)["loss"].detach().clone()
            w = weights(on)
            assert torch.equal(ref.bits(loss_on), ref.bits(loss_off)) and same_bits(w, weights(off)), f"{what}: step {i} differs with the average on"
            rec.update(w, alpha)
            rec.check(shadows(step_on.ema), alpha, f"{what} step {i}")
        assert step_on.ema.num_updates == step_on.ema.steps == steps
        assert step_on.fused and step_off.fused, "a Linear should have taken the rank-B pass"
    finally:
        step_on.close()
        step_off.close()


@pytest.mark.parametrize("overlap", [True, False])
def test_training_is_not_disturbed_and_the_shadow_is_the_recurrence(dev, overlap):
    check_twins_and_recurrence(dev, lambda: tiny_model(dev), lambda i: tiny_batch(dev, i), STEPS, f"overlap {overlap}", adam_overlap=overlap)


def test_the_box_model(dev):
    """BBSpatialRoadMap at the size its other tests use (hidden 16, latent 8, 256 x 306): another parameter list, two steps."""
    from driving_dirty_amd import synth
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.spatial import BBSpatialRoadMap

    def make_model():
        ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8))
        model = BBSpatialRoadMap(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=LR, output_img_freq=500, mse_loss=False))
        synth.fill_module(model, seed=17)
        model = model.to(dev)
        model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0
        return model

    def make_batch(i):
        views, road = synth.camera_batch(B, seed=31 + i).to(dev), synth.road_maps(B, seed=31 + i).to(dev)
        return (tuple(views), tuple({"bounding_box": synth.car_boxes(8 + j, seed=40 + 2 * i + j)} for j in range(B)), tuple(road))

    check_twins_and_recurrence(dev, make_model, make_batch, 2, "box model")


def test_frozen_parameters_are_left_out_exactly_until_the_model_unfreezes(dev):
    model = tiny_model(dev, unfreeze_epoch_no=1)
    assert model.frozen and not any(p.requires_grad for p in model.ae.parameters())
    step = train_step(model, ema_decay=DECAY)
    start, alpha = weights(model), 1.0 - DECAY
    rec = Recurrence(start)
    try:
        for i in range(3):
            step(tiny_batch(dev, i), i)
            rec.update(weights(model), alpha)
        w, s = weights(model), shadows(step.ema)
        frozen = [k for k in w if k.startswith("ae.")]
        assert frozen and len(frozen) < len(w)
        assert len(step.ema._tables()[0]) == len(w) - len(frozen), "the frozen tensors are not in the update's table"
        for k in w:
            if k.startswith("ae."):
                assert torch.equal(ref.bits(s[k]), ref.bits(w[k])) and torch.equal(ref.bits(w[k]), ref.bits(start[k])), k
            else:
                assert not torch.equal(s[k], start[k]) and not torch.equal(s[k], w[k]), f"{k}: the head's shadow has moved"
        rec.check(s, alpha, "frozen")
        model.current_epoch = 1      # training_step unfreezes the extractor; the listener rebuilds the table
        for i in range(3, 6):
            step(tiny_batch(dev, i), i)
            rec.update(weights(model), alpha)
            assert not model.frozen and len(step.ema._tables()[0]) == len(w)
        w, s = weights(model), shadows(step.ema)
        assert any(not torch.equal(w[k], start[k]) for k in frozen), "the extractor trains after the unfreeze"
        rec.check(s, alpha, "unfrozen")      # for ae.* the recurrence over steps 0..2 is the identity: it starts at the unfreeze
    finally:
        step.close()


def test_every_third_step_makes_two_updates_in_six_steps(dev):
    model = tiny_model(dev)
    step = train_step(model, ema_decay=DECAY, ema_every=3)
    rec, alpha = Recurrence(weights(model)), 1.0 - DECAY ** 3
    try:
        for i in range(STEPS):
            before = shadows(step.ema)
            step(tiny_batch(dev, i), i)
            if i % 3 == 2:
                rec.update(weights(model), alpha)
                assert step.ema.alpha() == alpha
            else:
                assert same_bits(shadows(step.ema), before), f"step {i} makes no update"
        assert step.ema.num_updates == 2 and step.ema.steps == STEPS
        rec.check(shadows(step.ema), alpha, "every 3")
    finally:
        step.close()


@pytest.fixture(scope="module")
def trained(dev):
    """Six steps with the average on; -> (model, step, the views to predict from)."""
    model = tiny_model(dev)
    step = train_step(model, ema_decay=DECAY)
    for i in range(STEPS):
        step(tiny_batch(dev, i), i)
    torch.cuda.synchronize()
    model.eval()
    yield model, step, torch.stack(tiny_batch(dev, 99)[0])
    step.close()


def test_averaged_applies_the_shadows_and_restores_the_weights(dev, trained):
    model, step, x = trained
    live, avg = weights(model), shadows(step.ema)
    outside = model.predict_road_map(x).clone()
    with step.averaged() as inner:
        assert inner is model and same_bits(weights(model), avg) and same_bits(shadows(step.ema), live)
        inside = model.predict_road_map(x).clone()
        with pytest.raises(RuntimeError, match="applied"):
            step.ema.update()
        with pytest.raises(RuntimeError, match="applied"):
            step.ema.state_dict()
    assert same_bits(weights(model), live) and same_bits(shadows(step.ema), avg)
    assert inside.dtype == torch.bool and int((inside != outside).sum()) > 0, "the averaged weights predict another map"
    assert torch.equal(model.predict_road_map(x), outside)
    with pytest.raises(KeyError, match="from the body"):
        with step.averaged():
            assert same_bits(weights(model), avg)
            raise KeyError("from the body")
    assert same_bits(weights(model), live) and same_bits(shadows(step.ema), avg) and not step.ema.is_applied
    before = {k: p.data_ptr() for k, p in model.named_parameters()}
    with step.averaged():
        assert before == {k: p.data_ptr() for k, p in model.named_parameters()}, "the parameters' storages keep their addresses"


def test_the_averaged_checkpoint_is_an_ordinary_checkpoint(dev, trained, tmp_path):
    from driving_dirty_amd.roadmap import RoadMapBCE
    model, step, x = trained
    live, avg = weights(model), shadows(step.ema)
    buffers = {k: b.detach().clone() for k, b in model.named_buffers()}
    with step.averaged():
        inside = model.predict_road_map(x).clone()
    path = str(tmp_path / "averaged.ckpt")
    step.ema.save_checkpoint(path)
    assert same_bits(weights(model), live) and same_bits(shadows(step.ema), avg), "the live model is unchanged"
    loaded = RoadMapBCE.load_from_checkpoint(path).to(dev).eval()
    loaded.ae.encoder.fc1.drop_p = loaded.ae.encoder.fc2.drop_p = 0.0
    assert same_bits(weights(loaded), avg)
    assert all(torch.equal(b, buffers[k]) for k, b in loaded.named_buffers()), "buffers are the live model's"
    assert torch.equal(loaded.predict_road_map(x), inside)


def test_a_state_dict_resumes_to_the_same_bits(dev):
    from driving_dirty_amd.ema import WeightEMA
    model = tiny_model(dev)
    step = train_step(model, ema_decay=DECAY, ema_warmup=True)
    try:
        for i in range(3):
            step(tiny_batch(dev, i), i)
        state = step.ema.state_dict()
        assert set(state) == {"shadows", "num_updates", "steps", "decay", "every", "warmup"}
        assert set(state["shadows"]) == {k for k, _ in model.named_parameters()} and state["num_updates"] == state["steps"] == 3
        fresh = WeightEMA(model, 0.5, every=2)
        fresh.load_state_dict(state)
        assert (fresh.decay, fresh.every, fresh.warmup, fresh.num_updates, fresh.steps) == (DECAY, 1, True, 3, 3)
        assert same_bits(shadows(fresh), shadows(step.ema))
        for i in range(3, 6):
            step(tiny_batch(dev, i), i)
            assert fresh.alpha() == 1.0 - min(DECAY, (1 + i) / (10 + i))
            fresh.update()
        assert same_bits(shadows(fresh), shadows(step.ema)) and fresh.num_updates == step.ema.num_updates == 6
        fresh.close()
    finally:
        step.close()


def test_a_parameter_the_kernels_cannot_take_is_refused_by_name(dev):
    from driving_dirty_amd.ema import HotpathError, WeightEMA
    net = torch.nn.Linear(4, 3).to(dev)
    net.bias.data = net.bias.data.double()
    with pytest.raises(HotpathError, match="'bias'"):
        WeightEMA(net, 0.9)
    net = torch.nn.Linear(4, 3).to(dev)
    net.weight.data = torch.zeros(4, 3, device=dev).t()
    with pytest.raises(HotpathError, match="'weight'"):
        WeightEMA(net, 0.9)
