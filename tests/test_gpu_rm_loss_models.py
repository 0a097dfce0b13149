"""GPU tests of the road-map loss in the models: the tiny ``RoadMapBCE`` of tests/test_gpu_ema_models.py and the small
joint model of tests/_joint_cases.py under ``rm_ts_weight=1, rm_pos_weight="auto"``.

The parameter gradients of one step are held to fp64 autograd of the reference loss (tests/_rm_loss_ref.py) on the model's OWN logits,
carried through the model's backward: within 2e-4 of each tensor's peak, the project's model bound.  With the flags off the step makes
the calls recorded for the parent (tests/golden/abi_call_trace.json) and never enters the new library."""
import importlib.util
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import _joint_cases as J
import _rm_loss_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON = dict(rm_ts_weight=1.0, rm_pos_weight="auto")
OFF = dict(rm_pos_weight=None, rm_bce_weight=1.0, rm_ts_weight=0.0, rm_ts_eps=1.0)
B = 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def tiny_model(dev, **hp):
    from driving_dirty_amd import synth
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))
    model = RoadMapBCE(Namespace(**{"pretrained_ae": ae, "unfreeze_epoch_no": 0, "learning_rate": 1e-2, "output_img_freq": 500, **hp}))
    synth.fill_module(model, seed=77)
    model = model.to(dev)
    model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0
    return model


def tiny_batch(dev, step=0):
    from driving_dirty_amd import synth
    views = synth.camera_batch(B, 16, 22, seed=100 + 10 * step).to(dev)
    road = synth.road_maps(B, seed=100 + 10 * step).to(dev)
    return (tuple(views), None, tuple(road))


def joint_batch(dev):
    from driving_dirty_amd import synth
    views, road = J.views_and_roads(dev, B)
    return (tuple(views), tuple({"bounding_box": synth.car_boxes(n, seed=3 + n)} for n in (12, 5)), tuple(road))


def check_parameter_gradients(model, logits, masks, loss_rm, parts, extra_loss=None):
    """``loss_rm`` and ``parts`` against the fp64 reference on ``logits`` [B, P]; then every parameter gradient of ``loss_rm`` (+
    ``extra_loss``) against the reference's dL/dlogits carried through the model's own backward (+ the backward of ``extra_loss``)."""
    b = logits.shape[0]
    target = torch.stack(tuple(masks)).reshape(b, -1).float()
    want, w_bce, w_ts, dz = ref.loss_and_grad(logits.detach(), target, "auto", 1.0, 1.0)
    for got, r, bound in zip((loss_rm.detach(), *parts), (want, w_bce, w_ts), ref.loss_bounds(logits.detach().cpu(), target.cpu(), "auto", 1.0, 1.0, 1.0)):
        assert abs(float(got) - float(r)) <= bound, (float(got), float(r), bound)
    assert not parts[0].requires_grad and not parts[1].requires_grad
    params = [(k, q) for k, q in model.named_parameters() if q.requires_grad]
    total = loss_rm if extra_loss is None else loss_rm + extra_loss
    got = torch.autograd.grad(total, [q for _, q in params], retain_graph=True, allow_unused=True)
    outputs, seeds = [logits], [dz.float().to(logits.device)]
    if extra_loss is not None:
        outputs, seeds = outputs + [extra_loss], seeds + [torch.ones_like(extra_loss)]
    through = torch.autograd.grad(outputs, [q for _, q in params], grad_outputs=seeds, allow_unused=True)
    assert any(g is not None for g in through)
    worst, want_of = 0.0, {k: w for (k, _), w in zip(params, through)}
    for (k, _), g, w in zip(params, got, through):
        assert (g is None) == (w is None), k
        if w is not None:
            err, peak = float((g - w).abs().max()), float(w.abs().max())
            if k.endswith("bias") and (k.split(".")[-2] in ("c1", "c2", "c3") or k.endswith(".fc1.bias")):
                # a bias in front of a train-mode BatchNorm: its gradient is exactly zero and either side holds the rounding noise of a
                # column sum; judged against its weight's peak, as tests/test_gpu_heads.py does
                peak = max(peak, float(want_of[k[:-len("bias")] + "weight"].abs().max()))
            worst = max(worst, err / max(peak, 1e-300))
            assert err <= ref.MODEL_GRAD_OF_PEAK * peak, (k, err, peak)
    return worst


def test_road_map_model_trains_on_the_loss(dev):
    """Both branches of ``RoadMapBCE._run_step``: the training step reads the collate's masks through the pointer table, any other
    step stacks them."""
    from driving_dirty_amd import ops
    model = tiny_model(dev, **ON)
    batch = tiny_batch(dev, 0)
    assert model.rm_loss == {"pos_weight": "auto", "bce_weight": 1.0, "ts_weight": 1.0, "ts_eps": 1.0}
    out = model.training_step(batch, 0)
    assert set(out) == {"loss", "log"} and set(out["log"]) == {"train_loss", "rm_bce", "rm_soft_ts"}
    for step_name in ("train", "valid"):
        loss, target_rm, logits, probs = model._run_step(batch, 0, step_name=step_name)
        assert (target_rm is None) == (step_name == "train")
        assert torch.equal(loss.detach(), out["loss"].detach()), "the two branches give the same bits"
        assert torch.equal(probs, ops.sigmoid(logits.detach().contiguous()))
        worst = check_parameter_gradients(model, logits.reshape(B, -1), batch[2], loss, model._rm_parts)
        print(f"RoadMapBCE under the road-map loss ({step_name} branch): worst parameter-gradient error {worst:.3e} of its tensor's peak "
              f"(bound {ref.MODEL_GRAD_OF_PEAK})")


def test_road_map_validation_reports_the_parts_and_calibrates_from_the_new_probs(dev):
    model = tiny_model(dev, calibrate_threshold=True, **ON)
    batch = tiny_batch(dev, 1)
    val = model.validation_step(batch, 0)
    assert set(val) == {"val_loss", "val_ts", "val_ts_rounded", "val_rm_bce", "val_rm_soft_ts", "ts_hist"}
    target = torch.stack(batch[2]).reshape(B, -1).float()
    with torch.no_grad():
        logits = model._logits(batch[0]).reshape(B, -1)
    want, w_bce, w_ts, _ = ref.loss_and_grad(logits, target, "auto", 1.0, 1.0)
    for got, r, bound in zip((val["val_loss"], val["val_rm_bce"], val["val_rm_soft_ts"]), (want, w_bce, w_ts),
                             ref.loss_bounds(logits.cpu(), target.cpu(), "auto", 1.0, 1.0, 1.0)):
        assert abs(float(got.detach()) - float(r)) <= bound
    end = model.validation_epoch_end([val, val])
    assert {"avg_val_loss", "avg_val_ts", "avg_val_ts_rounded", "avg_val_rm_bce", "avg_val_rm_soft_ts", "best_threshold"} <= set(end["log"])
    assert torch.equal(end["log"]["avg_val_rm_bce"], val["val_rm_bce"]) and model.rm_threshold is not None
    off = tiny_model(dev)
    assert set(off.validation_step(batch, 0)) == {"val_loss", "val_ts", "val_ts_rounded"}
    assert set(off.training_step(batch, 0)["log"]) == {"train_loss"}


def test_joint_model_takes_the_same_switch(dev):
    model = J.build_joint(dev, **ON)
    batch = joint_batch(dev)
    out = model.training_step(batch, 0)
    assert set(out["log"]) == {"train_loss", "roadmap_loss", "bbox_loss", "rm_bce", "rm_soft_ts"}
    s = model._run_step(batch, False, False)
    assert torch.equal(s["loss_rm"].detach(), out["log"]["roadmap_loss"].detach())
    worst = check_parameter_gradients(model, s["logits"].reshape(B, -1), batch[2], s["loss_rm"], s["rm_parts"], extra_loss=s["loss_bb"])
    print(f"JointRoadMapBBox under the road-map loss: worst parameter-gradient error {worst:.3e} of its tensor's peak (bound {ref.MODEL_GRAD_OF_PEAK})")
    val = model.validation_step(batch, 0)
    assert {"val_loss", "val_roadmap_loss", "val_bbox_loss", "val_rm_bce", "val_rm_soft_ts", "val_ts", "val_ts_rounded"} == set(val)
    assert torch.equal(val["val_loss"], val["val_roadmap_loss"] + val["val_bbox_loss"])
    end = model.validation_epoch_end([val, val])
    assert {"avg_val_rm_bce", "avg_val_rm_soft_ts", "avg_val_loss"} <= set(end["log"])
    stacked = (torch.stack(batch[0]), batch[1], torch.stack(batch[2]))      # the other branch of _step_inputs: an fp32 target
    with torch.no_grad():
        s2 = model._run_step(stacked, False, True)
    assert torch.equal(s2["loss_rm"], s["loss_rm"].detach()) and torch.equal(s2["probs"], val_probs(model, s))


def val_probs(model, s):
    from driving_dirty_amd import ops
    return ops.sigmoid(s["logits"].detach().contiguous())


def test_a_checkpoint_round_trips_the_hparams(dev, tmp_path):
    from driving_dirty_amd.roadmap import RoadMapBCE
    flags = dict(rm_pos_weight="auto", rm_bce_weight=0.7, rm_ts_weight=1.3, rm_ts_eps=0.5)
    model = tiny_model(dev, **flags)
    batch = tiny_batch(dev, 2)
    path = str(tmp_path / "rm_loss.ckpt")
    model.save_checkpoint(path)
    again = RoadMapBCE.load_from_checkpoint(path).to(dev)
    again.ae.encoder.fc1.drop_p = again.ae.encoder.fc2.drop_p = 0.0
    assert again.rm_loss == model.rm_loss == {"pos_weight": "auto", "bce_weight": 0.7, "ts_weight": 1.3, "ts_eps": 0.5}
    assert {k: getattr(again.hparams, k) for k in flags} == flags
    assert torch.equal(again.training_step(batch, 0)["loss"].detach(), model.training_step(batch, 0)["loss"].detach())


def test_with_the_flags_off_the_step_makes_the_parents_calls(dev, monkeypatch):
    """The recorder of tools/record_abi_call_trace.py around its road-map step, once with no ``rm_*`` hparam and once with all four at
    their defaults: both are the call list recorded for the parent, and the new library is never entered."""
    from driving_dirty_amd import rm_loss, synth
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    spec = importlib.util.spec_from_file_location("record_abi_call_trace", os.path.join(ROOT, "tools", "record_abi_call_trace.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(ROOT, "tests", "golden", "abi_call_trace.json")) as f:
        golden = json.load(f)["roadmap_fp32"]

    def entered(*a, **k):
        raise AssertionError("a model with the rm_* flags off entered libdd_rm_loss.so")
    monkeypatch.setattr(rm_loss, "launch", entered)

    def step(**hp):      # record_abi_call_trace.roadmap_fp32 with ``hp`` added
        torch.manual_seed(0)
        with rec.Recorder() as calls:
            ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))
            model = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-2, output_img_freq=500, **hp))
            synth.fill_module(model, seed=77)
            model = model.to(dev)
            np.random.seed(5)
            batches = [(tuple(synth.camera_batch(3, 16, 22, seed=100 + 10 * s).to(dev)), None, tuple(synth.road_maps(3, seed=100 + 10 * s).to(dev)))
                       for s in range(2)]
            rec._train(model, batches, lr=1e-2, big_numel=4096)
        return json.loads(json.dumps(calls))

    for hp in ({}, OFF):
        calls = step(**hp)
        assert len(calls) == len(golden) and all(a == b for a, b in zip(calls, golden)), hp
        assert any(c[0] == "dd_bce_logits_u8_ptrs" for c in calls)
    # ... and the joint model's step with the flags off makes the calls it makes without them
    batch = joint_batch(dev)
    traces = []
    for hp in ({}, OFF):
        model = J.build_joint(dev, **hp)
        with rec.Recorder() as calls:
            model.training_step(batch, 0)["loss"].backward()
        traces.append(json.loads(json.dumps(calls)))
    assert traces[0] == traces[1] and any(c[0] == "dd_bce_logits_u8_ptrs" for c in traces[0])
