"""GPU tests of the sampled prediction's uncertainty in the model: ``RoadMapBCE.predict_uncertainty`` against the fp64
oracle's per-draw passes with the same injected masks, repeatability under the seed, ``predict_road_map`` left as it was, the
validation step with and without ``hparams.mc_uncertainty``, and the ranking of a scene whose draws agree below one whose draws do not.
Models, batch and masks as tests/_head_mean_cases.py builds them (the smallest of the prediction tests, dropout ON); the oracle's
statistics and their bounds from tests/_head_uncert_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _head_mean_cases as hc  # noqa: E402
import _head_uncert_cases as cases  # noqa: E402
import _head_uncert_ref as ref  # noqa: E402

ALL = ("mean", "entropy", "mi", "var")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import mc, uncertainty
    mc.lib()
    uncertainty.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cpu_model():
    from driving_dirty_amd.roadmap import RoadMapBCE
    return hc.build(RoadMapBCE)


@pytest.fixture(scope="module")
def model(dev, cpu_model):
    from driving_dirty_amd.roadmap import RoadMapBCE
    m = hc.build(RoadMapBCE)
    m.load_state_dict(cpu_model.state_dict())
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def x(dev):
    return hc.views().to(dev)


def with_flags(model, **flags):
    class Flags:
        def __enter__(self):
            for k, v in flags.items():
                setattr(model.hparams, k, v)

        def __exit__(self, *exc):
            for k in flags:
                delattr(model.hparams, k)
    return Flags()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach().reshape(-1).view(torch.uint8), b.detach().reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("samples", hc.DRAWS)
def test_the_statistics_are_the_oracles_per_draw_passes(dev, model, cpu_model, x, samples):
    from driving_dirty_amd import mc, uncertainty
    from driving_dirty_amd.roadmap import eval_no_grad
    masks = hc.keeps(samples)
    want, bound = cases.model_reference(cpu_model, hc.views(), samples, masks)
    with eval_no_grad(model):
        pooled = model._pooled(x)
        got = uncertainty.predict(model, model.ae.encoder, pooled, samples, None, ALL, True, keeps=tuple(k.to(dev) for k in masks))
        mean = mc.head_mean_prob(model, model.ae.encoder, pooled, samples, None, keeps=tuple(k.to(dev) for k in masks))
    assert got._fields == ALL + ("scores",) and all(tuple(t.shape) == (hc.B, 800, 800) for t in got[:4]) and tuple(got.scores.shape) == (hc.B, 3)
    assert same_bits(got.mean, mean)
    used = {}
    for name in ALL + ("scores",):
        g = getattr(got, name).cpu().numpy().reshape(getattr(want, name).shape)
        used[name] = ref.fraction(g, getattr(want, name), getattr(bound, name))
    print(f"S = {samples}: largest fraction of the model bounds used: " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
          + f"; bounds up to mi {bound.mi.max():.3g}, var {bound.var.max():.3g}; mi score {want.scores[:, 1]}")
    assert all(v <= 1.0 for v in used.values()), used
    assert float(want.scores[:, 1].min()) > 10 * float(bound.scores[:, 1].max()), "the draws disagree by far more than the bound: zeros would not pass"


def test_a_call_is_a_function_of_weights_batch_and_seed(dev, model, x):
    state = torch.cuda.get_rng_state(dev)
    tau = hc.TAU
    before = model.predict_road_map(x, tau, mc_samples=8)
    one = model.predict_uncertainty(x, mc_samples=8, maps=ALL)
    assert torch.equal(torch.cuda.get_rng_state(dev), state), "torch's global generator is not touched"
    torch.cuda.manual_seed(999)      # ... and does not matter
    two = model.predict_uncertainty(x, mc_samples=8, maps=ALL)
    assert one._fields == ALL + ("scores",) and all(same_bits(a, b) for a, b in zip(one, two))
    after = model.predict_road_map(x, tau, mc_samples=8)
    assert torch.equal(before, after), "predict_road_map is what it was"
    assert torch.equal(one.mean > tau, before), "the draws are predict_road_map's draws, and `mean` its mean"
    default = model.predict_uncertainty(x, mc_samples=8)
    assert default._fields == ("mi", "scores") and same_bits(default.mi, one.mi) and same_bits(default.scores, one.scores)
    assert default.scores.dtype == torch.float64 and tuple(default.scores.shape) == (hc.B, 3) and tuple(default.mi.shape) == (hc.B, 800, 800)
    with with_flags(model, mc_samples=8):
        flagged = model.predict_uncertainty(x)
        assert same_bits(flagged.mi, one.mi)
        with with_flags(model, mc_seed=1):
            assert not same_bits(model.predict_uncertainty(x).mi, one.mi)
        with with_flags(model, tta_mirror=True):
            assert same_bits(model.predict_uncertainty(x).mi, one.mi), "tta_mirror is ignored"
    with pytest.raises(ValueError, match="mc_samples"):
        model.predict_uncertainty(x)
    with pytest.raises(ValueError, match="mc_samples"):
        model.predict_uncertainty(x, mc_samples=1)
    model.train()      # the method puts the module in eval mode itself and restores it
    model.ae.eval()
    try:
        assert same_bits(model.predict_uncertainty(x, mc_samples=8).mi, one.mi)
        assert model.training and model.fc1.training and not model.ae.training
    finally:
        model.eval()


def test_validation_under_the_flag(dev, monkeypatch):
    from driving_dirty_amd import mc, synth, uncertainty
    from driving_dirty_amd.roadmap import RoadMapBCE
    model = hc.build(RoadMapBCE).to(dev).eval()
    views, road = hc.views().to(dev), synth.road_maps(hc.B, seed=5).to(dev)
    batch = (tuple(views), None, tuple(road))
    calls = []
    real_mc, real_un = mc.launch, uncertainty.launch
    monkeypatch.setattr(mc, "launch", lambda name, *ops: (calls.append(name), real_mc(name, *ops))[1])
    monkeypatch.setattr(uncertainty, "launch", lambda name, *ops: (calls.append(name), real_un(name, *ops))[1])
    with with_flags(model, mc_samples=8, mc_seed=2):
        off = model.validation_step(batch, 0)
        assert calls == ["dd_head_mean_prob"], "without the flag: the parent's launches"
        with with_flags(model, mc_uncertainty=False):
            del calls[:]
            model.validation_step(batch, 0)
            assert calls == ["dd_head_mean_prob"]
        with with_flags(model, mc_uncertainty=True):
            del calls[:]
            on = model.validation_step(batch, 0)
            assert calls == ["dd_head_uncert"], "one pass of the head, not two"
            with torch.no_grad():
                want = model.predict_uncertainty(tuple(views), maps=()).scores.mean(0).float()
            with with_flags(model, tta_mirror=True):
                del calls[:]
                both = model.validation_step(batch, 0)
                assert calls == ["dd_head_uncert", "dd_head_uncert"]
            log = model.validation_epoch_end([on, on])["log"]
    assert set(on) == set(off) | set(uncertainty.VAL_KEYS) and set(uncertainty.VAL_KEYS) == {"val_mc_entropy", "val_mc_mi", "val_mc_var"}
    for k in ("val_ts_mc", "val_ts_rounded_mc"):      # the other keys come from the step's own single draw, torch's global generator
        assert same_bits(on[k], off[k]), k      # the mean's bits did not move
    for i, k in enumerate(uncertainty.VAL_KEYS):
        assert on[k].dtype == torch.float32 and on[k].dim() == 0 and same_bits(on[k], want[i]) and same_bits(log["avg_" + k], on[k]), k
        assert same_bits(both[k], on[k]), "under the mirror mode the scores are the unmirrored batch's"
    assert float(on["val_mc_mi"]) > 0 and float(on["val_mc_entropy"]) >= float(on["val_mc_mi"]) and float(on["val_mc_var"]) > 0
    assert same_bits(both["val_ts_mc"], off["val_ts_mc"]) and "val_ts_tta" in both
    with with_flags(model, mc_uncertainty=True):      # one draw: nothing to report, the parent's step
        del calls[:]
        assert set(model.validation_step(batch, 0)) == set(off) - {"val_ts_mc", "val_ts_rounded_mc"} and not calls


def test_disagreeing_draws_rank_above_agreeing_ones(dev, model):
    """Two scenes from the same frames (tests/_head_uncert_cases.ranking_inputs): the draws of scene 0 share one mask, those of scene 1
    have independent ones.  Scene 0's mutual-information score lies within the TIGHT bound of 0 -- its draws are the same logits bit for
    bit -- and scene 1's is larger; tests/test_head_uncert_ref.py shows on the CPU that the gap is more than twice any bound."""
    from driving_dirty_amd import ops, uncertainty
    from driving_dirty_amd.roadmap import eval_no_grad
    samples = cases.RANK_DRAWS
    xs, masks = cases.ranking_inputs()
    keeps = tuple(k.to(dev) for k in masks)
    with eval_no_grad(model):
        pooled = model._pooled(xs.to(dev))
        got = uncertainty.predict(model, model.ae.encoder, pooled, samples, None, ("mi", "var"), True, keeps=keeps)
        z = model.ae.encoder.latent_samples(pooled, samples, keeps, None)
        logits = ops.linear(z, model.fc1.weight, model.fc1.bias)
    assert all(torch.equal(logits[0], logits[s]) for s in range(1, samples)), "scene 0: one prediction, S times"
    _, tight = ref.stats_from_logits(logits[:samples].cpu().numpy(), samples)
    same, free = float(got.scores[0, 1]), float(got.scores[1, 1])
    print(f"mutual-information score: shared mask {same:.3g} (bound {float(tight.scores[0, 1]):.3g}), independent masks {free:.3g}")
    assert 0 <= same <= float(tight.scores[0, 1]) and free > same
    assert float(got.scores[0, 2]) <= float(tight.scores[0, 2]) and float(got.scores[1, 2]) > float(got.scores[0, 2])
    assert float(got.mi[1].double().mean()) == pytest.approx(free, rel=1e-12) and bool((got.mi[0] <= torch.from_numpy(tight.mi[0]).to(dev).reshape(800, 800)).all())
    assert np.all(np.isfinite(got.scores.cpu().numpy()))


def test_the_ranking_tool_writes_the_same_ranked_scores_twice(dev, cpu_model, tmp_path, monkeypatch):
    """tools/rank_uncertainty.py in this process on a checkpoint of the small model: scores.json ranks the scenes by their
    mutual-information score, which is ``predict_uncertainty``'s, the maps are written with ``--maps``, and a second run writes the same."""
    import json
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import rank_uncertainty as tool
    finally:
        sys.path.pop(0)
    from driving_dirty_amd import synth
    ckpt = str(tmp_path / "rm.ckpt")
    cpu_model.save_checkpoint(ckpt)
    outs = []
    for name in ("a", "b"):
        out = str(tmp_path / name)
        monkeypatch.setattr(sys, "argv", ["rank_uncertainty.py", "--rm_ckpt_path", ckpt, "--out", out, "--scenes", "4", "--batch_size", "3",
                                          "--mc_samples", "4", "--mc_seed", "7", "--maps"])
        tool.main()
        outs.append(out)
    first = json.load(open(os.path.join(outs[0], "scores.json")))
    assert first == json.load(open(os.path.join(outs[1], "scores.json"))) and first["mc_samples"] == 4 and first["mc_seed"] == 7
    rows = first["scenes"]
    assert sorted(r["scene"] for r in rows) == [0, 1, 2, 3] and [r["mi"] for r in rows] == sorted((r["mi"] for r in rows), reverse=True)
    assert all(set(r) == {"scene", "entropy", "mi", "var"} and r["entropy"] >= r["mi"] > 0 and r["var"] > 0 for r in rows)
    from driving_dirty_amd.roadmap import RoadMapBCE
    model = RoadMapBCE.load_from_checkpoint(ckpt).to(dev).eval()
    model.hparams.mc_seed = 7
    x = synth.camera_batch(4, hc.H, hc.W, seed=1).to(dev)
    want = model.predict_uncertainty(x[:3].contiguous(), mc_samples=4)
    by_scene = {r["scene"]: r for r in rows}
    for i in range(3):
        assert by_scene[i]["mi"] == float(want.scores[i, 1])
        assert np.array_equal(np.load(os.path.join(outs[0], f"mi_{i:05d}.npy")), want.mi[i].cpu().numpy())
        assert np.array_equal(np.load(os.path.join(outs[0], f"mi_{i:05d}.npy")), np.load(os.path.join(outs[1], f"mi_{i:05d}.npy")))
    assert os.path.exists(os.path.join(outs[0], "mi_00003.npy")) and not os.path.exists(os.path.join(outs[0], "mi_00004.npy"))
