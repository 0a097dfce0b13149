"""GPU tests of the road-map prediction path: the threat-score histogram (dd_ts_hist), the head as a boolean map
(dd_linear_sigmoid_gt), ``predict_road_map`` and the threshold calibration of the road-map modules."""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _predict_cases as pc  # noqa: E402
from _ts_curve_ref import ts_curve_ref, ts_hist_ref  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ dd_ts_hist
def _hist_inputs(n, bins, seed):
    """Random probabilities with the edge values in front (as many as fit): exact 0 and 1, a NaN, every k / bins, the fp32
    neighbours on both sides of several k / bins, values outside [0, 1]."""
    rs = np.random.RandomState(seed)
    prob = rs.random_sample(n).astype(np.float32)
    grid = np.arange(bins + 1, dtype=np.float32) / np.float32(bins)
    some = grid[np.unique(np.clip([0, 1, bins // 4, bins // 2, bins - 1, bins], 0, bins))]
    special = np.concatenate([np.float32([0.0, 1.0, np.nan, 0.5]), np.nextafter(some, np.float32(2)), np.nextafter(some, np.float32(-1)),
                              grid, np.float32([-0.25, 1.5, np.inf, 1e-45])]).astype(np.float32)
    m = min(n, special.size)
    prob[:m] = special[:m]
    target = rs.random_sample(n) < 0.3
    return prob, target


def _targets(target, kind, rs):
    if kind == "bool":
        return torch.from_numpy(target)
    if kind == "uint8":      # any non-zero byte is a positive
        return torch.from_numpy(np.where(target, rs.randint(1, 256, target.size), 0).astype(np.uint8))
    return torch.from_numpy(np.where(target, rs.choice(np.float32([1.0, 0.5, -2.0]), target.size), np.float32(-0.0)).astype(np.float32))


@pytest.mark.parametrize("bins", [2, 256, 1024])
@pytest.mark.parametrize("n", [4, 252, 256 * 1024 + 4, 2 * 800 * 800])
def test_ts_hist_equals_the_numpy_reference(dev, n, bins):
    from driving_dirty_amd import ops
    prob, target = _hist_inputs(n, bins, seed=n + bins)
    want = ts_hist_ref(prob, target, bins)
    assert want.sum() == n and (n < 3 or np.isnan(prob).sum() == 1)
    p = torch.from_numpy(prob).to(dev)
    rs = np.random.RandomState(7)
    for kind in ("bool", "uint8", "fp32"):
        got = ops.ts_histogram(p, _targets(target, kind, rs).to(dev), bins)
        assert got.dtype == torch.int64 and tuple(got.shape) == (2, bins + 1)
        assert np.array_equal(got.cpu().numpy(), want), kind
    again = ops.ts_histogram(p, torch.from_numpy(target).to(dev), bins)
    assert torch.equal(again, got)      # run to run: the same bits


def test_ts_hist_accumulates_and_refuses(dev):
    from driving_dirty_amd import _lib, ops
    bins, n = 256, 40000
    prob, target = _hist_inputs(n, bins, seed=5)
    p, t = torch.from_numpy(prob).to(dev), torch.from_numpy(target).to(dev)
    cut = 12000
    acc = ops.ts_histogram(p[:cut], t[:cut], bins)
    same = ops.ts_histogram(p[cut:], t[cut:], bins, out=acc)
    assert same is acc
    assert np.array_equal(acc.cpu().numpy(), ts_hist_ref(prob[:cut], target[:cut], bins) + ts_hist_ref(prob[cut:], target[cut:], bins))
    assert np.array_equal(acc.cpu().numpy(), ts_hist_ref(prob, target, bins))
    # unsupported bins / n: refused, nothing written
    before = acc.clone()
    for bad_bins in (3, 2048):
        buf = torch.full((2, bad_bins + 1), 9, device=dev, dtype=torch.int64)
        with pytest.raises(_lib.HotpathError):
            ops.ts_histogram(p, t, bad_bins, out=buf)
        assert bool((buf == 9).all())
    with pytest.raises(_lib.HotpathError):
        ops.ts_histogram(p[:6], t[:6], bins, out=acc)
    lib = _lib.lib()
    assert lib.dd_ts_hist(ops._p(p), ops._p(t), 7, n, bins, ops._p(acc), None) != 0      # unknown target dtype
    torch.cuda.synchronize()
    assert torch.equal(acc, before)


def test_ts_hist_agrees_with_the_threat_score_kernel(dev):
    from driving_dirty_amd import ops
    rs = np.random.RandomState(11)
    n = 2 * 800 * 800
    p = torch.from_numpy(rs.random_sample(n).astype(np.float32)).to(dev)
    t = torch.from_numpy((rs.random_sample(n) < 0.3).astype(np.float32)).to(dev)
    for bins in (2, 256):
        ts, _ = ops.ts_curve(ops.ts_histogram(p, t, bins))
        want = float(ops.threat_score(t, p, round_b=True))
        assert abs(float(ts[bins // 2]) - want) <= 1e-6 * want


# ------------------------------------------------------------------------------------------------ dd_linear_sigmoid_gt
GUARD = 256      # bytes on either side of the output (a multiple of 16: the output keeps the alignment the vector stores need)


def _fused_guarded(x, w, b, tau):
    """The kernel straight through the C ABI into a buffer with guard bytes around it."""
    from driving_dirty_amd import _lib, ops
    m, n = x.shape[0], w.shape[0]
    buf = torch.full((GUARD + m * n + GUARD,), 0xA5, device=x.device, dtype=torch.uint8)
    out = buf[GUARD:GUARD + m * n]
    _lib.check(_lib.lib().dd_linear_sigmoid_gt(ops._p(x), ops._p(w), ops._p(b), tau, ops._p(out), m, n, x.shape[1], ops._stream()), "dd_linear_sigmoid_gt")
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + m * n:] == 0xA5).all()), "guard bytes overwritten"
    assert bool((out <= 1).all())
    return out.reshape(m, n).bool()


@pytest.mark.parametrize("m,n,k", pc.CASES)
def test_linear_sigmoid_gt(dev, m, n, k):
    from driving_dirty_amd import ops
    xh, wh, bh = pc.head_inputs(m, n, k)
    x, w, b = (torch.from_numpy(a).to(dev) for a in (xh, wh, bh))
    # ops.linear wants N % 4 == 0: the unfused reference runs on the weight padded with zero rows, a column's sum does not depend on N
    pad = (-n) % 4
    wp, bp = torch.cat([w, w.new_zeros(pad, k)]).contiguous(), torch.cat([b, b.new_zeros(pad)]).contiguous()
    plain64 = x.double() @ w.double().t()
    for bias, bias_p in ((None, None), (b, bp)):
        logit64 = plain64 if bias is None else plain64 + bias.double()
        probs = ops.sigmoid(ops.linear(x, wp, bias_p))[:, :n]
        for tau in pc.TAUS:
            got = _fused_guarded(x, w, bias, tau)
            assert torch.equal(got, ops.linear_sigmoid_gt(x, w, bias, tau))
            # 1. fp64, outside the band around the threshold's logit; the band is narrow (tests/test_ts_curve_ref.py shows it from the inputs)
            band = pc.band_mask(logit64, tau)
            share = float(band.double().mean())
            wrong = (got != (torch.sigmoid(logit64) > tau)) & ~band
            print(f"m={m} n={n} k={k} bias={bias is not None} tau={tau}: band share {share:.2e}, mismatches outside {int(wrong.sum())}, "
                  f"differs from unfused {int((got != (probs > tau)).sum())}")
            assert share <= pc.BAND_CAP
            assert not bool(wrong.any())
            # 2. the unfused path, bit for bit
            assert torch.equal(got, probs > tau)


def test_linear_sigmoid_gt_refuses_what_linear_fwd_would_split(dev):
    from driving_dirty_amd import _lib, ops
    x, w = torch.zeros(2, 1024, device=dev), torch.zeros(64, 1024, device=dev)
    with pytest.raises(_lib.HotpathError):
        ops.linear_sigmoid_gt(x, w, None, 0.5)
    with pytest.raises(_lib.HotpathError):
        ops.linear_sigmoid_gt(x[:, :6].contiguous(), w[:, :6].contiguous(), None, 0.5)


# ------------------------------------------------------------------------------------------------ the modules
H, W = 16, 22      # the smallest encoder input of the head tests


def _model(cls, dev, precision, seed=77, **extra):
    from driving_dirty_amd import synth
    from driving_dirty_amd.autoencoder import BasicAE
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=H, input_width=6 * W))
    model = cls(Namespace(pretrained_ae=ae, precision=precision, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=10 ** 9, **extra))
    synth.fill_module(model, seed=seed)
    model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0      # the reference's dropout is on in eval mode too (components.py:108)
    return model.to(dev)


def _probs(model, x):
    out = model(x)
    return (out[1] if isinstance(out, tuple) else out).detach()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["RoadMapBCE", "RoadMap"])
def test_predict_road_map_is_forward_thresholded(dev, name, precision):
    from driving_dirty_amd import roadmap, synth
    model = _model(getattr(roadmap, name), dev, precision)
    views = synth.camera_batch(2, H, W, seed=5)
    frames = (views * 255).round().to(torch.uint8)
    samples = {"fp32 views": views.to(dev), "the collate's tuple": tuple(views.to(dev)),
               "uint8 frames": tuple(frames.permute(0, 1, 3, 4, 2).contiguous().to(dev))}
    for what, x in samples.items():
        model.eval()
        probs = _probs(model, x)
        assert 0.05 < float((probs > 0.5).float().mean()) < 0.95      # both classes present
        model.train()
        model.ae.eval()                     # a frozen extractor inside a training model
        for tau in (0.5, 0.45):      # this head's probabilities lie in 0.39 .. 0.61
            got = model.predict_road_map(x, tau)
            assert got.dtype == torch.bool and tuple(got.shape) == (2, 800, 800)
            assert torch.equal(got, probs > tau), (what, tau)
        assert model.training and model.fc1.training and not model.ae.training and not model.ae.encoder.fc1.fc_bn.training
        assert all(p.grad is None for p in model.parameters())
    assert torch.equal(model.predict_road_map(x), model.predict_road_map(x, 0.5))      # not calibrated: the reference's 0.5
    model.rm_threshold = 0.45
    assert torch.equal(model.predict_road_map(x), model.predict_road_map(x, 0.45)) and not torch.equal(model.predict_road_map(x), probs > 0.5)


def test_joint_model_predicts_through_its_roadmap_branch(dev):
    from driving_dirty_amd import ops, synth
    from driving_dirty_amd.joint import JointRoadMapBBox
    model = _model(JointRoadMapBBox, dev, None)
    views = synth.camera_batch(2, H, W, seed=6).to(dev)
    model.eval()
    with torch.no_grad():
        z = model.ae.encoder.forward_nhwc4(ops.wide_image(views))
        probs = ops.sigmoid(ops.linear(z, model.fc1.weight, model.fc1.bias)).reshape(2, 800, 800)
    model.train()
    assert torch.equal(model.predict_road_map(tuple(views), 0.47), probs > 0.47) and 0.05 < float((probs > 0.47).float().mean()) < 0.95
    assert model.training and all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("name", ["RoadMapBCE", "RoadMap"])
def test_calibration_round_trip(dev, name, tmp_path):
    from driving_dirty_amd import roadmap, synth
    cls = getattr(roadmap, name)
    model = _model(cls, dev, "fp32", calibrate_threshold=True)
    plain = _model(cls, dev, "fp32")
    model.eval(), plain.eval()
    keys = list(model.state_dict().keys())
    outs, probs, masks = [], [], []
    for i in range(2):
        views, road = synth.camera_batch(2, H, W, seed=20 + i).to(dev), synth.road_maps(2, seed=20 + i).to(dev)
        batch = (tuple(views), None, tuple(road))
        outs.append(model.validation_step(batch, i))
        off = plain.validation_step(batch, i)
        assert set(off) == {"val_loss", "val_ts_rounded", "val_ts"} and set(outs[-1]) == set(off) | {"ts_hist"}
        assert all(torch.equal(off[k], outs[-1][k]) for k in off)
        probs.append(_probs(model, tuple(views)).cpu().numpy())
        masks.append(road.cpu().numpy())
    end_off = plain.validation_epoch_end([{k: v for k, v in o.items() if k != "ts_hist"} for o in outs])
    assert set(end_off) == {"val_loss", "log"} and set(end_off["log"]) == {"avg_val_loss", "avg_val_ts_rounded", "avg_val_ts"}
    assert plain.rm_threshold is None and model.rm_threshold is None
    end = model.validation_epoch_end(outs)
    ts, best = ts_curve_ref(ts_hist_ref(np.concatenate(probs), np.concatenate(masks), 256))
    assert type(model.rm_threshold) is float and model.rm_threshold == best / 256
    log = end["log"]
    assert set(log) == set(end_off["log"]) | {"best_threshold", "best_val_ts", "val_ts_at_half"}
    assert log["best_threshold"] == best / 256 and log["best_val_ts"] == ts[best] and log["val_ts_at_half"] == ts[128]
    assert list(model.state_dict().keys()) == keys
    path = os.path.join(tmp_path, "rm.ckpt")
    model.save_checkpoint(path)
    loaded = cls.load_from_checkpoint(path)
    assert loaded.rm_threshold == model.rm_threshold and list(loaded.state_dict().keys()) == keys
    # a checkpoint from before the calibration existed: 0.5
    ckpt = torch.load(path, weights_only=False)
    del ckpt["hparams"]["rm_threshold"]
    torch.save(ckpt, path)
    assert cls.load_from_checkpoint(path).rm_threshold is None
