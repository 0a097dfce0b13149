"""GPU tests of ``hparams.box_rm_input``: the joint training step whose box head reads the road-map head's own map."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _joint_cases as jc  # noqa: E402

B = 2
TAU = 0.3
BOX_HEAD = ("space_map_cnn.", "box_merge.")
ROAD_HEAD = ("fc1.", "ae.encoder.fc1.", "ae.encoder.fc2.", "ae.encoder.fc_z_out.")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def batch(dev):
    from driving_dirty_amd import synth
    views, road = jc.views_and_roads(dev, B)
    targets = tuple({"bounding_box": synth.car_boxes(n, seed=3 + n)} for n in (12, 5))
    return tuple(views), targets, tuple(road)


def step(model, batch):
    """One training step in train mode -> (log with detached values, gradients by name); the model's gradients are cleared and BatchNorm's
    running statistics put back, so that every step of a test starts from the same model."""
    model.train()
    stats = {k: v.clone() for k, v in model.named_buffers()}
    out = model.training_step(batch, 0)
    out["loss"].backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        for k, v in model.named_buffers():
            v.copy_(stats[k])
    return {k: v.detach().clone() for k, v in out["log"].items()}, jc.grads_of(model)


def worst(a, b, prefixes):
    """Largest absolute difference between two gradient dicts over the parameters under ``prefixes`` (each must have a gradient)."""
    names = [k for k in a if k.startswith(prefixes)]
    assert names and all(a[k] is not None and b[k] is not None for k in names)
    return max(float((a[k] - b[k]).abs().max()) for k in names)


def test_target_is_the_step_without_the_flag(dev, batch):
    plain, flagged = jc.build_joint(dev), jc.build_joint(dev, box_rm_input="target")
    assert not hasattr(plain.hparams, "box_rm_input")
    log_a, g_a = step(plain, batch)
    log_b, g_b = step(flagged, batch)
    assert set(log_a) == set(log_b) == {"train_loss", "roadmap_loss", "bbox_loss"}
    for k in log_a:
        assert torch.equal(log_a[k], log_b[k]), k
    assert set(g_a) == set(g_b)
    for k in g_a:
        assert g_a[k] is not None and torch.equal(g_a[k], g_b[k]), k


def test_predicted_feeds_the_heads_own_map(dev, batch):
    """Bounds.  The box head's gradients are compared against a default model stepped on the batch with the road masks swapped for the
    head's own; that swapped step is run twice first, and likewise the road-map-only backward: where the two runs agree bit for bit
    the comparison demands bit equality, otherwise twice their largest difference.  Measured on an MI355X: both pairs of runs agree
    bit for bit (difference 0.0), so every comparison below is an equality."""
    from driving_dirty_amd import ops
    sample, targets, road = batch
    default = jc.build_joint(dev)
    own = jc.build_joint(dev, box_rm_input="predicted", rm_threshold=TAU)
    assert own.rm_threshold == TAU

    log_own, g_own = step(own, batch)
    log_def, g_def = step(default, batch)
    # the road-map loss still reads the ground truth
    assert torch.equal(log_own["roadmap_loss"], log_def["roadmap_loss"])

    # the map the box branch was fed: sigmoid(train-mode logits) > tau of the same forward
    default.train()
    stats = {k: v.clone() for k, v in default.named_buffers()}
    with torch.no_grad():
        logits, _ = default(sample, road)
        masks = tuple(ops.sigmoid(logits) > TAU)
        for k, v in default.named_buffers():
            v.copy_(stats[k])
    share, share_half = float(torch.stack(masks).float().mean()), float((ops.sigmoid(logits) > 0.5).float().mean())
    print(f"own road map: share {share:.3f} at {TAU}, {share_half:.3f} at 0.5; the batch's {float(torch.stack(road).float().mean()):.3f}")
    assert 0.05 < share < 0.95 and abs(share - share_half) > 0.01      # tau is the calibrated one, not 0.5
    assert not torch.equal(torch.stack(masks), torch.stack(road))
    assert not torch.equal(log_own["bbox_loss"], log_def["bbox_loss"])      # the flag does something

    swapped = (sample, targets, masks)
    log_1, g_1 = step(default, swapped)
    log_2, g_2 = step(default, swapped)
    spread_loss = abs(float(log_1["bbox_loss"]) - float(log_2["bbox_loss"]))
    spread = worst(g_1, g_2, BOX_HEAD)
    err_loss = abs(float(log_own["bbox_loss"]) - float(log_1["bbox_loss"]))
    err = worst(g_own, g_1, BOX_HEAD)
    print(f"box head: swapped step run to run: loss {spread_loss:.3e}, gradients {spread:.3e}; self-fed against it: loss {err_loss:.3e}, gradients {err:.3e}")
    assert err_loss <= 2 * spread_loss and err <= 2 * spread
    if spread == 0 and spread_loss == 0:
        assert torch.equal(log_own["bbox_loss"], log_1["bbox_loss"])
        assert all(torch.equal(g_own[k], g_1[k]) for k in g_own if k.startswith(BOX_HEAD))

    # no gradient of the box loss reaches the road-map head through the map: fc1 and the encoder's tail get the road-map loss's alone
    def road_only():
        default.train()
        stats = {k: v.clone() for k, v in default.named_buffers()}
        params = [(k, p) for k, p in default.named_parameters() if k.startswith(ROAD_HEAD)]
        loss = default.training_step(batch, 0)["log"]["roadmap_loss"]
        grads = torch.autograd.grad(loss, [p for _, p in params])
        with torch.no_grad():
            for k, v in default.named_buffers():
                v.copy_(stats[k])
        return {k: g.detach().clone() for (k, _), g in zip(params, grads)}

    r_1, r_2 = road_only(), road_only()
    assert set(r_1) == {k for k in g_own if k.startswith(ROAD_HEAD)} and "fc1.weight" in r_1 and "ae.encoder.fc1.fc1.weight" in r_1
    spread_r, err_r = worst(r_1, r_2, ROAD_HEAD), worst(g_own, r_1, ROAD_HEAD)
    print(f"road-map head and tail: road-map-only backward run to run {spread_r:.3e}; self-fed step against it {err_r:.3e}")
    assert err_r <= 2 * spread_r
    if spread_r == 0:
        assert all(torch.equal(g_own[k], r_1[k]) for k in r_1)
    # ... while in the default step they are the same too (the box branch never touched them), and the shared conv stack gets both losses
    assert all(torch.equal(g_def[k], r_1[k]) for k in r_1) or spread_r > 0
    assert all(g_own[k] is not None and bool(torch.isfinite(g_own[k]).all()) for k in g_own)
    assert not torch.equal(g_own["ae.encoder.c1.weight"], g_def["ae.encoder.c1.weight"])
