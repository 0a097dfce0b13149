"""Models and batches of the joint model's GPU tests (test_gpu_joint_*.py): the reference's 256 x 306 views (the heads fix that size),
everything else as small as it goes -- hidden 16, latent 8, B = 2 (train-mode BatchNorm needs more than one row) or an odd B = 3 in
the collate's per-sample form.  Closed-form inputs and weights (driving_dirty_amd/synth.py): the same numbers on any machine."""
import math
from argparse import Namespace

import torch

from driving_dirty_amd import synth

HP = dict(learning_rate=1e-3, output_img_freq=500)
HEAD_GAIN = 4.0      # the filled road-map head's probabilities lie in about 0.39 .. 0.61; four times the logits spreads them past 0.3


def build_joint(dev, seed=29, dropout=False, **extra):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.joint import JointRoadMapBBox
    model = JointRoadMapBBox(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=16, latent_dim=8)), **HP, **extra))
    synth.fill_module(model, seed=seed)
    with torch.no_grad():
        model.fc1.weight.mul_(HEAD_GAIN)
        model.fc1.bias.mul_(HEAD_GAIN)
    if not dropout:      # the reference's dropout is on in eval mode too (components.py:108)
        model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0
    return model.to(dev)


def centre_box_map(model, x, rm):
    """An untrained box head's map lies on one side of 0.5, where validation decodes it: move the last layer's bias so that the
    median of the map computed with ``rm`` is 0.5.  The decoding is what the tests are about, not the head's training."""
    with torch.no_grad():
        m = float(model(x, rm)[1].median())
        assert 0.0 < m < 1.0
        model.box_merge.up_conv_5.bias -= math.log(m / (1.0 - m))


def views_and_roads(dev, b, seed=17):
    return synth.camera_batch(b, seed=seed).to(dev), synth.road_maps(b, seed=seed).to(dev)


def input_forms(views):
    """The three forms ``forward`` takes, from fp32 views [B,6,3,H,W] on the device."""
    frames = (views * 255).round().to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous()
    return {"stacked": views, "tuple": tuple(views), "uint8": tuple(frames)}


def flags(model):
    return [m.training for m in model.modules()]


def grads_of(model):
    """{name: gradient clone or None}, and the gradients cleared."""
    out = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    return out
