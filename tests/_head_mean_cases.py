"""Models, batches, injected masks and the fp64 reference of the sampled-prediction tests, shared by the CPU test that checks the
reference alone (test_head_mean_surface.py) and the GPU tests that use it (test_gpu_head_mean_models.py).  The smallest model the
prediction tests build (test_gpu_predict.py): 16 x 22 views, hidden 16, latent 8 -- with the dropout ON at the reference's p = 0.2,
which is what this feature is about.  Closed-form inputs and weights (driving_dirty_amd/synth.py): the same numbers on any machine."""
from argparse import Namespace

import torch

from driving_dirty_amd import synth

H, W = 16, 22
B = 3
HIDDEN, LATENT = 16, 8
HEAD_GAIN = 4.0      # as tests/_joint_cases.py: spreads the filled head's probabilities past 0.3 .. 0.7
TAU = 0.47
DRAWS = (5, 16)      # 15 rows: the fused tail, one row tile; 48 rows: past the fused tail's 32, two row tiles
KERNEL_BOUND, MODEL_BOUND = 2e-5, 2e-4      # of the peak: the project's bounds for one kernel and for a model against fp64
HP = dict(unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=10 ** 9)


def build(cls, seed=77, **extra):
    """On the CPU, dropout as constructed (p = 0.2); move it with ``.to(dev)``."""
    from driving_dirty_amd.autoencoder import BasicAE
    ae = BasicAE(Namespace(hidden_dim=HIDDEN, latent_dim=LATENT, input_height=H, input_width=6 * W))
    model = cls(Namespace(pretrained_ae=ae, **HP, **extra))
    synth.fill_module(model, seed=seed)
    with torch.no_grad():
        model.fc1.weight.mul_(HEAD_GAIN)
        model.fc1.bias.mul_(HEAD_GAIN)
    return model


def views(seed=5):
    return synth.camera_batch(B, H, W, seed=seed)


def keeps(samples, seed=3):
    """Two keep masks [B * samples, hidden] of 0 / 1 at the reference's keep rate 0.8, scene-major."""
    g = torch.Generator().manual_seed(seed + 1000 * samples)
    return tuple(torch.empty((B * samples, HIDDEN)).bernoulli_(0.8, generator=g) for _ in range(2))


def draw(masks, samples, s):
    """The masks of draw ``s`` of every scene: [B, hidden] each."""
    return tuple(k.reshape(B, samples, HIDDEN)[:, s].contiguous() for k in masks)


def reference64(model, x, samples, masks):
    """fp64 mean over the draws of the probabilities of ``model`` (on the CPU) -> [B,800,800]: the oracle's encoder and head with the
    model's weights, in eval mode, one pass per draw with that draw's masks."""
    from oracle import ae_parts, steps
    enc = ae_parts.EncoderNet(HIDDEN, LATENT, 3, H, 6 * W)
    enc.load_state_dict(model.ae.encoder.state_dict())
    head = torch.nn.Linear(LATENT, 640000)
    head.load_state_dict(model.fc1.state_dict())
    enc, head = enc.double().eval(), head.double()
    with torch.no_grad():
        probs = [steps.roadmap_forward(enc, head, x.double(), tuple(k.double() for k in draw(masks, samples, s)))[1] for s in range(samples)]
    return torch.stack(probs).mean(0)


def band(mean64, tau=TAU, bound=MODEL_BOUND):
    """Elements whose fp64 mean lies within the model bound of ``tau``: there, and only there, an fp32 model may land on the other side."""
    return (mean64 - tau).abs() <= bound * float(mean64.abs().max())
