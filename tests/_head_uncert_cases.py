"""The case grid of the uncertainty kernel's tests, shared by the CPU test that checks the reference and its bounds alone
(test_head_uncert_ref.py) and the GPU tests (test_gpu_head_uncert.py): the same shapes, the same operands.

The shapes are the smallest that reach every branch, by the reasoning of tests/test_gpu_head_mean.py.  (scenes, S): draw groups that
sit in one accumulator lane (2, 4) and that do not (3, 5, 33); rows up to 32 (the one-tile kernel) and past it (the two-tile one);
several launches, the last one smaller ((5,16) = 4 + 1 scenes, (2,33) = 1 + 1, (33,2) = 32 + 1; (7,8) = 7 of 8; (13,5) = 12 + 1); more
than 8 scenes in a launch, so that a gathering lane owns several ((9,2), (33,2), (13,5)); S = 1 and S = 64.  n: below one 128-column
block (16, 100), across it (130, 272: two and three blocks' partials), n % 16 != 0 (100), n % 4 != 0 (130: the element-wise stores and
a ragged last block in the column sums).  k: one chunk of 4, one k-tile and a bit, the 8 tiles past which ``dd_linear_fwd`` splits.
The operands are those of tests/test_gpu_head_mean.py; ``WIDE`` is the spread at which the logits of every group reach +-30, so that
both tails carry real values."""
import numpy as np

from test_gpu_head_mean import operands as _operands

GROUPS = ((3, 1), (9, 2), (3, 3), (5, 4), (13, 5), (7, 8), (5, 16), (2, 33), (1, 64), (33, 2))      # (scenes, S)
N_SIZES = (16, 100, 130, 272)
K_SIZES = (4, 68, 512)
NARROW, WIDE = 3.0, 36.0
SPREADS = (NARROW, WIDE)


def operands(dev, scenes, samples, n, k, bias=True, spread=NARROW):
    return _operands(dev, scenes, samples, n, k, bias, spread)


def shapes():
    """(n, k, bias, spread) over the whole product."""
    return [(n, k, bias, spread) for k in K_SIZES for n in N_SIZES for bias in (True, False) for spread in SPREADS]


def logits32_cpu(x, w, b):
    """fp32 logits of CPU operands: the fp64 product rounded once (the GPU tests take the product's own from ``ops.linear``)."""
    z = x.double() @ w.double().t()
    if b is not None:
        z = z + b.double()
    return z.float().numpy()


def numpy_operands(x, w, b):
    return x.detach().cpu().numpy(), w.detach().cpu().numpy(), None if b is None else b.detach().cpu().numpy()


def identical_draws(z32, samples):
    """The logits with every draw of a scene replaced by its first."""
    z = np.asarray(z32).reshape(-1, samples, z32.shape[1])
    return np.repeat(z[:, :1], samples, axis=1).reshape(z32.shape).copy()



# ---- the models' cases: tests/_head_mean_cases.py's model, batch and masks, with the fp64 oracle extended to the statistics --------------
RANK_DRAWS = 5


def model_logits64(model, x, samples, masks):
    """fp64 logits [B * S, 640000], scene-major, of ``model`` (on the CPU): the oracle's encoder and head with the model's weights, in
    eval mode, one pass per draw with that draw's masks (``_head_mean_cases.reference64``'s loop, kept at the logits)."""
    import torch

    import _head_mean_cases as hc
    from oracle import ae_parts, steps
    enc = ae_parts.EncoderNet(hc.HIDDEN, hc.LATENT, 3, hc.H, 6 * hc.W)
    enc.load_state_dict(model.ae.encoder.state_dict())
    head = torch.nn.Linear(hc.LATENT, 640000)
    head.load_state_dict(model.fc1.state_dict())
    enc, head = enc.double().eval(), head.double()
    b = x.shape[0]
    with torch.no_grad():
        draws = [steps.roadmap_forward(enc, head, x.double(), tuple(k.double().reshape(b, samples, -1)[:, s].contiguous() for k in masks))[0]
                 for s in range(samples)]
    return torch.stack([d.reshape(b, -1) for d in draws], dim=1).reshape(b * samples, -1).numpy()


def model_reference(model, x, samples, masks):
    """(Stats in fp64, Stats of bounds) of the model's statistics: the oracle's logits, which a model may miss by ``MODEL_BOUND`` of
    their peak, through ``_head_uncert_ref.stats_of_logits64``."""
    import _head_mean_cases as hc
    import _head_uncert_ref as ref
    z = model_logits64(model, x, samples, masks)
    return ref.stats_of_logits64(z, samples, hc.MODEL_BOUND * float(np.abs(z).max()))


def ranking_inputs(samples=RANK_DRAWS, seed=9):
    """Two scenes from the SAME frames and their keep masks [2 * S, hidden] x 2: scene 0 draws one mask and repeats it in every draw (its
    draws are one prediction: no model uncertainty), scene 1 draws ``samples`` independent masks."""
    import torch

    import _head_mean_cases as hc
    x = hc.views()[:1].repeat(2, 1, 1, 1, 1).contiguous()
    g = torch.Generator().manual_seed(seed)
    masks = []
    for _ in range(2):
        one = torch.empty((1, hc.HIDDEN)).bernoulli_(0.8, generator=g).repeat(samples, 1)
        masks.append(torch.cat([one, torch.empty((samples, hc.HIDDEN)).bernoulli_(0.8, generator=g)]))
    return x, tuple(masks)
