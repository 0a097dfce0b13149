"""Reference of include/dd_head_mean.h's semantics, for the CPU and the GPU tests of the sampled road-map head.

``mean_prob64``: the mean over a scene's S draws of ``sigmoid(x W^T + b)`` in fp64 -- what the kernels approximate.
``mean_in_draw_order``: the PINNED fp32 order restated with torch's fp32 arithmetic (IEEE adds and one multiply, on the CPU or the
device alike): ``sum = p[b,0]; sum += p[b,1]; ...; mean = sum * float32(1 / S)``.  Given the probabilities ``p`` a kernel's single draws
have, the kernel's mean equals this bit for bit.
``gt``: ``mean > tau`` with ``tau`` rounded to fp32, strictly; a NaN mean is False."""
import numpy as np
import torch


KERNEL_BOUND = 2e-5      # the project's kernel bound: a GEMM's fp32 result within 2e-5 of the peak of its fp64 reference


def prob_bound(peak_logit, samples):
    """How far an fp32 mean probability may lie from the fp64 one: the logit's kernel bound through the sigmoid's slope (at most 1/4),
    the sigmoid's own 3 x 2^-24 absolute (csrc/dd_device.h), and S - 1 adds and one multiply of partial sums that stay below S, each
    within half an ulp: S x 2^-24 of the mean."""
    return 0.25 * KERNEL_BOUND * peak_logit + 3 * 2.0 ** -24 + samples * 2.0 ** -24


def mean_prob64(x, w, bias, samples, with_bound=False):
    """x [scenes * samples, k] (scene-major), w [n, k], bias [n] or None -> fp64 [scenes, n]; ``with_bound``: also ``prob_bound`` of these
    logits."""
    x, w = x.detach().double().cpu(), w.detach().double().cpu()
    z = x @ w.t()
    if bias is not None:
        z = z + bias.detach().double().cpu()
    mean = torch.sigmoid(z).reshape(-1, samples, w.shape[0]).mean(1)
    return (mean, prob_bound(float(z.abs().max()), samples)) if with_bound else mean


def inv_samples(samples):
    """``(float)(1.0 / S)`` of the header: the fp32 nearest the fp64 quotient."""
    return float(np.float32(1.0 / samples))


def mean_in_draw_order(p, samples):
    """fp32 p [scenes * samples, n], row b * samples + s draw s of scene b -> fp32 [scenes, n] in the pinned order."""
    assert p.dtype == torch.float32 and p.shape[0] % samples == 0
    p = p.reshape(-1, samples, p.shape[1])
    total = p[:, 0].clone()
    for s in range(1, samples):
        total = total + p[:, s]
    return total * torch.tensor(inv_samples(samples), dtype=torch.float32, device=p.device)


def gt(mean, tau):
    return mean > torch.tensor(float(tau), dtype=torch.float32, device=mean.device)
