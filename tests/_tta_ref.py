"""Mirror test-time averaging (include/dd_tta.h) in plain torch indexing: ``0.5 * (P(a) + P(m).flip(1))`` and ``> tau``.

On fp32 tensors ``a + b`` is one rounded add and ``0.5 * x`` is exact (below the subnormal range aside, which no input here reaches),
so the expressions below ARE the semantics, bit for bit.  For logits on the device ``P`` is ``ops.sigmoid``: the dense head's one
sigmoid, the same by construction.  ``mean_prob_cpu`` is the pure-CPU variant for probabilities."""
import torch


def mean_prob_cpu(a, m):
    """Probabilities [B,h,w] on any device, without any kernel of the package."""
    assert a.dtype == torch.float32 and m.dtype == torch.float32 and a.shape == m.shape and a.dim() == 3
    return 0.5 * (a + m.flip(1))


def sigmoid_dev(z):
    """``ops.sigmoid`` for any element count (it wants a multiple of 4: padded with zeros, cut back)."""
    from driving_dirty_amd import ops
    flat = z.contiguous().reshape(-1)
    pad = (-flat.numel()) % 4
    p = ops.sigmoid(torch.cat([flat, flat.new_zeros(pad)]).contiguous())
    return p[:flat.numel()].reshape(z.shape)


def mean_prob(a, m, from_logits):
    """Device tensors [B,h,w] -> the mean, as the header states it."""
    if from_logits:
        a, m = sigmoid_dev(a), sigmoid_dev(m)
    return mean_prob_cpu(a, m)


def gt(mean, tau):
    """``mean > tau``, strictly, tau rounded to fp32; NaN compares False."""
    return mean > torch.tensor(tau, dtype=torch.float32, device=mean.device)
