"""fp64 reference of include/dd_ema.h, its error bounds, and the inputs the EMA tests share.

The reference: ``e + float64(float32(alpha)) * (w - e)`` in fp64, and that recurrence for several steps (carried in fp64, never
rounded to fp32 on the way).

The bound is derived, not measured.  With M = max(|e|, |w|) per element the kernel's subtract errs by at most 2^-24 |w - e| <=
2^-23 M, alpha <= 1 does not grow that, and the fused multiply-add adds at most 2^-24 M: 1.5 * 2^-23 M in all.  One update is held
to 2^-22 M plus one denormal ulp.  Over k updates with a fixed alpha the errors contract by (1 - alpha) each step, so their sum
stays below the one-step bound / alpha: the k-step result is held to 2^-22 M_run / alpha plus one denormal ulp, M_run the running
maximum of M."""
import numpy as np
import torch

from driving_dirty_amd import synth

EPS22 = 2.0 ** -22
DENORMAL_ULP = 2.0 ** -149


def f32(alpha):
    """The fp32 the launcher is handed, as a Python float."""
    return float(np.float32(alpha))


def update(e, w, alpha):
    """One update in fp64.  ``e``, ``w``: tensors of any float dtype (the fp64 state of a recurrence, or fp32 values)."""
    e, w = e.detach().double().cpu(), w.detach().double().cpu()
    return e + f32(alpha) * (w - e)


def magnitude(e, w):
    return torch.maximum(e.detach().double().cpu().abs(), w.detach().double().cpu().abs())


def one_step_bound(m):
    return EPS22 * m + DENORMAL_ULP


def k_step_bound(m_run, alpha):
    return EPS22 * m_run / f32(alpha) + DENORMAL_ULP


def assert_within(got, want, bound, what):
    """Every element of fp32 ``got`` within ``bound`` (a tensor) of fp64 ``want``; prints the worst ratio first."""
    err = (got.detach().double().cpu() - want).abs()
    ratio = float((err / bound).max())
    print(f"{what}: worst error / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), (what, ratio)


def pair(n, name):
    """(e, w) fp32 [n] on the CPU: hash_uniform in +-2, and w within 1e-3 of e for half of the elements (the even ones)."""
    e = synth.hash_uniform((n,), synth.key_salt("ema_e_" + name), -2.0, 2.0)
    w = synth.hash_uniform((n,), synth.key_salt("ema_w_" + name), -2.0, 2.0)
    near = e + synth.hash_uniform((n,), synth.key_salt("ema_d_" + name), -1e-3, 1e-3)
    w[0::2] = near[0::2]
    return e, w


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def word_patterns(n, name):
    """fp32 [n] on the CPU whose first words are the bit patterns a float copy could damage: quiet and signalling NaNs with
    payloads, -0.0, +-inf, the smallest and the largest denormal; the rest hash values."""
    t = synth.hash_uniform((n,), synth.key_salt("ema_s_" + name), -2.0, 2.0)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8ABCDE, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000],
                       dtype=np.uint32).view(np.int32)
    words = t.view(torch.int32).clone()
    k = min(n, len(special))
    words[:k] = torch.from_numpy(special[:k].copy())
    return words.view(torch.float32)
