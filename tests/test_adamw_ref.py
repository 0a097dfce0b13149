"""The reference of tests/_adamw_ref.py against torch.optim.AdamW, without a GPU: the algorithm in fp64, the one fp32 rounding that
defines ``keep`` and ``p1``, and the fp32 model on the grids the GPU tests use."""
import numpy as np
import pytest
import torch

import _adamw_ref as ref
import _element_ref as E
from _element_ref import D, F


def f32(x):
    return float(F(x))


def test_the_reference_is_adamw_in_fp64_over_several_steps():
    """Four consecutive steps of torch.optim.AdamW on fp64 tensors against the reference with p * keep left in fp64
    (``round_p1=False``), state carried in fp64: every p, exp_avg and exp_avg_sq to 1e-12 relative.  The hyper-parameters are given
    to torch as the fp32 numbers the kernels take; the betas are ones whose 1 - beta is exact in fp32 (0.875, 1 - 2^-10), because the
    kernels' 1 - beta is an fp32 subtraction (dd_adam.h) and torch's a double one."""
    rs = np.random.RandomState(3)
    n, lr, wd, b1, b2, eps = 257, f32(1e-3), 0.05, 0.875, 1.0 - 2.0 ** -10, f32(1e-8)
    assert f32(b1) == b1 and f32(b2) == b2 and float(F(1) - F(b1)) == 1.0 - b1 and float(F(1) - F(b2)) == 1.0 - b2
    p0 = rs.uniform(-2, 2, n)
    grads = [rs.uniform(-1, 1, n) * 10.0 ** rs.uniform(-4, 0, n) for _ in range(4)]
    q = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.AdamW([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    keep = 1.0 - lr * wd
    for step, g in enumerate(grads, 1):
        q.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        # fp64 state in, fp64 out: adam64 takes its tensors as fp64 whatever they hold
        p1, M, V, U, _ = ref.adamw64(p, g, m, v, lr, b1, b2, eps, step, 1.0, keep, round_p1=False)
        p, m, v = p1 + U, M, V
        st = opt.state[q]
        for name, mine, theirs in (("p", p, q.detach().numpy()), ("m", m, st["exp_avg"].numpy()), ("v", v, st["exp_avg_sq"].numpy())):
            err = np.abs(mine - theirs).max() / np.abs(theirs).max()
            print(f"step {step} {name}: {err:.3g}")
            assert err <= 1e-12, (step, name, err)
    assert int(opt.state[q]["step"]) == 4


def test_rounding_p1_moves_the_reference_by_half_an_ulp_of_p1_and_no_more():
    """The rounded and the exact p * keep differ by at most half an ulp of p1; where the product is exact in fp32 (keep a power of
    two) the two references are the same numbers."""
    p, g, m, v = ref.grid(4099)
    cfg = (1e-3, 0.9, 0.999, 1e-8, 10, 1.0)
    for keep in ref.KEEPS:
        k = F(keep)
        r = ref.adamw64(p, g, m, v, *cfg, keep=k)
        x = ref.adamw64(p, g, m, v, *cfg, keep=D(k), round_p1=False)
        assert r[0].dtype == np.float32 and np.all(np.abs(D(r[0]) - x[0]) <= 0.5 * D(np.spacing(np.abs(r[0]))))
        for a, b in zip(r[1:], x[1:]):
            assert np.array_equal(a, b), "the moments and the update never see the decay"
        if keep in (1.0, 0.5):
            assert np.array_equal(D(r[0]), x[0])
    assert np.array_equal(ref.bits(ref.decayed(p, 1.0)), ref.bits(p)), "keep == 1 keeps p's bits"


@pytest.mark.parametrize("foreach", [False, True])
def test_zero_gradients_and_zero_moments_give_p_times_keep_bit_for_bit(foreach):
    """One fp32 step of torch.optim.AdamW on the CPU with g = m = v = 0: p * float32(1 - lr * wd), the bits of ``decayed`` and of the
    fp32 model, for pairs whose 1 - lr * wd is no fp32 number."""
    p0 = ref.grid(4099)[0]
    zeros = np.zeros_like(p0)
    for lr, wd in ref.LR_WD:
        q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch.optim.AdamW([q], lr=lr, weight_decay=wd, foreach=foreach)
        q.grad = torch.zeros_like(q)
        opt.step()
        keep = ref.keep32(lr, wd)
        want = ref.decayed(p0, keep)
        assert np.array_equal(ref.bits(q.detach().numpy()), ref.bits(want)), (lr, wd)
        got = ref.model_adamw(p0, zeros, zeros, zeros, lr, 0.9, 0.999, 1e-8, 1, 1.0, keep)
        assert np.array_equal(ref.bits(got[0]), ref.bits(want)) and not got[1].any() and not got[2].any()
        assert not np.array_equal(want, p0)


def test_keep_is_one_rounding_of_the_double():
    from driving_dirty_amd import adamw
    differs = 0
    for lr, wd in ref.LR_WD:
        exact = 1.0 - lr * wd
        keep = adamw.keep_of(lr, wd)
        assert isinstance(keep, float) and keep == float(ref.keep32(lr, wd)) == float(F(exact))
        assert keep != exact, f"1 - {lr} * {wd} is an fp32 number: pick another pair"
        assert abs(keep - exact) <= 2.0 ** -25, "half an ulp of a number in [0.5, 1]"
        differs += float(F(1) - F(F(lr) * F(wd))) != keep      # what fp32 arithmetic on fp32 arguments would have given
    assert differs, "no pair tells the double computation from an fp32 one"
    assert adamw.keep_of(1e-3, 0.0) == 1.0 and adamw.keep_of(0.0, 5.0) == 1.0 and adamw.keep_of(0.5, 2.0) == 0.0
    for lr, wd in ((1.0, 1.5), (1e-3, float("nan")), (1e-3, float("inf"))):
        with pytest.raises(ValueError, match="keep"):
            adamw.keep_of(lr, wd)


def test_the_fp32_model_stays_inside_the_bounds_taken_from_p1():
    """The model of the kernels against ``adamw64`` on one step's 16 configurations x KEEPS, within the MODEL's constants of
    _element_ref (no hardware allowance: the model's square root and reciprocal are correctly rounded)."""
    p, g, m, v = ref.grid(8195)
    worst = 0.0
    for cfg in E.adam_configs(step=10):
        for keep in ref.KEEPS:
            k = F(keep)
            p1, M, V, U, mag = ref.adamw64(p, g, m, v, *cfg, keep=k)
            pn, mn, vn = ref.model_adamw(p, g, m, v, *cfg, keep=k)
            ok = E.adam_bounded(M, V, U)
            tol = E.adam_bounds(p1, M, V, U, mag, kv=E.ADAM_MODEL_KV, km=E.ADAM_MODEL_KM, ku=E.ADAM_MODEL_KU)
            err = E.adam_errors(p1, pn, mn, vn, M, V, U)
            for e, t in zip(err, tol):
                worst = max(worst, float(E.error_fraction(e[ok], t[ok]).max()))
    print(f"worst error / bound: {worst:.3f}")
    assert worst <= 1.0
