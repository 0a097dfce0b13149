"""The reference, the fp32 model and the input grids of decoupled weight decay (include/dd_adamw.h): ``p1 = fl32(p * keep)``, then the
Adam element of tests/_element_ref.py on ``(p1, g, m, v)``.  CPU only (numpy).  The bounds and the grids are _element_ref's, taken from
the ROUNDED p1: the multiply is one correctly rounded fp32 operation, part of the definition and not of the error.
"""
import numpy as np

import _element_ref as E
from _element_ref import D, F, N_GRID  # noqa: F401

KEEPS = (1.0, 1.0 - 1e-5, 0.99, 0.5)       # off; a small decay (lr 1e-3 x wd 1e-2); 1 %; a power of two (the multiply is exact)
SIZES = (N_GRID, 1, 3, 4)                  # the 16-byte body + more than one workgroup + a 3-element tail; a tail alone; one vector alone
# (lr, weight_decay) whose 1 - lr * wd is no fp32 number (tests/test_adamw_ref.py asserts that of each)
LR_WD = ((1e-3, 1e-2), (1e-3, 0.05), (3e-4, 0.1), (1e-2, 1e-2), (0.1, 0.3), (1e-3, 1.0), (0.3, 0.3))      # the last: fp32 arithmetic on fp32 arguments gives another number


def keep32(lr, weight_decay):
    """``keep`` as the kernels are handed it: the product and the difference in double, ONE rounding to fp32."""
    return F(1.0 - float(lr) * float(weight_decay))


def decayed(p, keep):
    """p1: one rounding to fp32 of p * keep (numpy's float32 multiply is correctly rounded)."""
    with np.errstate(all="ignore"):
        return (np.asarray(p, dtype=F) * F(keep)).astype(F)


def adamw64(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, keep=1.0, round_p1=True):
    """One step of torch.optim.AdamW on fp32 state -> (p1, M, V, U, mag): ``p1`` the decayed parameter, the rest ``adam64`` of
    (p1, g, m, v); the new parameter is p1 + U.  ``round_p1=False`` leaves p * keep in fp64 (``keep`` then as it is given): AdamW in
    exact arithmetic, what tests/test_adamw_ref.py holds against torch in fp64."""
    p1 = decayed(p, keep) if round_p1 else np.asarray(p, dtype=D) * D(keep)
    M, V, U, mag = E.adam64(p1, g, m, v, lr, b1, b2, eps, step, grad_scale)
    return p1, M, V, U, mag


def model_adamw(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, keep=1.0):
    """The fp32 model: ``model_adam`` of _element_ref on the decayed parameter -> (p, m, v)."""
    return E.model_adam(decayed(p, keep), g, m, v, lr, b1, b2, eps, step, grad_scale)


def grid(n=N_GRID):
    """(p, g, m, v): the first ``n`` elements of ``adam_grid()``."""
    return tuple(t[:n].copy() for t in E.adam_grid())


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.int32)
