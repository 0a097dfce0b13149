"""Inputs of the dd_linear_sigmoid_gt tests, shared by the CPU test that checks them (test_ts_curve_ref.py) and the GPU test that
uses them (test_gpu_predict.py): seeded numpy, the same numbers on any machine."""
import math

import numpy as np

M_SIZES = (1, 2, 33, 65, 130)          # one 32-row tile, two, the 64-row chunk boundary, three launches
N_SIZES = (64, 1000, 4099)             # below one 128-column block, % 16 != 0, % 4 != 0 with a ragged last block
K_SIZES = (64, 128)                    # the latent of the width-128 and the width-256 configuration
CASES = [(m, n, k) for k in K_SIZES for n in N_SIZES for m in M_SIZES] + [(2, 640000, 64)]      # + the head's own width once
TAUS = (0.5, 0.25, 250.0 / 256.0)
BAND_REL, BAND_ABS, BAND_CAP = 2e-5, 1e-6, 1e-3


def head_inputs(m, n, k):
    """x ~ N(0, 1) [m, k], w ~ U(-1/8, 1/8) [n, k], bias ~ U(-0.1, 0.1) [n], fp32."""
    rs = np.random.RandomState(1000003 * m + 101 * k + n)
    x = rs.standard_normal((m, k)).astype(np.float32)
    w = (rs.random_sample((n, k)) * 0.25 - 0.125).astype(np.float32)
    b = (rs.random_sample(n) * 0.2 - 0.1).astype(np.float32)
    return x, w, b


def band_mask(logit64, tau):
    """Elements whose fp64 logit is within the kernel contract (2e-5 of the peak logit) of the threshold's logit: there, and only
    there, an fp32 kernel may land on the other side of ``sigmoid(logit) > tau``."""
    edge = math.log(tau / (1.0 - tau))
    return abs(logit64 - edge) <= BAND_REL * abs(logit64).max() + BAND_ABS
