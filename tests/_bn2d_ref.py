"""fp64 reference, seeded inputs and error bounds for the BatchNorm2d kernel family of the Conv -> BatchNorm2d -> ReLU variant
(csrc/bn2d.hip, the statistics epilogue of dd_conv_fwd_stats, dd_conv_dgrad_bn / dd_conv_wgrad_bn): plain torch on the CPU, following
include/dd_hotpath.h.  Tensors are NHWC, 32 channels last; every input is an fp32 tensor that the reference takes exactly.

THE BOUND, stated before any kernel ran: an output's error, relative to the peak of the reference tensor, is at most
max(B, MARGIN * E_ref).  B is the bound the guard-band cases use for that output (KERNEL_TOL; GRAD_TOL = 10 x KERNEL_TOL for du,
dgamma, dbeta).  E_ref is the error of torch's own fp32 batch norm (forward and autograd, on the CPU) on the same inputs against the
same fp64 reference (`reference_fp32_error`): with a large offset |mean| / sigma no fp32 implementation can meet B, because u itself
is only known to 2^-24 |mean|.  MARGIN = 4: the kernels fold (u - mean) invstd gamma + beta into u sc + sh, two more roundings at the
magnitude |mean| sc; a CPU model of an exact-statistics kernel with the folded form stays within 2.5 x torch's error for ratios 0..4096.

THE EXCLUSION CAP: a ReLU or mask decision may flip where the fp64 pre-activation |z| <= FLIP_ULPS * 2^-24 * max|u sc| of its channel;
such elements may be left out of a gradient comparison, at most FLIP_CAP of a tensor's elements.  tests/test_bn2d_ref.py asserts that the
inputs used here stay under the cap on the reference alone.  For the pooling gradient the decision is which tap of a window is its
maximum: a window whose two largest pre-activations are closer than that threshold without being equal is left out as a whole."""
import functools
import math

import torch
from torch.nn import functional as F

from driving_dirty_amd import synth

C = 32
KERNEL_TOL = 2e-5                 # tests/test_gpu_guard_layout.py, tests/test_gpu_guard_conv.py: of the tensor's peak
GRAD_TOL = 10 * KERNEL_TOL        # du, dgamma, dbeta there
MARGIN = 4
FLIP_ULPS, FLIP_CAP = 8, 1e-3
EPS, MOMENTUM = 1e-5, 0.1
RATIOS = (0, 1, 8, 64, 512)       # |mean| / sigma of the stand-alone chain
CONV_RATIOS = (0, 8, 64, 512)     # bias / (std of the bias-free conv output) of dd_conv_fwd_stats
ZERO_MEAN_CHANNEL = 5
GRID_CAP_PIXELS = 65536           # dd_grid_for: 2048 workgroups of 256 lanes, 8 lanes per pixel -> past it a lane makes a second trip
CHAIN_PIXELS = (2, 63, 1408, 257 * 257)      # 257 * 257 = 66049: the smallest odd count past the cap, some lanes make two trips and some one
OUTPUT_BOUNDS = {"save_mean": KERNEL_TOL, "save_invstd": KERNEL_TOL, "affine": KERNEL_TOL, "running_mean": KERNEL_TOL,
                 "running_var": KERNEL_TOL, "y": KERNEL_TOL, "du": GRAD_TOL, "dgamma": GRAD_TOL, "dbeta": GRAD_TOL}
# (cin, stride, has in_affine): the three layers of the v2 encoder
CONV_KINDS = ((3, 1, False), (32, 1, True), (32, 2, True))
CONV_SHAPES = ((2, 7, 33), (3, 5, 65))       # ragged last strips of one pixel (33 = 32 + 1, 65 = 64 + 1; under stride 2: 17, 33), odd heights
# dd_pool4_bn_*: one lane per (window, 4-channel group), so ITS grid-stride loop makes a second trip past 4 * 65536 pixels only:
# (1, 258, 256) stays inside the cap (516 workgroups), (1, 513, 512) = 262656 pixels is the smallest odd-height shape past it
POOL_SHAPES = ((2, 6, 10), (1, 258, 256), (1, 513, 512))


def hu(shape, name, lo=-1.0, hi=1.0, dtype=torch.float32):
    return synth.hash_uniform(shape, synth.key_salt(name), lo, hi, dtype)


# ------------------------------------------------------------------------------------------------ inputs
def channel_signs():
    """fp64 [32]: +1, -1 alternating, 0 at ZERO_MEAN_CHANNEL -- every channel its own offset, so a channel mix-up shows."""
    s = torch.tensor([1.0 if c % 2 == 0 else -1.0 for c in range(C)], dtype=torch.float64)
    s[ZERO_MEAN_CHANNEL] = 0.0
    return s


def channel_sigma():
    return hu((C,), "bn2d_sigma", 0.25, 1.0, torch.float64)


def inputs(shape, ratio, name="bn2d_u"):
    """fp32 [*shape, 32]: u[..., c] = sigma_c * noise + mean_c, noise uniform with unit variance, mean_c = +-ratio * sigma_c."""
    noise = hu(tuple(shape) + (C,), f"{name}{tuple(shape)}", -math.sqrt(3.0), math.sqrt(3.0), torch.float64)
    sigma = channel_sigma()
    return (noise * sigma + channel_signs() * ratio * sigma).float()


def gamma_beta(kind):
    """fp32 (gamma, beta).  "positive": gamma in [0.5, 1.5].  "signs": channels 3k negative, 3k + 1 exactly zero (beta +0.3 and -0.3
    alternating on them), 3k + 2 positive."""
    g, b = hu((C,), "bn2d_gamma", 0.5, 1.5), hu((C,), "bn2d_beta", -0.5, 0.5)
    if kind == "signs":
        for c in range(C):
            if c % 3 == 0:
                g[c] = -g[c]
            elif c % 3 == 1:
                g[c] = 0.0
                b[c] = 0.3 if c % 2 else -0.3
    else:
        assert kind == "positive", kind
    return g, b


def running_stats():
    return hu((C,), "bn2d_rm", -0.3, 0.3), hu((C,), "bn2d_rv", 0.5, 1.5)


# ------------------------------------------------------------------------------------------------ the fp64 chain
def batch_stats(u):
    """(mean, biased variance) fp64 [32] over every dimension but the last, two-pass."""
    u64 = u.double().reshape(-1, C)
    mean = u64.mean(0)
    return mean, ((u64 - mean) ** 2).mean(0)


def affine_table(mean, invstd, gamma, beta):
    sc = gamma.double() * invstd
    sh = beta.double() - mean * sc
    return torch.cat([sc, sh, sc, sh])


def chain(u, gamma, beta, rm0, rv0, g_raw, training, momentum=MOMENTUM, eps=EPS):
    """dd_bn2d_stats -> _finalize -> _apply_relu -> _bwd in fp64.  `g_raw` is the gradient w.r.t. the ReLU's OUTPUT; "g" of the result
    is what dd_bn2d_bwd is handed (masked by the fp64 ReLU), "z" the pre-activation."""
    u64 = u.double().reshape(-1, C)
    n = u64.shape[0]
    if training:
        mean, var = batch_stats(u64)
        rm = (1 - momentum) * rm0.double() + momentum * mean
        rv = (1 - momentum) * rv0.double() + momentum * var * n / (n - 1)
    else:
        mean, var, rm, rv = rm0.double(), rv0.double(), rm0.double(), rv0.double()
    invstd = 1 / (var + eps).sqrt()
    aff = affine_table(mean, invstd, gamma, beta)
    sc, sh = aff[:C], aff[C:2 * C]
    z = u64 * sc + sh
    g = g_raw.double().reshape(-1, C) * (z > 0)
    xhat = (u64 - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    du = sc * (g - dbeta / n - xhat * dgamma / n) if training else sc * g
    shape = tuple(u.shape)
    return {"save_mean": mean, "save_invstd": invstd, "affine": aff, "running_mean": rm, "running_var": rv, "z": z.reshape(shape),
            "y": F.relu(z).reshape(shape), "g": g.reshape(shape), "du": du.reshape(shape), "dgamma": dgamma, "dbeta": dbeta}


def peak_error(got, want):
    """max |got - want| / max |want| (fp64, on the CPU); a reference that is identically zero must be met exactly."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.numel() == 0:
        return 0.0
    err, peak = float((got - want).abs().max()), float(want.abs().max())
    if not math.isfinite(err):
        return math.inf
    if peak == 0.0:
        return 0.0 if err == 0.0 else math.inf
    return err / peak


def fp32_batch_norm(u, gamma, beta, rm0, rv0, g, training, momentum=MOMENTUM, eps=EPS):
    """torch's own fp32 batch norm on the CPU, forward and autograd, on the inputs the kernels get (`g` already masked): the outputs of
    `chain` by name."""
    x = u.reshape(-1, C).t().unsqueeze(0).contiguous().requires_grad_(True)      # [1, 32, npix]
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    z, sm, si = torch.native_batch_norm(x, gm, bt, rm, rv, bool(training), momentum, eps)
    if not training:
        sm, si = rm0.clone(), 1 / (rv0 + eps).sqrt()
    z.backward(g.reshape(-1, C).t().unsqueeze(0).contiguous())
    sc = gamma * si
    sh = beta - sm * sc
    back = lambda t: t.detach()[0].t().reshape(tuple(u.shape))
    return {"save_mean": sm.detach(), "save_invstd": si.detach(), "affine": torch.cat([sc, sh, sc, sh]), "running_mean": rm, "running_var": rv,
            "y": back(F.relu(z)), "du": back(x.grad), "dgamma": gm.grad, "dbeta": bt.grad}


def reference_fp32_error(u, gamma, beta, rm0, rv0, g, training, want=None):
    """{output: E_ref}: the error of `fp32_batch_norm` against `chain` (`want`: its result, when the caller has it), as peak_error."""
    if want is None:
        want = chain(u, gamma, beta, rm0, rv0, g, training)
    got = fp32_batch_norm(u, gamma, beta, rm0, rv0, g, training)
    return {k: peak_error(v, want[k]) for k, v in got.items()}


def bound(name, e_ref):
    return max(OUTPUT_BOUNDS[name], MARGIN * e_ref)


@functools.lru_cache(maxsize=8)
def chain_case(npix, ratio, training, kind="positive"):
    """Everything a test of the stand-alone chain needs, computed once: the fp32 inputs, the fp64 outputs, E_ref per output."""
    u = inputs((npix,), ratio)
    gamma, beta = gamma_beta(kind)
    rm0, rv0 = running_stats()
    g_raw = hu((npix, C), f"bn2d_g{npix}")
    want = chain(u, gamma, beta, rm0, rv0, g_raw, training)
    g = want["g"].float()
    want = chain(u, gamma, beta, rm0, rv0, g, training)      # the gradient the kernel is handed is the ROUNDED masked one (g * mask == g)
    return {"u": u, "gamma": gamma, "beta": beta, "rm0": rm0, "rv0": rv0, "g": g, "want": want,
            "e_ref": reference_fp32_error(u, gamma, beta, rm0, rv0, g, training, want)}


# ------------------------------------------------------------------------------------------------ flips
def flip_threshold(u, sc):
    """fp64 [32]: FLIP_ULPS * 2^-24 * max |u sc| per channel."""
    return FLIP_ULPS * 2.0 ** -24 * (u.double().reshape(-1, C) * sc.double()).abs().amax(0)


def undecided(u, sc, sh):
    """bool, u's shape: the elements whose sign of z = u sc + sh an fp32 evaluation may get wrong."""
    z = u.double() * sc.double() + sh.double()
    return z.abs() <= flip_threshold(u, sc)


# ------------------------------------------------------------------------------------------------ the pool
def _windows(u, sc, sh):
    b, h, w, _ = u.shape
    feat = F.relu(u.double() * sc.double() + sh.double()).permute(0, 3, 1, 2).reshape(b, C * h * w // 4, 4)      # NCHW order, windows of 4
    return feat


def pool4(u, sc, sh):
    """NCHW-order max_pool1d(4) over relu(u sc + sh): fp64 [B, 32 H W / 4]."""
    return _windows(u, sc, sh).amax(2)


def pool4_bwd(gp, u, sc, sh):
    """Its backward, as the gradient w.r.t. the BN output with the ReLU applied: fp64 NHWC.  The first of equal taps takes the gradient,
    a window whose maximum is 0 none."""
    b, h, w, _ = u.shape
    feat = _windows(u, sc, sh)
    m = feat.amax(2, keepdim=True)
    is_max = feat == m
    first = is_max & (is_max.double().cumsum(2) == 1)
    d = first.double() * (gp.double().reshape(b, -1, 1) * (m > 0))
    return d.reshape(b, C, h, w).permute(0, 2, 3, 1).contiguous()


def pool_undecided(u, sc, sh):
    """bool NHWC: the elements of the windows whose gradient an fp32 evaluation may route otherwise -- the maximum's sign is undecided, or
    the two largest taps are closer than the flip threshold without being equal (which of them is the maximum is such a decision too)."""
    b, h, w, _ = u.shape
    thr = flip_threshold(u, sc).view(1, C, 1).expand(b, C, h * w // 4).reshape(b, -1)
    z = (u.double() * sc.double() + sh.double()).permute(0, 3, 1, 2).reshape(b, -1, 4)
    top = z.topk(2, dim=2).values
    gap = top[..., 0] - top[..., 1]
    skip = (top[..., 0].abs() <= thr) | ((gap > 0) & (gap <= thr) & (top[..., 0] > -thr))
    return skip.unsqueeze(2).expand(-1, -1, 4).reshape(b, C, h, w).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=2)
def pool_case(shape):
    """The inputs of a dd_pool4_bn_fwd / _bwd test: u at ratio 1, the (scale, shift) table of gamma_beta("signs") from u's own statistics."""
    b, h, w = shape
    u = inputs(shape, 1, "bn2d_pool")
    gamma, beta = gamma_beta("signs")
    mean, var = batch_stats(u)
    aff = affine_table(mean, 1 / (var + EPS).sqrt(), gamma, beta).float()
    sc, sh = aff[:C], aff[C:2 * C]
    gp = hu((b, C * h * w // 4), f"bn2d_gp{shape}")
    return {"u": u, "affine": aff, "gp": gp, "pooled": pool4(u, sc, sh), "dfeat": pool4_bwd(gp, u, sc, sh), "skip": pool_undecided(u, sc, sh)}


# ------------------------------------------------------------------------------------------------ the conv layers
def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=4)
def conv_layer(kind, shape):
    """The ratio-independent part of a dd_conv_fwd_stats case: the stored input (NHWC fp32; 4 stored channels for the image layer), the
    in_affine table or None, the weights, the bias-free fp64 output (NHWC) and its per-channel standard deviation."""
    cin, stride, aff_in = kind
    b, h, w = shape
    wt = hu((C, cin, 3, 3), f"bn2d_w{cin}{stride}", -0.3, 0.3)
    if aff_in:
        pre = inputs(shape, 1, "bn2d_pre")
        gamma, beta = gamma_beta("positive")
        mean, var = batch_stats(pre)
        aff = affine_table(mean, 1 / (var + EPS).sqrt(), gamma, beta).float()
        xin = F.relu(pre.double() * aff[:C].double() + aff[C:2 * C].double())
        x = pre
    else:
        img = hu((b, h, w, 3), f"bn2d_img{shape}", 0.0, 1.0)
        x = torch.zeros(b, h, w, 4)
        x[..., :3] = img
        aff, xin = None, img.double()
    conv0 = nhwc(F.conv2d(nchw(xin), wt.double(), None, stride=stride, padding=1))
    return {"x": x, "affine": aff, "weight": wt, "conv0": conv0, "std": batch_stats(conv0)[1].sqrt()}


def conv_bias(layer, ratio):
    """fp32 [32]: the offset as it arises in training -- bias_c = +-ratio * (std of channel c of the bias-free output), 0 on one channel."""
    return (channel_signs() * ratio * layer["std"]).float()


@functools.lru_cache(maxsize=2)
def sign_layer(stride, shape=CONV_SHAPES[0]):
    """A 32 -> 32 layer whose input is seen through a table of gamma_beta("signs"): the INPUT pair [0:64) from the signed gamma, the MASK
    pair [64:128) the same rolled by one channel (so a kernel that reads the wrong pair fails, and the signs differ per channel between them).
    fp64 references: u = conv(relu(pre sc + sh)) + bias, dx = conv^T(gy) * (pre msc + msh > 0), dw, dbias."""
    b, h, w = shape
    pre = inputs(shape, 1, "bn2d_spre")
    gamma, beta = gamma_beta("signs")
    mean, var = batch_stats(pre)
    t = affine_table(mean, 1 / (var + EPS).sqrt(), gamma, beta).float()
    sc, sh = t[:C], t[C:2 * C]
    msc, msh = torch.roll(sc, 1), torch.roll(sh, 1)
    aff = torch.cat([sc, sh, msc, msh])
    wt = hu((C, C, 3, 3), f"bn2d_sw{stride}", -0.3, 0.3)
    bias = hu((C,), f"bn2d_sb{stride}", -0.2, 0.2)
    xin = nchw(F.relu(pre.double() * sc.double() + sh.double())).requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), bias.double().requires_grad_(True)
    u = F.conv2d(xin, w64, b64, stride=stride, padding=1)
    gy = hu(tuple(nhwc(u).shape), f"bn2d_sgy{stride}")
    u.backward(nchw(gy).double())
    mask = (pre.double() * msc.double() + msh.double()) > 0
    return {"pre": pre, "affine": aff, "weight": wt, "bias": bias, "gy": gy, "u": nhwc(u.detach()), "dx": nhwc(xin.grad) * mask,
            "dw": w64.grad, "dbias": b64.grad, "skip": undecided(pre, msc, msh)}


# ------------------------------------------------------------------------------------------------ models of the two accumulation schemes
def _lanes(u, lanes):
    """u [n, 32] fp32 -> (values [trips, lanes, 32] fp32, valid [trips, lanes] bool): pixel p is met by lane p % lanes on trip p // lanes,
    as in a grid-stride loop."""
    n = u.shape[0]
    trips = -(-n // lanes)
    v = torch.zeros(trips * lanes, C)
    v[:n] = u
    ok = torch.zeros(trips * lanes, dtype=torch.bool)
    ok[:n] = True
    return v.reshape(trips, lanes, C), ok.reshape(trips, lanes)


def model_raw_moments(u, lanes=GRID_CAP_PIXELS):
    """(mean, invstd) fp64 from per-lane fp32 sums of v and of fl(v v), the lanes combined in fp64, var = q/n - m^2 in fp64: what the
    kernels did before they kept a pivot."""
    u = u.reshape(-1, C)
    v, ok = _lanes(u, min(lanes, u.shape[0]))
    s, q = torch.zeros(v.shape[1], C), torch.zeros(v.shape[1], C)
    for t in range(v.shape[0]):
        m = ok[t].unsqueeze(1)
        s = torch.where(m, s + v[t], s)
        q = torch.where(m, q + v[t] * v[t], q)
    n = u.shape[0]
    mean = s.double().sum(0) / n
    var = (q.double().sum(0) / n - mean * mean).clamp_min(0.0)
    return mean, 1 / (var + EPS).sqrt()


def model_merged_moments(u, lanes=GRID_CAP_PIXELS, row=32):
    """(mean, invstd) fp64 from per-lane fp32 moments about the lane's first value, `row` lanes merged in fp64 into (n, mean, M2) stored as
    fp32 (the mean in two), the rows merged by Chan's formula in fp64: what the kernels do."""
    u = u.reshape(-1, C)
    v, ok = _lanes(u, min(lanes, u.shape[0]))
    piv = v[0]
    s, q, cnt = torch.zeros_like(piv), torch.zeros_like(piv), torch.zeros(v.shape[1], 1)
    for t in range(v.shape[0]):
        m = ok[t].unsqueeze(1)
        d = v[t] - piv
        s = torch.where(m, s + d, s)
        q = torch.where(m, q + d * d, q)
        cnt = cnt + m.float()
    pad = (-v.shape[1]) % row
    z = lambda x: torch.cat([x.double(), torch.zeros(pad, x.shape[1], dtype=torch.float64)]).reshape(-1, row, x.shape[1])
    n_l, p_l, s_l, q_l = z(cnt), z(piv), z(s), z(q)
    d = p_l - p_l[:, :1]                                   # every lane of a row onto the first lane's pivot
    n_r = n_l.sum(1)
    s_r = (s_l + n_l * d).sum(1)
    q_r = (q_l + d * (2 * s_l + n_l * d)).sum(1)
    mean_r = p_l[:, 0] + s_r / n_r.clamp_min(1)
    mean_r = mean_r.float().double() + (mean_r - mean_r.float().double()).float().double()      # two floats: the fp32 mean and what it rounds away
    m2_r = (q_r - s_r * s_r / n_r.clamp_min(1)).clamp_min(0.0).float().double()
    n = n_r.sum(0)
    mean = (n_r * mean_r).sum(0) / n
    m2 = m2_r.sum(0) + (n_r * (mean_r - mean) ** 2).sum(0)
    return mean, 1 / (m2 / n + EPS).sqrt()
