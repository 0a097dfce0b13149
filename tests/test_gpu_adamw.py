"""GPU tests of the kernels of include/dd_adamw.h (csrc/libdd_adamw.so) on the grids of tests/_element_ref.py: ``dd_adamw_step`` in
both scale forms, ``dd_adamw_step_multi`` and ``dd_decay``, against each other and the parent's kernels bit for bit and against the fp64
reference of tests/_adamw_ref.py within the bounds of _element_ref taken from the rounded ``p1``.  p, m and v are compared as int32
views, so that NaN patterns count."""
import numpy as np
import pytest
import torch

import _adamw_ref as ref
import _element_ref as E
from _element_ref import F

pytestmark = pytest.mark.gpu

SMALL = tuple(n for n in ref.SIZES if n != ref.N_GRID)      # 1, 3, 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import adamw
    adamw.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def state(dev):
    host = E.adam_grid()
    return host, tuple(torch.from_numpy(t).to(dev) for t in host)


def k32(keep):
    return float(F(keep))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def fused(st, cfg, keep, n=None, scale=None):
    """One dd_adamw_step on clones of the first n elements -> (p, m, v); ``scale``: a device tensor in place of cfg's grad_scale."""
    from driving_dirty_amd import adamw
    p, g, m, v = (t[:n].clone() for t in st)
    lr, b1, b2, eps, step, gs = cfg
    adamw.step_flat(p, g, m, v, lr, b1, b2, eps, step, gs if scale is None else scale, k32(keep))
    return p, m, v


def sequential(st, cfg, keep, n=None, decay="torch"):
    """The separate multiply -- torch's, or dd_decay -- followed by the parent's dd_adam_step."""
    from driving_dirty_amd import adamw, ops
    p, g, m, v = (t[:n].clone() for t in st)
    lr, b1, b2, eps, step, gs = cfg
    if decay == "torch":
        p.mul_(k32(keep))
    elif decay == "dd_decay":
        adamw.decay(p, k32(keep))
    ops.adam_step_flat(p, g, m, v, lr, b1, b2, eps, step, gs)
    return p, m, v


@pytest.mark.parametrize("keep", ref.KEEPS)
def test_the_fused_pass_is_the_multiply_followed_by_the_parents_pass(dev, state, keep):
    """(a) dd_adamw_step == p.mul_(keep) + dd_adam_step, and == dd_decay + dd_adam_step; (c) keep == 1 == dd_adam_step alone; (d) the
    device-scale form == the by-value form.  All 96 configurations on the 65 539-element grid, one step's 16 on n = 1, 3, 4."""
    _, st = state
    for n, cfgs in [(ref.N_GRID, E.adam_configs())] + [(n, E.adam_configs(step=10)) for n in SMALL]:
        for cfg in cfgs:
            got = fused(st, cfg, keep, n)
            for a, b in zip(got, sequential(st, cfg, keep, n)):
                assert same_bits(a, b), (n, cfg, keep)
            on_dev = fused(st, cfg, keep, n, scale=torch.tensor([cfg[5]], device=dev, dtype=torch.float32))
            for a, b in zip(got, on_dev):
                assert same_bits(a, b), ("device scale", n, cfg, keep)
            if keep == 1.0:
                for a, b in zip(got, sequential(st, cfg, keep, n, decay=None)):
                    assert same_bits(a, b), ("keep == 1", n, cfg)
        for a, b in zip(fused(st, cfgs[0], keep, n), sequential(st, cfgs[0], keep, n, decay="dd_decay")):
            assert same_bits(a, b), ("dd_decay", n, keep)


@pytest.mark.parametrize("keep", ref.KEEPS)
def test_the_fused_pass_against_fp64_within_the_bounds_taken_from_p1(dev, state, keep):
    """(b) m within ADAM_KM x 2^-24 of its terms' magnitude, v within ADAM_KV x 2^-24, p_new - p1 within _element_ref's update bound with
    p1 = fl32(p * keep): the multiply is one correctly rounded operation and belongs to the definition."""
    host, st = state
    p, g, m, v = host
    worst = [0.0, 0.0, 0.0]
    for cfg in E.adam_configs():
        pn, mn, vn = (t.cpu().numpy() for t in fused(st, cfg, keep))
        p1, M, V, U, mag = ref.adamw64(p, g, m, v, *cfg, keep=F(keep))
        ok = E.adam_bounded(M, V, U)
        assert ok.mean() >= 0.99
        fr = [float(E.error_fraction(e, t)[ok].max()) for e, t in zip(E.adam_errors(p1, pn, mn, vn, M, V, U), E.adam_bounds(p1, M, V, U, mag))]
        assert np.max(fr) <= 1.0, (cfg, keep, fr)      # np.max keeps a NaN, which fails
        worst = [max(a, b) for a, b in zip(worst, fr)]
    print(f"keep {keep}: worst error / bound over 96 configurations: m {worst[0]:.3f}, v {worst[1]:.3f}, update {worst[2]:.3f}")


@pytest.mark.parametrize("step", [1, 1000])
def test_special_values(dev, step):
    """adam_special_grid() (zero, subnormal, infinite and NaN gradients; 16 vectors and a 3-element tail): the fused pass has the bits of
    the multiply followed by the parent's pass -- whose pattern of zeros, infinities and NaNs tests/test_gpu_element_range.py holds to
    torch's -- in both scale forms, and where the reference is bounded it lies within the bounds."""
    host = E.adam_special_grid()
    st = tuple(torch.from_numpy(t).to(dev) for t in host)
    cfg = (1e-3, 0.9, 0.999, 1e-8, step, 1.0)
    p, g, m, v = host
    for keep in ref.KEEPS:
        got = fused(st, cfg, keep)
        for other in (sequential(st, cfg, keep), fused(st, cfg, keep, scale=torch.ones(1, device=dev))):
            for a, b in zip(got, other):
                assert same_bits(a, b), (keep, step)
        if keep == 1.0:
            for a, b in zip(got, sequential(st, cfg, keep, decay=None)):
                assert same_bits(a, b)
        pn, mn, vn = (t.cpu().numpy() for t in got)
        p1, M, V, U, mag = ref.adamw64(p, g, m, v, *cfg, keep=F(keep))
        ok = E.adam_bounded(M, V, U)
        fr = [float(E.error_fraction(e, t)[ok].max()) for e, t in zip(E.adam_errors(p1, pn, mn, vn, M, V, U), E.adam_bounds(p1, M, V, U, mag))]
        assert ok.any() and np.max(fr) <= 1.0, (keep, fr)


MULTI_SIZES = (1, 255, 256, 257, 1000)


@pytest.mark.parametrize("count", [5, 49, 97])
def test_the_multi_tensor_launch_gives_the_flat_kernels_bits(dev, state, count):
    """Tensors of 1, 255, 256, 257 and 1000 elements at offsets that are no multiple of four elements; 49 and 97 of them cross the
    48-tensor table once and twice; a keep per tensor that includes 1.0; by value and with the device scale.  Each tensor has the bits of
    dd_adamw_step on an aligned copy (and so, by the test above, of the multiply followed by the parent's pass)."""
    from driving_dirty_amd import adamw
    _, st = state
    cfg = (1e-3, 0.9, 0.999, 1e-8, 3, 0.37)
    lr, b1, b2, eps, step, gs = cfg
    sizes = [MULTI_SIZES[i % 5] for i in range(count)]
    keeps = [k32(ref.KEEPS[i % 4]) for i in range(count)]
    assert 1.0 in keeps and len(set(keeps)) == 4
    spans, off = [], 1
    for size in sizes:
        spans.append((off, size))
        off += size + 5 + (size % 2)      # offsets 1, 7, ...: odd and even element offsets, never all multiples of four
    assert off <= ref.N_GRID and any(o % 4 for o, _ in spans)
    want = [fused(tuple(t[o:o + s] for t in st), cfg, k) for (o, s), k in zip(spans, keeps)]
    for scale in (gs, torch.tensor([gs], device=dev, dtype=torch.float32)):
        work = tuple(t.clone() for t in st)
        quads = [tuple(t[o:o + s] for t in work) for o, s in spans]
        adamw.step_multi(quads, keeps, lr, b1, b2, eps, step, scale)
        for (o, s), (p, _, m, v), w in zip(spans, quads, want):
            for a, b in zip((p, m, v), w):
                assert same_bits(a, b), (o, s)
        mask = torch.ones(ref.N_GRID, dtype=torch.bool, device=dev)
        for o, s in spans:
            mask[o:o + s] = False
        for t, t0 in zip((work[0], work[2], work[3]), (st[0], st[2], st[3])):
            assert same_bits(t[mask], t0[mask]), "an element between two tensors of the table was written"
        assert same_bits(work[1], st[1]), "the gradients are read only"


DECAY_BIG = 4 * (5 * 65536 + 1000) + 3      # past the capped grid (256 workgroups of 256 lanes, four vectors each): the unrolled loop, the
#                                             single-vector loop behind it twice, and the tail


@pytest.mark.parametrize("n", ref.SIZES + (DECAY_BIG,))
def test_decay_is_the_fp32_multiply_and_stops_at_n(dev, state, n):
    from driving_dirty_amd import _lib, adamw
    _, st = state
    extra = 8
    grid = torch.cat([st[0], st[2]])
    src = grid.repeat(-(-(n + extra) // grid.numel()))[:n + extra]
    _lib.call("dd_set_adam_blocks_per_cu", 1)      # the library's default, whatever an earlier test of the process left
    for keep in ref.KEEPS:
        buf = src.clone()
        adamw.decay(buf[:n], k32(keep))
        assert same_bits(buf[:n], src[:n] * k32(keep)), (n, keep)
        assert same_bits(buf[n:], src[n:]), "elements past n were written"
        assert same_bits(buf[:n].cpu(), torch.from_numpy(ref.decayed(src[:n].cpu().numpy(), keep)))
