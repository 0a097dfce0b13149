"""Guard-band cases (tests/_guard.py) for the launch functions of include/dd_adamw.h (csrc/libdd_adamw.so): every operand with 64 KiB
of 0xFF around it, at the alignment the header states and no more -- 16 bytes for the flat buffers, 4 for the tensors of a table and
for the device scale.  What a case asserts: tests/test_gpu_guard_dense.py.  Both scale forms of the two step functions are cases of
their own (two kernels each).  No launcher picks a kernel by alignment, so the two modes are compared bit for bit.
tests/test_adamw_surface.py checks, without a GPU, that every function of the header is the subject of a case here.

An over-read whose value is discarded cannot be seen by these tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import _adamw_ref as ref
from _guard import Case, Check, adam_table, run_case

pytestmark = pytest.mark.gpu

P_TOL, MV_TOL = 1e-6, 2e-6      # tests/test_gpu_guard_dense.py: ADAM_P_TOL, ADAM_MV_TOL, of the tensor's peak magnitude
CFG = (1e-3, 0.9, 0.999, 1e-8, 3, 0.5)
KEEP = float(np.float32(0.99))
FLAT_N = 10007                  # tests/test_gpu_guard_dense.py's dd_adam_step case: 2501 vectors (ten workgroups) and a 3-element tail
MULTI_SIZES = [1, 3, 32, 255, 256, 257, 864, 4097] + [7 + i for i in range(50)]      # 58 tensors: the 48-tensor table is crossed
DECAY_SIZES = (FLAT_N, 3)       # ... and a tail alone
SCALE_FORMS = ("value", "dev")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import adamw
    adamw.lib()
    return torch.device("cuda:0")


def pgmv(n, salt):
    rs = np.random.RandomState(1000 + salt)
    f = lambda lo, hi: torch.from_numpy(rs.uniform(lo, hi, n).astype(np.float32))
    return f(-1.0, 1.0), f(-0.1, 0.1), f(-0.05, 0.05), f(1e-4, 1e-2)


def reference(p, g, m, v, keep):
    """(p, m, v) of tests/_adamw_ref.py's fp64 reference as torch fp64."""
    p1, M, V, U, _ = ref.adamw64(p.numpy(), g.numpy(), m.numpy(), v.numpy(), *CFG, keep=np.float32(keep))
    return torch.from_numpy(p1.astype(np.float64) + U), torch.from_numpy(M), torch.from_numpy(V)


CASES = []


def _flat(form):
    def fn(arena, mode):
        from driving_dirty_amd import adamw
        lr, b1, b2, eps, step, gs = CFG
        p0, g0, m0, v0 = pgmv(FLAT_N, 0)
        p, g, m, v = arena.inout(p0, 16, "p"), arena.put(g0, 16, "g"), arena.inout(m0, 16, "m"), arena.inout(v0, 16, "v")
        sc = arena.put(torch.tensor([gs]), 4, "grad_scale_dev") if form == "dev" else None
        adamw.launch("dd_adamw_step", p, g, m, v, FLAT_N, lr, b1, b2, eps, step, 0.0 if form == "dev" else gs, sc, KEEP)
        outs = arena.verify()
        pr, mr, vr = reference(p0, g0, m0, v0, KEEP)
        return [Check("p", outs["p"], pr, P_TOL), Check("m", outs["m"], mr, MV_TOL), Check("v", outs["v"], vr, MV_TOL)]
    return fn


def _multi(form):
    def fn(arena, mode):
        from driving_dirty_amd import adamw
        lr, b1, b2, eps, step, gs = CFG
        host = [pgmv(n, 1 + i) for i, n in enumerate(MULTI_SIZES)]
        keeps = [1.0 if i % 3 == 0 else KEEP for i in range(len(host))]
        quads = [(arena.inout(p, 4, f"p{i}"), arena.put(g, 4, f"g{i}"), arena.inout(m, 4, f"m{i}"), arena.inout(v, 4, f"v{i}"))
                 for i, (p, g, m, v) in enumerate(host)]
        sc = arena.put(torch.tensor([gs]), 4, "grad_scale_dev") if form == "dev" else None
        adamw.launch("dd_adamw_step_multi", adam_table(quads), (C.c_float * len(keeps))(*keeps), len(quads), lr, b1, b2, eps, step,
                     0.0 if form == "dev" else gs, sc)
        outs = arena.verify()
        refs = [reference(*q, k) for q, k in zip(host, keeps)]
        cat = lambda key: torch.cat([outs[f"{key}{i}"] for i in range(len(host))])
        return [Check("p", cat("p"), torch.cat([r[0] for r in refs]), P_TOL), Check("m", cat("m"), torch.cat([r[1] for r in refs]), MV_TOL),
                Check("v", cat("v"), torch.cat([r[2] for r in refs]), MV_TOL)]
    return fn


def _decay(n):
    def fn(arena, mode):
        from driving_dirty_amd import adamw
        p0 = pgmv(n, 99)[0]
        p = arena.inout(p0, 16, "p")
        adamw.launch("dd_decay", p, n, KEEP)
        outs = arena.verify()
        return [Check("p", outs["p"], torch.from_numpy(ref.decayed(p0.numpy(), KEEP)), how="exact")]
    return fn


for _form in SCALE_FORMS:
    CASES.append(Case(f"dd_adamw_step[n={FLAT_N},scale={_form}]", "dd_adamw_step", _flat(_form)))
    CASES.append(Case(f"dd_adamw_step_multi[{len(MULTI_SIZES)} tensors,scale={_form}]", "dd_adamw_step_multi", _multi(_form), capacity=24 << 20))
for _n in DECAY_SIZES:
    CASES.append(Case(f"dd_decay[n={_n}]", "dd_decay", _decay(_n)))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
