"""Guard-band cases (tests/_guard.py) for the launch functions of include/dd_rm_loss.h (csrc/libdd_rm_loss.so): every operand of one
call -- each per-sample mask of a pointer table an operand of its own -- with 64 KiB of 0xFF around it, at the alignment the header
states and no more (16 bytes for fp32, 4 for a byte mask, 8 for stats and the workspace, 4 for loss_out).  Nothing is written outside
probs, dlogits, stats, coef, loss_out and the workspace, and the workspace is exactly the bytes the header's formula gives.  What a
case asserts: tests/test_gpu_guard_dense.py.

The shape is (3, CHUNK + 4): a whole piece and a ragged one of a single vector per sample, sample 1 with an empty target and sample 2
a full one.  No launcher picks a kernel by alignment, so the two modes are compared bit for bit.  The last test here
checks, without a GPU, that every function of the header is the subject of a case.

An over-read whose value is discarded cannot be seen by these tests."""
import numpy as np
import pytest
import torch

import _rm_loss_ref as ref
from _guard import Case, Check, ptr_table, run_case

SHAPE = (3, ref.CHUNK + 4)
SETTING = ("auto", 0.7, 1.3, 1.0)      # pos_weight, bce_weight, ts_weight, ts_eps
GRAD_SCALE = 2.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import rm_loss
    rm_loss.lib()
    return torch.device("cuda:0")


CASES = []


def _target(arena, t, form):
    """The target's operands in the arena -> (entry point suffix, operands that describe it)."""
    if form == "f32":
        return "", (arena.put(t, 16, "target"), 0)
    if form == "u8":
        return "", (arena.put(t.to(torch.uint8), 4, "target"), 1)
    return "_u8_ptrs", (ptr_table([arena.put(row.to(torch.uint8), 4, f"mask{i}") for i, row in enumerate(t)]),)


def _fwd(form):
    def fn(arena, mode):
        from driving_dirty_amd import rm_loss
        z, t = ref.case(SHAPE)
        b, per = SHAPE
        w, alpha, beta, eps = SETTING
        logits = arena.put(z, 16, "logits")
        suffix, described = _target(arena, t, form)
        probs, loss = arena.out((b, per), torch.float32, 16, "probs"), arena.out(3, torch.float32, 4, "loss_out")
        stats, coef = arena.out((b, 5), torch.float64, 8, "stats"), arena.out((b, 4), torch.float32, 16, "coef")
        nbytes = rm_loss.workspace_bytes(b, per)
        ws = arena.workspace(nbytes, 8)
        rm_loss.launch("dd_rm_loss_fwd" + suffix, logits, *described, b, per, rm_loss.POS_WEIGHT_AUTO, alpha, beta, eps, probs, loss, stats, coef,
                       ws, nbytes)
        outs = arena.verify()
        want = ref.loss_and_grad(z, t, w, alpha, beta, eps)[:3]
        for got, r, bound in zip(outs["loss_out"].tolist(), want, ref.loss_bounds(z, t, w, alpha, beta, eps)):
            assert abs(got - float(r)) <= bound, (form, mode, got, float(r), bound)
        err, bound = (outs["stats"].numpy() - ref.stats(z, t).numpy()), ref.stat_bounds(z, t)
        assert bool((np.abs(err) <= bound).all()), (form, mode, err, bound)
        return [Check("probs", outs["probs"], torch.sigmoid(z.double()), 1e-6), Check("loss_out", outs["loss_out"], outs["loss_out"], how="asserted"),
                Check("stats", outs["stats"], outs["stats"], how="asserted"), Check("coef", outs["coef"], outs["coef"], how="asserted")]
    return fn


def _bwd(form):
    def fn(arena, mode):
        from driving_dirty_amd import rm_loss
        z, t = ref.case(SHAPE)
        b, per = SHAPE
        p = torch.sigmoid(z)                                                     # any probabilities serve; these are fp32 values
        c = (torch.tensor([[3e-5, 1e-5, 2e-5, 4e-5]]) * torch.tensor([[1.0], [0.5], [2.0]])).float()      # [3, 4], a row per sample
        probs, coef = arena.put(p, 16, "probs"), arena.put(c, 16, "coef")
        suffix, described = _target(arena, t, form)
        dz = arena.out((b, per), torch.float32, 16, "dlogits")
        rm_loss.launch("dd_rm_loss_bwd" + suffix, probs, *described, b, per, coef, GRAD_SCALE, dz)
        outs = arena.verify()
        pd, td, cd = p.double(), t.double(), c.double() * GRAD_SCALE
        c0, c1, c2, c3 = (cd[:, k:k + 1] for k in range(4))
        want = c1 * (1 - td) * pd - c0 * td * (1 - pd) + pd * (1 - pd) * (c3 * (1 - td) - c2 * td)      # the header's formula
        assert ref.grad_excess(outs["dlogits"], want) <= ref.GRAD_OF_PEAK
        return [Check("dlogits", outs["dlogits"], want, ref.GRAD_OF_PEAK)]
    return fn


for _form in ("f32", "u8"):
    CASES.append(Case(f"dd_rm_loss_fwd[{_form}]", "dd_rm_loss_fwd", _fwd(_form)))
    CASES.append(Case(f"dd_rm_loss_bwd[{_form}]", "dd_rm_loss_bwd", _bwd(_form)))
CASES.append(Case("dd_rm_loss_fwd_u8_ptrs[3 masks]", "dd_rm_loss_fwd_u8_ptrs", _fwd("ptrs")))
CASES.append(Case("dd_rm_loss_bwd_u8_ptrs[3 masks]", "dd_rm_loss_bwd_u8_ptrs", _bwd("ptrs")))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)


def test_every_launch_function_of_the_library_has_a_guard_case():
    """The census of tests/test_guard_arena.py for this library: this module imports without a GPU, names only launch functions of
    dd_rm_loss.h, and every one of them is the subject of a case.  None picks a kernel by alignment."""
    from driving_dirty_amd import rm_loss
    assert CASES and len({c.name for c in CASES}) == len(CASES)
    assert {e for c in CASES for e in c.entry} == set(rm_loss.STREAMED) == set(rm_loss.SIGNATURES)
    assert not any(c.picks_kernel_by_alignment or c.crosses for c in CASES)
    for entry in rm_loss.STREAMED:
        assert sum(1 for c in CASES if c.entry == (entry,)) >= 1, entry
