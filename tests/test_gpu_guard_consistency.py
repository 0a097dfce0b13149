"""Guard-band cases (tests/_guard.py) for the launch functions of include/dd_consistency.h (csrc/libdd_consistency.so): every operand of
one call with 64 KiB of 0xFF around it, at the alignment the header states and no more (4 bytes for a, m, da, dm and loss, 8 for stats
and the workspace).  Nothing is written outside da, dm, loss, stats and the workspace, and the workspace is exactly the bytes the
header's formula gives.  What a case asserts: tests/test_gpu_guard_dense.py.

The shapes: (3,5,6) and (1,7,5), whose w % 4 != 0 takes the 4-byte path at either alignment, and the piece-boundary shapes (2,1,CHUNK+4)
and (2,2,CHUNK/2+4), for which the launcher picks its kernel by the alignment -- 16-byte accesses in the natural mode, 4-byte ones in
the minimal mode, where every fp32 operand sits 4 bytes past a 256-byte boundary.  Both kernels give an element to the same lane in the
same order, so these cases keep the bit-for-bit comparison of the two modes (``crosses``).  The last test here checks, without a GPU,
that every function of the header is the subject of a case.

An over-read whose value is discarded cannot be seen by these tests."""
import pytest
import torch

import _consistency_ref as ref
from _guard import Case, Check, run_case

SCALAR_SHAPES = [(3, 5, 6), (1, 7, 5)]
BOUNDARY_SHAPES = [(2, 1, ref.CHUNK + 4), (2, 2, ref.CHUNK // 2 + 4)]
GRAD_SCALE = 2.0
ALIGNMENT_PICKS = {"dd_cons_fwd": "w % 4 == 0 and a, m 16-byte aligned", "dd_cons_fwd_grad": "w % 4 == 0 and a, m, da, dm 16-byte aligned"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import consistency
    consistency.lib()
    return torch.device("cuda:0")


CASES = []


def _case(shape, grad):
    def fn(arena, mode):
        from driving_dirty_amd import consistency
        a_cpu, m_cpu = ref.inputs(shape, salt=7)
        b, h, w = shape
        a, m = arena.put(a_cpu, 4, "a"), arena.put(m_cpu, 4, "m")
        if grad:
            da, dm = arena.out(shape, torch.float32, 4, "da"), arena.out(shape, torch.float32, 4, "dm")
        loss, stats = arena.out(1, torch.float32, 4, "loss"), arena.out((b, 2), torch.float64, 8, "stats")
        nbytes = consistency.workspace_bytes(b, h * w)
        ws = arena.workspace(nbytes, 8)
        if w % 4 == 0:      # the launcher's predicate: the two modes run its two kernels
            assert (a.data_ptr() % 16 == 0 and m.data_ptr() % 16 == 0) == (mode == "natural")
        if grad:
            consistency.launch("dd_cons_fwd_grad", a, m, b, h, w, GRAD_SCALE, da, dm, loss, stats, ws, nbytes)
        else:
            consistency.launch("dd_cons_fwd", a, m, b, h, w, loss, stats, ws, nbytes)
        outs = arena.verify()
        w_loss, w_stats, w_da, w_dm = ref.loss_and_grad(a_cpu, m_cpu, GRAD_SCALE)
        # fresh unit-stride copies of the two columns (also for B = 1): the comparison of the two modes views a result as bytes
        q, d = (outs["stats"][:, k].clone(memory_format=torch.contiguous_format) for k in range(2))
        checks = [Check("loss", outs["loss"].reshape(()), w_loss, ref.LOSS_REL, how="scalar"),
                  Check("Q", q, w_stats[:, 0], ref.LOSS_REL), Check("D", d, w_stats[:, 1], how="exact")]
        if grad:
            checks += [Check("da", outs["da"], w_da, ref.GRAD_OF_PEAK), Check("dm", outs["dm"], w_dm, ref.GRAD_OF_PEAK)]
        return checks
    return fn


for _shape in SCALAR_SHAPES + BOUNDARY_SHAPES:
    for _entry, _grad in (("dd_cons_fwd", False), ("dd_cons_fwd_grad", True)):
        CASES.append(Case(f"{_entry}{list(_shape)}", _entry, _case(_shape, _grad), crosses=(_entry,) if _shape in BOUNDARY_SHAPES else None))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)


@pytest.mark.gpu
def test_a_workspace_one_byte_short_is_refused_on_the_host(dev):
    from driving_dirty_amd import consistency
    b, h, w = BOUNDARY_SHAPES[0]
    a, m = (t.to(dev) for t in ref.inputs((b, h, w), salt=7))
    loss, stats = torch.full((1,), -1.0, device=dev), torch.full((b, 2), -1.0, device=dev, dtype=torch.float64)
    da, dm = torch.full_like(a, -1.0), torch.full_like(m, -1.0)
    nbytes = consistency.workspace_bytes(b, h * w)
    ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    with pytest.raises(consistency.HotpathError, match=f"workspace_bytes = {nbytes - 1}"):
        consistency.launch("dd_cons_fwd", a, m, b, h, w, loss, stats, ws, nbytes - 1)
    with pytest.raises(consistency.HotpathError, match=f"workspace_bytes = {nbytes - 1}"):
        consistency.launch("dd_cons_fwd_grad", a, m, b, h, w, 1.0, da, dm, loss, stats, ws, nbytes - 1)
    torch.cuda.synchronize()
    assert float(loss) == -1.0 and bool((stats == -1).all()) and bool((da == -1).all()) and bool((dm == -1).all()), "nothing was launched"
    consistency.launch("dd_cons_fwd", a, m, b, h, w, loss, stats, ws, nbytes)
    assert float(loss) > 0


def test_every_launch_function_of_the_library_has_a_guard_case():
    """The census of tests/test_guard_arena.py for this library: this module imports without a GPU, names only launch functions of
    dd_consistency.h, and every one of them is the subject of a case on both paths; the cases that cross the launcher's alignment pick
    are the ones ALIGNMENT_PICKS lists."""
    from driving_dirty_amd import consistency
    assert CASES and len({c.name for c in CASES}) == len(CASES)
    assert {e for c in CASES for e in c.entry} == set(consistency.STREAMED) == set(consistency.SIGNATURES)
    assert not any(c.picks_kernel_by_alignment for c in CASES), "every case keeps the bit-for-bit comparison of the two modes"
    assert {e for c in CASES for e in c.crosses} == set(ALIGNMENT_PICKS)
    for entry in consistency.STREAMED:
        assert sum(1 for c in CASES if c.entry == (entry,) and c.crosses) >= 1 and sum(1 for c in CASES if c.entry == (entry,) and not c.crosses) >= 1, entry
    assert all(w % 4 for _, _, w in SCALAR_SHAPES) and all(w % 4 == 0 and h * w > ref.CHUNK for _, h, w in BOUNDARY_SHAPES)
