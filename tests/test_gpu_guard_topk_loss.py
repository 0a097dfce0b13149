"""Guard-band cases (tests/_guard.py) for the launch functions of include/dd_topk_loss.h (csrc/libdd_topk_loss.so): every operand of one
call with 64 KiB of 0xFF around it, at the alignment the header states and no more (16 bytes for logits, probs and dlogits, 4 for a byte
mask and loss_out, 8 for stats and the workspace).  Nothing is written outside probs, dlogits, loss_out, stats and the workspace, the
workspace is exactly the bytes the header's formula gives, and -- left 0xFF -- nothing of it is read before the call has written it: a
count added onto an unzeroed histogram or a state block read too early would move n_b and tau_b, which are held exactly.

The shapes: (3, 8), and the piece-boundary shapes (2, CHUNK + 4) and (2, 2 CHUNK - 4); keep below per_sample (the selection runs) and
equal to it (the selection is skipped, the histograms stay untouched).  The launcher picks no kernel by alignment: the two modes are
compared bit for bit.  The last test here checks, without a GPU, that every function of the header is the subject of a case.

An over-read whose value is discarded cannot be seen by these tests."""
import pytest
import torch

import _topk_loss_ref as ref
from _guard import Case, Check, ptr_table, run_case

SHAPES = [(3, 8), (2, ref.CHUNK + 4), (2, 2 * ref.CHUNK - 4)]
GRAD_SCALE = 2.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import topk_loss
    topk_loss.lib()
    return torch.device("cuda:0")


CASES = []


def _case(shape, keep, table, grad):
    def fn(arena, mode):
        from driving_dirty_amd import topk_loss
        z_cpu, t_cpu = ref.logits_and_target(shape, salt=11)
        b, per = shape
        z = arena.put(z_cpu, 16, "logits")
        if table:
            masks = [arena.put(t_cpu[i], 4, f"mask{i}") for i in range(b)]
            target = ptr_table(masks)
        else:
            target = arena.put(t_cpu, 4, "target")
        probs = arena.out(shape, torch.float32, 16, "probs")
        dz = arena.out(shape, torch.float32, 16, "dlogits") if grad else None
        loss, stats = arena.out(2, torch.float32, 4, "loss_out"), arena.out((b, 4), torch.float64, 8, "stats")
        nbytes = topk_loss.workspace_bytes(b, per)
        assert nbytes == ref.header_workspace_bytes(b, per)
        ws = arena.workspace(nbytes, 8)
        topk_loss.launch("dd_topk_bce_u8_ptrs" if table else "dd_topk_bce", z, target, b, per, keep, GRAD_SCALE, probs, dz, loss, stats, ws, nbytes)
        outs = arena.verify()
        w_loss, w_all, w_stats, w_dz, _ = ref.loss_and_grad(z_cpu, t_cpu, keep, GRAD_SCALE)
        col = [outs["stats"][:, k].clone(memory_format=torch.contiguous_format) for k in range(4)]
        checks = [Check("loss", outs["loss_out"][0].reshape(()), w_loss, ref.LOSS_REL, how="scalar"),
                  Check("L_all", outs["loss_out"][1].reshape(()), w_all, ref.LOSS_REL, how="scalar"),
                  Check("n", col[0], w_stats[:, 0], how="exact"), Check("sum_sel", col[1], w_stats[:, 1], ref.LOSS_REL),
                  Check("tau", col[2], w_stats[:, 2], how="exact"), Check("sum_all", col[3], w_stats[:, 3], ref.LOSS_REL),
                  Check("probs", outs["probs"], torch.sigmoid(z_cpu.double()), 1e-6, how="abs")]
        if grad:
            checks.append(Check("dlogits", outs["dlogits"], w_dz, ref.GRAD_OF_PEAK))
        return checks
    return fn


for _shape in SHAPES:
    for _table in (False, True):
        _entry = "dd_topk_bce_u8_ptrs" if _table else "dd_topk_bce"
        for _keep, _grad in ((max(1, _shape[1] // 4), True), (_shape[1], True), (3, False)):
            CASES.append(Case(f"{_entry}{list(_shape)}-K{_keep}{'' if _grad else '-nograd'}", _entry, _case(_shape, _keep, _table, _grad)))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)


@pytest.mark.gpu
def test_a_workspace_one_byte_short_is_refused_on_the_host(dev):
    from driving_dirty_amd import topk_loss
    b, per = SHAPES[1]
    z, t = (x.to(dev) for x in ref.logits_and_target((b, per), salt=11))
    loss, stats = torch.full((2,), -1.0, device=dev), torch.full((b, 4), -1.0, device=dev, dtype=torch.float64)
    probs, dz = torch.full_like(z, -1.0), torch.full_like(z, -1.0)
    nbytes = topk_loss.workspace_bytes(b, per)
    ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    masks = ptr_table([t[0], t[1]])
    for name, target in (("dd_topk_bce", t), ("dd_topk_bce_u8_ptrs", masks)):
        with pytest.raises(topk_loss.HotpathError, match=f"workspace_bytes = {nbytes - 1}"):
            topk_loss.launch(name, z, target, b, per, 5, 1.0, probs, dz, loss, stats, ws, nbytes - 1)
    torch.cuda.synchronize()
    assert bool((loss == -1).all()) and bool((stats == -1).all()) and bool((probs == -1).all()) and bool((dz == -1).all()), "nothing was launched"
    topk_loss.launch("dd_topk_bce", z, t, b, per, 5, 1.0, probs, dz, loss, stats, ws, nbytes)
    assert float(loss[0]) > 0


def test_every_launch_function_of_the_library_has_a_guard_case():
    """The census of tests/test_guard_arena.py for this library: this module imports without a GPU, names only launch functions of
    dd_topk_loss.h, and every one of them is the subject of a case with and without the selection and without the gradient."""
    from driving_dirty_amd import topk_loss
    assert CASES and len({c.name for c in CASES}) == len(CASES)
    assert {e for c in CASES for e in c.entry} == set(topk_loss.STREAMED) == set(topk_loss.SIGNATURES)
    assert not any(c.picks_kernel_by_alignment or c.crosses for c in CASES), "no launcher here picks a kernel by alignment"
    for entry in topk_loss.STREAMED:
        assert sum(1 for c in CASES if c.entry == (entry,)) == 3 * len(SHAPES), entry
    assert all(per % 4 == 0 for _, per in SHAPES) and sum(per > ref.CHUNK for _, per in SHAPES) == 2
