"""Guard-band cases (tests/_guard.py) for the launch functions of include/dd_ema.h (csrc/libdd_ema.so): every tensor of both tables an
operand of its own with 64 KiB of 0xFF around it, at the 16-byte alignment the header states and no more.  What a case asserts:
tests/test_gpu_guard_dense.py.

Neither launcher picks a kernel by alignment (there is one kernel per function), so the two modes are compared bit for bit.  The
tables: (5,) one vector and a one-element tail, (CHUNK+1,) a whole piece and a piece that is only a tail, (3, 4, 1) three tensors
with a tail alone, a vector alone and a single element.  tests/test_ema_surface.py checks, without a GPU, that every function of the
header is the subject of a case here.

An over-read whose value is discarded cannot be seen by these tests."""
import pytest
import torch

import _ema_ref as ref
from _guard import Case, Check, run_case

pytestmark = pytest.mark.gpu

TABLES = ("5", "CHUNK+1", "3,4,1")
ALPHA = 0.1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import ema
    ema.lib()
    return torch.device("cuda:0")


def counts_of(table):
    from driving_dirty_amd import ema
    return {"5": (5,), "CHUNK+1": (ema.CHUNK + 1,), "3,4,1": (3, 4, 1)}[table]


CASES = []


def _split(t, counts):
    return list(torch.split(t, list(counts)))


def _case(entry, table):
    def fn(arena, mode):
        from driving_dirty_amd import ema
        counts = counts_of(table)
        e0, w0 = ref.pair(sum(counts), "guard" + table)
        if entry == "dd_ema_update_ptrs":
            es = [arena.inout(t, 16, f"e{i}") for i, t in enumerate(_split(e0, counts))]
            ws = [arena.put(t, 16, f"w{i}") for i, t in enumerate(_split(w0, counts))]
            ema.launch(entry, *ema.pointer_tables(es, ws), ALPHA)
            outs = arena.verify()
            got = torch.cat([outs[f"e{i}"] for i in range(len(counts))])
            ref.assert_within(got, ref.update(e0, w0, ALPHA), ref.one_step_bound(ref.magnitude(e0, w0)), f"{entry}[{table}] {mode}")
            return [Check("e", got, got, how="asserted")]
        a = [arena.inout(t, 16, f"a{i}") for i, t in enumerate(_split(e0, counts))]
        b = [arena.inout(t, 16, f"b{i}") for i, t in enumerate(_split(w0, counts))]
        ema.launch(entry, *ema.pointer_tables(a, b))
        outs = arena.verify()
        return [Check("a", torch.cat([outs[f"a{i}"] for i in range(len(counts))]), w0, how="exact"),
                Check("b", torch.cat([outs[f"b{i}"] for i in range(len(counts))]), e0, how="exact")]
    return fn


for _entry in ("dd_ema_update_ptrs", "dd_ema_swap_ptrs"):
    for _table in TABLES:
        CASES.append(Case(f"{_entry}[{_table}]", _entry, _case(_entry, _table)))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
