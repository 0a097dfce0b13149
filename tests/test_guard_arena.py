"""The guard arena of tests/_guard.py can fail: planted faults on CPU tensors, with a fake two-stage "kernel" written in torch.

The fake kernel is y = 2 x and loss = sum x^2 through a workspace of ROWS fp64 partial sums -- the shape of the library's two-stage
reductions.  A correct one passes in both alignment modes; each planted fault makes ``verify()`` raise a GuardError that names the
operand, the kind of damage and where it is."""
import pytest
import torch

from _guard import GAP, MODES, Arena, Case, Check, GuardError, run_case

N, ROWS = 1027, 8


def build(mode):
    arena = Arena("cpu", mode, capacity=1 << 20)
    x_cpu = torch.linspace(-1.0, 1.0, N)
    ops = {"x": arena.put(x_cpu, 16, "x"),
           "scale": arena.put(torch.tensor([2.0]), 4, "scale"),
           "y": arena.out((N,), torch.float32, 16, "y"),
           "loss": arena.out((1,), torch.float64, 8, "loss"),
           "ws": arena.workspace(ROWS * 8, 16, "workspace"),
           "count": arena.inout(torch.tensor([3], dtype=torch.int64), 8, "count")}
    return arena, x_cpu, ops


def fake_kernel(o, fault=None):
    x, y, part = o["x"], o["y"], o["ws"].view(torch.float64)
    y.copy_(x * o["scale"])
    rows = ROWS - 1 if fault == "row_unwritten" else ROWS
    for r in range(rows):
        s = (x[r::ROWS].double() ** 2).sum()
        if fault == "accumulate":
            part[r] += s          # a store that is an accumulate: fine on zeroed memory, NaN on 0xFF
        else:
            part[r] = s
    o["loss"][0] = part.sum()
    o["count"] += 1


@pytest.mark.parametrize("mode", MODES)
def test_correct_kernel_passes(mode):
    arena, x_cpu, o = build(mode)
    fake_kernel(o)
    outs = arena.verify()
    assert set(outs) == {"y", "loss", "count"}
    assert torch.equal(outs["y"], 2 * x_cpu) and int(outs["count"]) == 4
    assert abs(float(outs["loss"]) - float((x_cpu.double() ** 2).sum())) < 1e-9


@pytest.mark.parametrize("mode", MODES)
def test_layout(mode):
    """Addresses: 0 (natural) or the operand's own alignment (minimal) modulo 256; every gap at least 64 KiB and all 0xFF; an output
    and a workspace are left 0xFF; the workspace holds exactly the bytes asked for."""
    arena, x_cpu, o = build(mode)
    aligns = {"x": 16, "scale": 4, "y": 16, "loss": 8, "workspace": 16, "count": 8}
    for name, align in aligns.items():
        assert arena.address(name) % 256 == (0 if mode == "natural" else align), name
        front, behind = arena.gaps(name)
        assert GAP == 64 * 1024 and GAP <= front < GAP + 256 and GAP <= behind < GAP + 256, (name, front, behind)
    assert o["x"].data_ptr() == arena.address("x") and o["y"].data_ptr() == arena.address("y")
    assert o["ws"].numel() == ROWS * 8 and o["ws"].dtype == torch.uint8
    assert bool((o["ws"] == 0xFF).all()) and bool(torch.isnan(o["y"]).all()) and bool(torch.isnan(o["loss"]).all())
    payload = sum(op.nbytes for op in arena.operands)
    first, last = arena.operands[0], arena.operands[-1]
    span = arena.buf[first.start - GAP:last.start + last.nbytes + GAP]
    assert int((span == 0xFF).sum()) >= span.numel() - payload      # everything between the payloads is fill
    torch.testing.assert_close(o["x"], x_cpu, rtol=0, atol=0)


def raises(arena, operand, what):
    with pytest.raises(GuardError) as e:
        arena.verify()
    assert (e.value.operand, e.value.what) == (operand, what), str(e.value)
    assert operand in str(e.value)
    return e.value


@pytest.mark.parametrize("mode", MODES)
def test_one_byte_behind_an_output(mode):
    arena, _, o = build(mode)
    fake_kernel(o)
    y = arena._find("y")
    arena.buf[y.start + y.nbytes] = 0
    assert raises(arena, "y", "behind").offset == 0
    arena.buf[y.start + y.nbytes] = 0xFF
    arena.buf[y.start + y.nbytes + 4099] = 7       # a stray store a tile row further on
    assert raises(arena, "y", "behind").offset == 4099


@pytest.mark.parametrize("mode", MODES)
def test_one_byte_in_front_of_an_output(mode):
    arena, _, o = build(mode)
    fake_kernel(o)
    y = arena._find("y")
    arena.buf[y.start - 1] = 0
    assert raises(arena, "y", "front").offset == -1
    # the first operand's front gap and the last operand's back gap are watched too
    arena.buf[y.start - 1] = 0xFF
    arena.buf[arena._find("x").start - GAP] = 1
    assert raises(arena, "x", "front").offset == -GAP
    arena.buf[arena._find("x").start - GAP] = 0xFF
    c = arena._find("count")
    arena.buf[c.start + c.nbytes + GAP - 1] = 1
    assert raises(arena, "count", "behind").offset == GAP - 1


@pytest.mark.parametrize("mode", MODES)
def test_an_input_element_changed(mode):
    arena, _, o = build(mode)
    fake_kernel(o)
    o["x"][513] = 0.25
    assert raises(arena, "x", "input").offset == 513
    arena, _, o = build(mode)
    fake_kernel(o)
    o["scale"][0] = -2.0
    raises(arena, "scale", "input")


@pytest.mark.parametrize("mode", MODES)
def test_a_value_read_from_the_gap_reaches_the_output(mode):
    """An n % 4 tail that loads a whole vector: the element past the input is the gap's 0xFFFFFFFF, a NaN."""
    arena, _, o = build(mode)
    fake_kernel(o)
    x = arena._find("x")
    past = arena.buf[x.start:x.start + x.nbytes + 4].view(torch.float32)      # x and one element more
    o["y"][N - 1] = past[N] * 2.0
    assert raises(arena, "y", "nonfinite").offset == N - 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fault", ["accumulate", "row_unwritten"])
def test_workspace_accumulated_onto_or_left_unwritten(mode, fault):
    """A partial-sum row that is added to instead of stored, or that the grid never reaches: right on fresh (zero) memory, NaN in
    the result here."""
    arena, _, o = build(mode)
    fake_kernel(o, fault)
    raises(arena, "loss", "nonfinite")


def test_an_unwritten_output_is_caught_and_operand_names_are_unique():
    arena, _, o = build("minimal")
    fake_kernel(o)
    o["y"][5:9] = float("nan")
    assert raises(arena, "y", "nonfinite").offset == 5
    with pytest.raises(AssertionError):
        arena.put(torch.zeros(4), 16, "x")
    with pytest.raises(ValueError):
        arena.workspace(2 << 20, 16, "too_big")


GUARD_MODULES = ("test_gpu_guard_dense", "test_gpu_guard_layout", "test_gpu_guard_conv", "test_gpu_guard_heads", "test_gpu_guard_bf16",
                 "test_gpu_guard_gconv", "test_gpu_guard_rm", "test_gpu_guard_replay")

# Launch functions that an existing test already runs, by a direct call, into a buffer with a sentinel-filled guard behind it.
GUARDED_ELSEWHERE = {
    **{n: "tests/test_gpu_batch_boundaries.py::test_fp32_sample_gathers" for n in (
        "dd_stitch6_ptrs", "dd_stitch6_bf16_ptrs", "dd_stitch6_bf16_ptrs_masked", "dd_view_to_nhwc4_ptrs")},
    **{n: "tests/test_gpu_batch_boundaries.py::test_uint8_frame_gathers" for n in (
        "dd_stitch6_u8_ptrs", "dd_stitch6_bf16_u8_ptrs", "dd_stitch6_bf16_u8_ptrs_masked", "dd_view_to_nhwc4_u8_ptrs")},
    "dd_subsample_nhwc4_u8_ptrs": "tests/test_gpu_batch_boundaries.py::test_road_mask_taps",
    "dd_boxes_to_binary_map": "tests/test_gpu_batch_boundaries.py::test_rasteriser_130_samples",
    "dd_box_iou_ats": "tests/test_gpu_batch_boundaries.py::test_iou_ats_130_samples",
    "dd_linear_sigmoid_gt": "tests/test_gpu_predict.py (_fused_guarded)",
    "dd_component_boxes": "tests/test_gpu_box_eval.py (guard region behind boxes)",
    "dd_component_obb": "tests/test_gpu_box_fit.py (guard regions behind boxes, moments and workspace)",
}
# The one launch function the issue exempts.
EXEMPT = {"dd_clock_probe"}


def _case_tables():
    import importlib
    return {mod: importlib.import_module(mod) for mod in GUARD_MODULES}


def test_the_case_tables_import_without_a_gpu_and_name_real_launch_functions():
    """Every case is about launch functions the header declares (a misspelt name would make a coverage claim empty), case names are
    unique, and every launcher listed as picking its kernel by alignment has a case whose two modes run its two kernels."""
    from driving_dirty_amd import _lib
    names = set()
    for mod, m in _case_tables().items():
        assert m.CASES, mod
        for c in m.CASES:
            assert c.name not in names, c.name
            names.add(c.name)
            assert c.entry and set(c.entry) <= _lib.STREAMED, (c.name, set(c.entry) - _lib.STREAMED)
            assert set(c.crosses) <= set(c.entry), c.name
        picks = set(getattr(m, "ALIGNMENT_PICKS", {}))
        crossed = {e for c in m.CASES for e in c.crosses}
        assert crossed == picks, (mod, crossed ^ picks)


def test_every_launch_function_is_accounted_for():
    """The launch functions of the header (the names of _lib.CALL_OPERANDS that take a stream) are, each exactly once: the subject
    of a guard case, guarded by an existing test (GUARDED_ELSEWHERE), or dd_clock_probe (a measurement aid; the dd_set_* / dd_get_*
    settings take no stream and are not launch functions).  A launch function added later without a guard case fails here."""
    from driving_dirty_amd import _lib
    launch = {n for n in _lib.CALL_OPERANDS if n in _lib.STREAMED}
    assert launch == set(_lib.STREAMED)
    covered = {e for m in _case_tables().values() for c in m.CASES for e in c.entry}
    groups = {"case": covered, "elsewhere": set(GUARDED_ELSEWHERE), "exempt": EXEMPT}
    for name, g in groups.items():
        assert g <= launch, (name, g - launch)
    keys = list(groups)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not (groups[a] & groups[b]), (a, b, groups[a] & groups[b])
    assert launch == set().union(*groups.values()), sorted(launch - set().union(*groups.values()))
    assert len(covered) == 125


def test_run_case_compares_the_two_modes_bit_for_bit():
    """run_case: a kernel whose result depends on the address (here: on the mode) fails unless the case says its launcher picks
    a kernel by alignment."""
    def fn(arena, mode):
        x = arena.put(torch.tensor([1.0, 2.0, 3.0, 4.0]), 16, "x")
        y = arena.out((4,), torch.float32, 16, "y")
        y.copy_(x * (1.0 if mode == "natural" else 1.0 + 2.0 ** -23))
        return [Check("y", arena.verify()["y"], torch.tensor([1.0, 2.0, 3.0, 4.0]), 1e-6)]
    with pytest.raises(AssertionError, match="differs between"):
        run_case(Case("addr", "dd_none", fn), "cpu")
    run_case(Case("addr", "dd_none", fn, picks_kernel_by_alignment=True), "cpu")
    with pytest.raises(AssertionError):
        run_case(Case("tol", "dd_none", lambda a, m: [Check("y", torch.tensor([1.001]), torch.tensor([1.0]), 1e-6)]), "cpu")
