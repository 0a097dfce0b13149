"""Guard-band cases (tests/_guard.py) that REPLAY existing kernel-level tests with every device operand redirected into the arena:
the bf16 decoder kernels of csrc/decoder_bf16.hip (dd_dec_bf16_*) under tests/test_gpu_ae_bf16.py::test_dc1_against_oracle and
::test_dc3_dc4_against_oracle, and the component entry points of csrc/boxeval.hip that no test calls into a guarded buffer
(dd_label_components, dd_split_components, dd_labelled_boxes, dd_labelled_obb) under tests/test_gpu_box_eval.py and
tests/test_gpu_box_split.py.

The replayed test function runs unchanged -- its own fp64 oracle, its own bounds (bf16 ulps, 1e-4 of the sums, exact labels and
boxes, ULP_BOUND for oriented corners) -- while ``Redirect`` (tests/test_gpu_guard_gconv.py) stands in for the ``call`` of ops, ops_bf16
and gconv: each tensor a wrapper hands to an entry point is mirrored by an arena operand of the same size, inputs copied in,
outputs and workspaces left 0xFF (``boxes`` and ``moments``, which the entry points are documented to write only up to the count,
take over what the wrapper put there), at 16-byte alignment between 64 KiB guards.  Afterwards the mirrored outputs are handed
back, so the replayed assertions judge what the kernels wrote into the arena; the case itself adds the arena's checks and the
bit-for-bit comparison of every mirrored output across the two alignments.

An over-read whose value is discarded cannot be seen by these tests.

Run time on an MI355X: see tests/test_gpu_guard_layout.py (the guard files are timed together)."""
import pytest
import torch

from _guard import Case, Check, run_case
from test_gpu_guard_gconv import Redirect

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class Deferred(Redirect):
    """The replayed tests read results between calls (``.cpu()``, ``torch.equal``), so the mirrored outputs are handed back after
    every call, not only at the end; ``verify()`` still runs once, after the last one."""

    def __call__(self, name, *operands):
        super().__call__(name, *operands)
        for view, orig, label, const in self.mirrors.values():
            if not const and view.dtype == orig.dtype and tuple(view.shape) == tuple(orig.shape):
                orig.copy_(view)


def _replay(tests, want, inout=()):
    """tests: [(module name, function name, arguments after ``dev``)]."""
    def fn(arena, mode):
        import importlib

        from driving_dirty_amd import gconv, ops, ops_bf16
        red = Deferred(arena, inout=inout)
        mods = (ops, ops_bf16, gconv)
        real = [m.call for m in mods]
        for m in mods:
            m.call = red
        try:
            for mod, func, args in tests:
                getattr(importlib.import_module(mod), func)(arena.dev, *args)
        finally:
            for m, r in zip(mods, real):
                m.call = r
        outs = red.finish()
        assert set(want) <= set(red.called), sorted(set(want) - set(red.called))
        # held to their references by the replayed assertions above; listed for the comparison of the two alignments
        return [Check(label, outs[label], outs[label], how="asserted") for _, _, label, const in red.mirrors.values() if label in outs]
    return fn


DEC = ("dd_dec_bf16_split64", "dd_dec_bf16_merge64", "dd_dec_bf16_dc1_fwd", "dd_dec_bf16_dc34_fwd", "dd_dec_bf16_dc4_bwd",
       "dd_dec_bf16_dc3_dgrad", "dd_dec_bf16_dc3_wgrad")
COMPONENTS = ("dd_label_components", "dd_split_components", "dd_labelled_boxes", "dd_labelled_obb")

CASES = []
for _shape in ((1, 1, 1), (3, 5, 7), (2, 13, 37)):      # tests/test_gpu_ae_bf16.py::SHAPES: one pixel, odd sizes, more than one tile row
    CASES.append(Case(f"dd_dec_bf16[{_shape}]", DEC, _replay(
        [("test_gpu_ae_bf16", "test_dc1_against_oracle", (_shape,)), ("test_gpu_ae_bf16", "test_dc3_dc4_against_oracle", (_shape,))], DEC),
        capacity=256 << 20))
for _name, _r, _g in (("hand", 2, 4), ("0.6", 1, 2)):
    CASES.append(Case(f"components[{_name},split_px={_r},grow={_g}]", COMPONENTS, _replay(
        [("test_gpu_box_eval", "test_labels_of_components_that_straddle_tile_corners", ()),
         ("test_gpu_box_split", "test_labelled_fits_of_plain_components_are_the_component_fits", ()),
         ("test_gpu_box_split", "test_boxes_from_split_labels_equal_the_reference", (_name, _r, _g))], COMPONENTS, inout=("boxes", "moments")),
        capacity=256 << 20))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_guard(dev, c):
    run_case(c, dev)
