"""Weight averaging without a GPU: include/dd_ema.h and the library built from it, the launchers' host-side refusals, the binder it
shares with the augmentation and the mirror averaging, the decay schedule as numbers, the command line, and TrainStep with it off."""
import ctypes as C
import math
import os
from argparse import ArgumentParser, Namespace

import pytest

from _surface import ROOT, exported_symbols, header, kernel_resources

FUNCTIONS = {"dd_ema_update_ptrs", "dd_ema_swap_ptrs"}


def models():
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    return BasicAE, RoadMapBCE, RoadMap, BBSpatialRoadMap, JointRoadMapBBox


def test_header_declares_the_two_launch_functions_and_the_library_exports_exactly_them():
    from driving_dirty_amd import build, ema
    signatures, streamed = header("dd_ema.h")
    assert set(signatures) == FUNCTIONS and set(streamed) == FUNCTIONS, "both are launch functions (void* stream last)"
    assert ema.SIGNATURES == signatures and ema.STREAMED == streamed
    assert ema.OPERANDS == {"dd_ema_update_ptrs": 5, "dd_ema_swap_ptrs": 4}
    assert os.path.exists(build.EXTENSIONS["ema"].lib), "build the HIP libraries first (python __graft_entry__.py)"
    assert {n for n in exported_symbols(build.EXTENSIONS["ema"].lib) if n.startswith("dd_")} == FUNCTIONS
    assert build.build(force=False, verbose=False) == build.LIB and not build.needs_build()


def test_the_constants_are_the_headers():
    from driving_dirty_amd import ema
    text = open(os.path.join(ROOT, "include", "dd_ema.h")).read()
    assert f"#define DD_EMA_CHUNK {ema.CHUNK}" in text and f"#define DD_EMA_TABLE_MAX {ema.TABLE_MAX}" in text
    assert ema.CHUNK % 1024 == 0 and ema.TABLE_MAX >= 1      # a piece is whole 16-byte vectors for 256 lanes


def test_one_binder_serves_the_three_extension_libraries():
    from driving_dirty_amd import _lib, augment, build, ema, tta
    for name in ("lib", "launch", "last_error"):
        fn = vars(ema)[name]      # module-level names, so that a monkeypatched ``launch`` takes effect
        assert isinstance(fn.__self__, _lib.Extension) and fn.__func__ is getattr(_lib.Extension, name)
        assert fn.__self__ is ema.lib.__self__
    assert ema.LIB == build.EXTENSIONS["ema"].lib and ema.SIGNATURES == header("dd_ema.h")[0]
    assert "call" not in vars(ema) and "size" not in vars(ema)
    assert ema.lib.__self__ is not augment.lib.__self__ and ema.lib.__self__ is not tta.lib.__self__
    assert ema.lib() is ema.lib()
    with pytest.raises(ema.HotpathError, match="operands given"):      # wrong operand count
        ema.launch("dd_ema_update_ptrs", None, None, None, 1)
    with pytest.raises(ema.HotpathError, match="operands given"):
        ema.launch("dd_ema_swap_ptrs", None, None, None, 1, 0.5)
    with pytest.raises(ema.HotpathError, match="not a function of include/dd_ema.h"):
        ema.launch("dd_tta_mean_prob", 1 << 20, 2 << 20, 3 << 20, 2, 4, 8, 0)


def test_the_kernels_use_no_scratch_no_lds_and_no_spills():
    from driving_dirty_amd import build
    ks = kernel_resources().kernels(build.EXTENSIONS["ema"].lib)
    assert len(ks) == 2, [k[".name"] for k in ks]      # one kernel per function: the whole table, every size
    for k in ks:
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, k[".name"]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k[".name"]


def test_launchers_refuse_bad_arguments_without_a_gpu():
    from driving_dirty_amd import ema
    lib = ema.lib()
    A, B = (1 << 20, 2 << 20, 3 << 20), (5 << 20, 6 << 20, 7 << 20)      # never dereferenced: every call below is refused on the host

    def ptrs(values):
        return (C.c_void_p * len(values))(*values)

    def counts(values):
        return (C.c_int64 * len(values))(*values)

    def refused(rc, *words):
        msg = ema.last_error()
        assert rc != 0 and msg and all(w in msg for w in words), (rc, msg)

    def update(a=A, b=B, n=(8, 5, 4096), tensors=3, alpha=0.5):
        return lib.dd_ema_update_ptrs(a and ptrs(a), b and ptrs(b), n and counts(n), tensors, alpha, None)

    def swap(a=A, b=B, n=(8, 5, 4096), tensors=3, alpha=None):
        return lib.dd_ema_swap_ptrs(a and ptrs(a), b and ptrs(b), n and counts(n), tensors, None)

    for fn, who, first, second in ((update, "ema_update_ptrs", "ema_ptrs", "param_ptrs"), (swap, "ema_swap_ptrs", "a_ptrs", "b_ptrs")):
        refused(fn(a=None), who, first, "NULL")                                   # a null table
        refused(fn(b=None), who, second, "NULL")
        refused(fn(n=None), who, "counts", "NULL")
        refused(fn(a=(A[0], None, A[2])), who, first + "[1]", "NULL")             # ... and a null entry
        refused(fn(b=(None,) + B[1:]), who, second + "[0]", "NULL")
        for bad in (0, -1):
            refused(fn(tensors=bad), who, "tensors", str(bad))
        refused(fn(n=(8, 0, 4096)), who, "counts[1]", "2^31")
        refused(fn(n=(8, 5, -4)), who, "counts[2]", "2^31")
        refused(fn(n=(1 << 31, 5, 4096)), who, "counts[0]", "2^31")               # exactly 2^31 elements
        refused(fn(n=(8, 5, 1 << 40)), who, "counts[2]", "2^31")
        refused(fn(a=(A[0], A[1] + 4, A[2])), who, first + "[1]", "16-byte")       # a misaligned pointer
        refused(fn(b=(B[0], B[1], B[2] + 8)), who, second + "[2]", "16-byte")
        refused(fn(b=(B[0], A[0], B[2])), who, first + "[0]", second + "[1]", "overlaps")      # the same buffer on both sides
        refused(fn(b=(A[2] + 4096 * 4 - 16, B[1], B[2])), who, first + "[2]", second + "[0]", "overlaps")      # begins inside the last 16 bytes
        refused(fn(a=(B[1] + 16, A[1], A[2])), who, first + "[0]", second + "[1]", "overlaps")                   # ... and the other way round
    for bad in (float("nan"), -0.001, 1.0001, float("inf"), -float("inf")):
        refused(update(alpha=bad), "ema_update_ptrs", "alpha", "[0, 1]")
    assert update(alpha=0.0) == 0      # every average keeps its bits: the operands are checked, nothing is launched


def test_the_decay_schedule_as_numbers():
    from driving_dirty_amd import ema
    d = 0.999
    assert ema.alpha_at(d, 1, 0) == 1.0 - d and ema.alpha_at(d, 4, 0) == 1.0 - d ** 4 and ema.alpha_at(d, 4, 123) == 1.0 - d ** 4
    for t, want in ((0, 1 / 10), (1, 2 / 11), (9, 10 / 19), (10_000, d)):
        assert ema.decay_at(d, t, warmup=True) == min(d, (1 + t) / (10 + t)) == want
        assert ema.alpha_at(d, 1, t, warmup=True) == 1.0 - want
        assert ema.alpha_at(d, 3, t, warmup=True) == 1.0 - want ** 3
        assert ema.decay_at(d, t) == d
    assert (1 + 8981) / (10 + 8981) < d < (1 + 8992) / (10 + 8992)      # where the warmup hands over to the decay
    assert math.isclose(ema.alpha_at(0.9, 2, 0), 0.19)


def test_the_parsers_take_the_three_flags_and_default_to_off():
    parsed = {}
    for cls in models():
        args = cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([])
        assert (args.ema_decay, args.ema_every, args.ema_warmup) == (0.0, 1, False), cls
        assert isinstance(args.ema_decay, float) and isinstance(args.ema_every, int)
        args = cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args(["--ema_decay", "0.999", "--ema_every", "4", "--ema_warmup"])
        assert (args.ema_decay, args.ema_every, args.ema_warmup) == (0.999, 4, True), cls
        parsed[cls.__name__] = set(vars(args))
    # the joint parser is still the union of the two single-task ones (tests/test_joint_surface.py)
    assert parsed["JointRoadMapBBox"] == (parsed["BBSpatialRoadMap"] | parsed["RoadMapBCE"] | {"box_rm_input"}) - {"unfreeze_epoch_no", "mse_loss"}


def test_train_step_with_averaging_off_holds_no_average():
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    from driving_dirty_amd.train import TrainStep
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))
    for extra in ({}, {"ema_decay": 0.0, "ema_every": 4, "ema_warmup": True}):
        model = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, **extra))
        step = TrainStep(model, scheduler=False, adam_overlap=False)
        assert step.ema is None
        with pytest.raises(RuntimeError, match="averaging is off"):
            step.averaged()
        step.close()
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match="ema_decay"):
            TrainStep(model, scheduler=False, adam_overlap=False, ema_decay=bad)
    with pytest.raises(_hotpath_error(), match="fc1.weight|parameter '"):      # on: the shadows live on the device, by name
        TrainStep(model, scheduler=False, adam_overlap=False, ema_decay=0.99)


def _hotpath_error():
    from driving_dirty_amd._lib import HotpathError
    return HotpathError


def test_every_launch_function_of_the_library_has_a_guard_case():
    """The census of tests/test_guard_arena.py for this library: the case table imports without a GPU, names only launch functions of
    dd_ema.h, and every one of them is the subject of a case.  Neither picks a kernel by alignment."""
    import test_gpu_guard_ema as guard
    from driving_dirty_amd import ema
    assert guard.CASES and len({c.name for c in guard.CASES}) == len(guard.CASES)
    assert {e for c in guard.CASES for e in c.entry} == set(ema.STREAMED) == set(ema.SIGNATURES)
    assert not any(c.picks_kernel_by_alignment or c.crosses for c in guard.CASES)
    for entry in ema.STREAMED:
        assert sum(1 for c in guard.CASES if c.entry == (entry,)) == len(guard.TABLES) == 3
    assert [guard.counts_of(t) for t in guard.TABLES] == [(5,), (ema.CHUNK + 1,), (3, 4, 1)]


def test_train_step_refuses_averaging_under_a_live_gradsync():
    """One process, a gloo group of one with the collectives forced on: the same refusal as clipping's.  One GPU only."""
    import torch.distributed as dist
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    from driving_dirty_amd.train import TrainStep
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))
    model = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500))
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="ema_decay under a live GradSync"):
            TrainStep(model, scheduler=False, adam_overlap=False, force_collectives=True, ema_decay=0.99)
        step = TrainStep(model, scheduler=False, adam_overlap=False, force_collectives=True)      # off: no refusal
        assert step.ema is None
        step.close()
    finally:
        dist.destroy_process_group()
