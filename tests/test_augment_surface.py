"""The augmentation's surface without a GPU: include/dd_augment.h and the library built from it, the launchers' host-side refusals,
the augmenter's draws, defaults, flags and errors, and the box mirror."""
import ctypes as C
import os
from argparse import ArgumentParser, Namespace

import numpy as np
import pytest
import torch

import _augment_ref as ref
from _surface import exported_symbols, header

AUG = dict(aug_mirror=0.5, aug_brightness=0.2, aug_contrast=0.1, aug_per_view=0.05, aug_view_drop=0.25, aug_seed=7)


def test_header_declares_launch_functions_of_its_own_and_the_library_exports_exactly_them():
    from driving_dirty_amd import _lib, augment, build
    signatures, streamed = header("dd_augment.h")
    assert set(signatures) == {"dd_aug_views_u8_ptrs", "dd_aug_views_ptrs", "dd_aug_masks_u8_ptrs"}
    assert set(signatures) == set(streamed), "every function of dd_augment.h is a launch function (void* stream last)"
    assert all(n.startswith("dd_aug_") for n in signatures)
    assert not set(signatures) & set(_lib.SIGNATURES)
    assert augment.SIGNATURES == signatures and augment.OPERANDS == {n: len(a) - 1 for n, (_, a) in signatures.items()}
    assert os.path.exists(build.EXTENSIONS["augment"].lib), "build the HIP libraries first (python __graft_entry__.py)"
    assert {n for n in exported_symbols(build.EXTENSIONS["augment"].lib) if n.startswith("dd_")} == set(signatures)
    assert build.build(force=False, verbose=False) == build.LIB and not build.needs_build()
    assert "launch" in vars(augment) and "call" not in vars(augment) and "size" not in vars(augment)


def test_every_launch_function_of_the_extension_has_a_guard_case():
    """The census of tests/test_guard_arena.py for the extension library: its case table imports without a GPU, names only launch
    functions of dd_augment.h, and every one of them is the subject of a case.  None picks a kernel by alignment."""
    import test_gpu_guard_augment as guard
    from driving_dirty_amd import augment
    assert guard.CASES and len({c.name for c in guard.CASES}) == len(guard.CASES)
    covered = {e for c in guard.CASES for e in c.entry}
    assert covered == set(augment.STREAMED) == set(augment.SIGNATURES)
    assert not any(c.picks_kernel_by_alignment or c.crosses for c in guard.CASES)


def test_launchers_refuse_bad_arguments_without_a_gpu():
    from driving_dirty_amd import augment
    lib = augment.lib()
    ok_flags, bad_flags = (C.c_uint32 * 2)(1, 1 << 13), (C.c_uint32 * 2)(0, 2)
    color = (C.c_float * 24)(*([1.0, 0.0] * 12))
    table = (C.c_void_p * 2)(4096, 8192)      # never dereferenced: every call below is refused on the host
    out = 1 << 20

    def refused(rc, *words):
        msg = augment.last_error()
        assert rc != 0 and msg and all(w in msg for w in words), (rc, msg)

    for fn, who in ((lib.dd_aug_views_u8_ptrs, "aug_views_u8_ptrs"), (lib.dd_aug_views_ptrs, "aug_views_ptrs")):
        refused(fn(None, ok_flags, color, out, 2, 4, 5, None), who, "NULL")
        refused(fn(table, None, color, out, 2, 4, 5, None), who, "NULL")
        refused(fn(table, ok_flags, None, out, 2, 4, 5, None), who, "NULL")
        refused(fn(table, ok_flags, color, None, 2, 4, 5, None), who, "NULL")
        refused(fn(table, ok_flags, color, out, 0, 4, 5, None), who, "non-positive")
        refused(fn(table, ok_flags, color, out, -3, 4, 5, None), who, "non-positive")
        refused(fn(table, ok_flags, color, out, 2, 0, 5, None), who, "non-positive")
        refused(fn(table, ok_flags, color, out, 2, 4, -1, None), who, "non-positive")
        refused(fn(table, bad_flags, color, out, 2, 4, 5, None), who, "flags[1]", "0x2")
        refused(fn(table, ok_flags, color, out + 4, 2, 4, 5, None), who, "16-byte")
        refused(fn((C.c_void_p * 2)(4096, None), ok_flags, color, out, 2, 4, 5, None), who, "null sample")
    fn, who = lib.dd_aug_masks_u8_ptrs, "aug_masks_u8_ptrs"
    refused(fn(None, ok_flags, out, 2, 4, 5, None), who, "NULL")
    refused(fn(table, None, out, 2, 4, 5, None), who, "NULL")
    refused(fn(table, ok_flags, None, 2, 4, 5, None), who, "NULL")
    refused(fn(table, ok_flags, out, 0, 4, 5, None), who, "non-positive")
    refused(fn(table, ok_flags, out, 2, 0, 5, None), who, "non-positive")
    refused(fn(table, ok_flags, out, 2, 4, 0, None), who, "non-positive")
    refused(fn(table, (C.c_uint32 * 2)(1, 1 << 14), out, 2, 4, 5, None), who, "flags[1]")
    refused(lib.dd_aug_views_ptrs((C.c_void_p * 2)(4096, 8194), ok_flags, color, out, 2, 4, 5, None), "aligned")      # fp32 on 2 bytes
    with pytest.raises(augment.HotpathError, match="operands given"):
        augment.launch("dd_aug_masks_u8_ptrs", table, ok_flags, out, 2, 4)
    with pytest.raises(augment.HotpathError, match="not a function"):
        augment.launch("dd_stitch6_ptrs", table, out, 2, 4, 5)


def test_draw_is_seeded_per_rank_and_leaves_the_global_generators_alone():
    from driving_dirty_amd.augment import FLAG_MIRROR, Augmenter
    torch.manual_seed(123)
    np.random.seed(123)
    t0, n0 = torch.get_rng_state(), np.random.get_state()
    a, again, other = Augmenter(Namespace(**AUG), rank=0), Augmenter(Namespace(**AUG), rank=0), Augmenter(Namespace(**AUG), rank=1)
    fa, ca = a.draw(64)
    fb, cb = again.draw(64)
    fo, co = other.draw(64)
    assert torch.equal(fa, fb) and torch.equal(ca, cb)
    assert not torch.equal(fa, fo) and not torch.equal(ca, co)
    f2, c2 = a.draw(64)
    assert not torch.equal(fa, f2), "the generator moves on"
    assert torch.equal(torch.get_rng_state(), t0)
    n1 = np.random.get_state()
    assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]
    assert fa.dtype == torch.int64 and tuple(fa.shape) == (64,) and ca.dtype == torch.float32 and tuple(ca.shape) == (64, 6, 2)
    # what the draws are: one blank bit at most, only known bits, the factors in their ranges, the bias that of the contrast
    blank = (fa >> 8) & 0x3F
    assert bool(((fa & ~(FLAG_MIRROR | (0x3F << 8))) == 0).all()) and bool(((blank & (blank - 1)) == 0).all())
    lo, hi = (1 - 0.2) * (1 - 0.1) * (1 - 0.05), (1 + 0.2) * (1 + 0.1) * (1 + 0.05)
    assert float(ca[..., 0].min()) >= lo - 1e-6 and float(ca[..., 0].max()) <= hi + 1e-6
    assert float(ca[..., 1].abs().max()) <= 0.5 * 0.1 + 1e-6 and torch.equal(ca[:, :1, 1].expand(64, 6), ca[..., 1])
    # the mirror frequency at p = 0.5 over 4096 samples: 0.5 +- 0.04 is 5 sigma of a fair coin (sigma = 0.5 / sqrt(4096) = 0.0078)
    flags, _ = Augmenter(Namespace(aug_mirror=0.5, aug_seed=1)).draw(4096)
    assert abs(float((flags & FLAG_MIRROR).double().mean()) - 0.5) <= 0.04
    # one view dropped with probability 0.25, uniformly: every view is hit (6 x 170 expected)
    flags, color = Augmenter(Namespace(aug_view_drop=0.25, aug_seed=1)).draw(4096)
    assert abs(float(((flags >> 8) != 0).double().mean()) - 0.25) <= 5 * (0.25 * 0.75 / 4096) ** 0.5
    assert all(int(((flags >> (8 + v)) & 1).sum()) > 100 for v in range(6))
    assert bool((color[..., 0] == 1).all()) and bool((color[..., 1] == 0).all()), "no jitter asked for: the identity colour, exactly"


def test_defaults_are_off_and_apply_hands_the_batch_back():
    from driving_dirty_amd.augment import Augmenter
    for hp in (None, Namespace(), Namespace(aug_mirror=0.0, aug_brightness=0, aug_contrast=0.0, aug_per_view=0.0, aug_view_drop=0.0, aug_seed=5)):
        a = Augmenter(hp)
        assert a.enabled is False
        batch = (torch.zeros(2, 6, 3, 4, 5), None, (torch.zeros(4, 4, dtype=torch.bool),) * 2)
        assert a.apply(batch) is batch
        views = torch.zeros(2, 6, 3, 4, 5)
        assert a.apply(views) is views
    assert Augmenter(Namespace(aug_per_view=0.1)).enabled is True


def test_the_four_parsers_accept_the_flags():
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    argv = ["--aug_mirror", "0.5", "--aug_brightness", "0.2", "--aug_contrast", "0.1", "--aug_per_view", "0.05", "--aug_seed", "9"]
    for cls in (BasicAE, RoadMapBCE, RoadMap, BBSpatialRoadMap, JointRoadMapBBox):
        hp = cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args(argv + ["--aug_view_drop", "0.3"])
        assert (hp.aug_mirror, hp.aug_brightness, hp.aug_contrast, hp.aug_per_view, hp.aug_view_drop, hp.aug_seed) == (0.5, 0.2, 0.1, 0.05, 0.3, 9)
        off = cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([])
        assert (off.aug_mirror, off.aug_brightness, off.aug_contrast, off.aug_per_view, off.aug_view_drop, off.aug_seed) == (0, 0, 0, 0, 0, 0)


def test_models_build_their_augmenter_from_the_hparams():
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    small = dict(hidden_dim=16, latent_dim=8, input_height=16, input_width=6 * 22)
    assert BasicAE(Namespace(**small)).augment.enabled is False
    ae = BasicAE(Namespace(**small, aug_mirror=0.5, aug_seed=3))
    assert ae.augment.enabled and ae.augment.mirror == 0.5 and ae.augment.seed == 3 and ae.augment.rank == 0
    with pytest.raises(ValueError, match="aug_view_drop"):
        BasicAE(Namespace(**small, aug_view_drop=0.1))
    hp = dict(unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500)
    for cls in (RoadMapBCE, RoadMap, BBSpatialRoadMap, JointRoadMapBBox):
        assert cls(Namespace(pretrained_ae=BasicAE(Namespace(**small)), **hp)).augment.enabled is False
        m = cls(Namespace(pretrained_ae=BasicAE(Namespace(**small)), **hp, aug_view_drop=0.5, aug_contrast=0.2))
        assert m.augment.enabled and m.augment.view_drop == 0.5 and m.augment.contrast == 0.2
        assert "augment" not in "".join(m.state_dict()), "the augmenter holds no parameters or buffers"


@pytest.mark.parametrize("hp", [dict(aug_mirror=1.5), dict(aug_mirror=-0.1), dict(aug_view_drop=2), dict(aug_brightness=1.0),
                                dict(aug_contrast=-0.2), dict(aug_per_view=3.0), dict(aug_seed=-1)])
def test_values_outside_their_ranges_raise(hp):
    from driving_dirty_amd.augment import Augmenter
    with pytest.raises(ValueError, match=next(iter(hp))):
        Augmenter(Namespace(**hp))


def test_a_mirrored_sample_with_a_prerasterised_map_raises_before_any_launch(monkeypatch):
    from driving_dirty_amd import augment
    launched = []
    monkeypatch.setattr(augment, "launch", lambda *a: launched.append(a))
    a = augment.Augmenter(Namespace(aug_mirror=1.0))
    target = ({"bounding_box": torch.zeros(1, 2, 4, dtype=torch.float64), "bb_map": torch.zeros(800, 800)},) * 2
    batch = (torch.zeros(2, 6, 3, 4, 5), target, (torch.zeros(4, 4, dtype=torch.bool),) * 2)
    with pytest.raises(ValueError, match="bb_map"):
        a.apply(batch)
    with pytest.raises(ValueError, match="bb_map"):
        a.apply(batch, draw=(torch.tensor([0, 1]), torch.tensor([[[1.0, 0.0]] * 6] * 2)))
    assert not launched


def test_box_mirror_is_an_involution_and_keeps_dtype_and_device():
    from driving_dirty_amd import synth
    from driving_dirty_amd.augment import mirror_boxes
    bb = synth.car_boxes(9, seed=3)
    assert bb.dtype == torch.float64
    for x in (bb, bb.float(), bb[:0]):
        m = mirror_boxes(x)
        assert m.dtype == x.dtype and m.shape == x.shape and m.is_contiguous()
        assert torch.equal(m, ref.boxes(x))
        back = mirror_boxes(m)
        assert torch.equal(back.view(torch.int64 if x.dtype == torch.float64 else torch.int32),
                           x.view(torch.int64 if x.dtype == torch.float64 else torch.int32)), "applied twice: the identity, bit for bit"
    # front-left becomes front-right: x kept, y negated
    m = mirror_boxes(bb)
    assert torch.equal(m[:, 0, 1], bb[:, 0, 0]) and torch.equal(m[:, 1, 1], -bb[:, 1, 0])
    assert torch.equal(m[:, 0, 2], bb[:, 0, 3]) and torch.equal(m[:, 1, 2], -bb[:, 1, 3])
    with pytest.raises(ValueError):
        mirror_boxes(torch.zeros(3, 4, 2))


def test_the_reference_mirror_of_the_views_is_the_blockwise_reversal_of_the_wide_image():
    """The reference itself against the geometry: in the wide image of view order [0,1,2,5,4,3] the mirror reverses columns [0,3W)
    as a block and columns [3W,6W) likewise."""
    x = torch.arange(2 * 6 * 3 * 2 * 5, dtype=torch.float32).reshape(2, 6, 3, 2, 5)
    ident = torch.tensor([[[1.0, 0.0]] * 6] * 2)
    got = ref.views(x, [1, 0], ident)

    def wide(v):
        return v[:, [0, 1, 2, 5, 4, 3]].permute(0, 2, 3, 1, 4).reshape(v.shape[0], 3, 2, 30)
    w, wm = wide(x), wide(got)
    assert torch.equal(wm[0, ..., :15], w[0, ..., :15].flip(-1)) and torch.equal(wm[0, ..., 15:], w[0, ..., 15:].flip(-1))
    assert torch.equal(wm[1], w[1])
