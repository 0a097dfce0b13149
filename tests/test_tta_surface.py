"""Mirror test-time averaging without a GPU: include/dd_tta.h and the library built from it, the launchers' host-side refusals, the
binder it shares with the augmentation, the mode's resolution, the command line, and where the flag is kept."""
import inspect
import os
from argparse import ArgumentParser, Namespace

import pytest

from _surface import exported_symbols, header, kernel_resources

FUNCTIONS = {"dd_tta_mean_prob", "dd_tta_mean_gt"}


def small_ae():
    from driving_dirty_amd.autoencoder import BasicAE
    return BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))


def models():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    return RoadMapBCE, RoadMap, BBSpatialRoadMap, JointRoadMapBBox


def build_model(cls, **extra):
    return cls(Namespace(pretrained_ae=small_ae(), unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, **extra))


def test_header_declares_the_two_launch_functions_and_the_library_exports_exactly_them():
    from driving_dirty_amd import build, tta
    signatures, streamed = header("dd_tta.h")
    assert set(signatures) == FUNCTIONS and set(streamed) == FUNCTIONS, "both are launch functions (void* stream last)"
    assert tta.SIGNATURES == signatures and tta.STREAMED == streamed
    assert tta.OPERANDS == {"dd_tta_mean_prob": 7, "dd_tta_mean_gt": 8}
    assert os.path.exists(build.EXTENSIONS["tta"].lib), "build the HIP libraries first (python __graft_entry__.py)"
    assert {n for n in exported_symbols(build.EXTENSIONS["tta"].lib) if n.startswith("dd_")} == FUNCTIONS
    assert build.build(force=False, verbose=False) == build.LIB and not build.needs_build()


def test_one_binder_serves_both_extension_libraries():
    from driving_dirty_amd import _lib, augment, build, tta
    for mod, lib, hdr in ((augment, build.EXTENSIONS["augment"].lib, "dd_augment.h"), (tta, build.EXTENSIONS["tta"].lib, "dd_tta.h")):
        for name in ("lib", "launch", "last_error"):
            fn = vars(mod)[name]      # module-level names, so that a monkeypatched ``launch`` takes effect
            assert isinstance(fn.__self__, _lib.Extension) and fn.__func__ is getattr(_lib.Extension, name)
        assert mod.LIB == lib and mod.SIGNATURES == header(hdr)[0]
        assert "call" not in vars(mod) and "size" not in vars(mod)
    assert augment.lib.__self__ is not tta.lib.__self__
    assert tta.lib() is tta.lib()
    with pytest.raises(tta.HotpathError, match="operands given"):
        tta.launch("dd_tta_mean_gt", 1 << 20, 2 << 20, 0.5, 3 << 20, 2, 4)
    with pytest.raises(tta.HotpathError, match="not a function of include/dd_tta.h"):
        tta.launch("dd_aug_masks_u8_ptrs", 1 << 20, 2 << 20, 3 << 20, 2, 4, 5, 0)


def test_the_kernels_use_no_scratch_and_no_lds():
    from driving_dirty_amd import build
    ks = kernel_resources().kernels(build.EXTENSIONS["tta"].lib)
    assert len(ks) >= 6, [k[".name"] for k in ks]      # vector and scalar forms, bytes and fp32, logits and probabilities
    for k in ks:
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0 and k[".group_segment_fixed_size"] == 0, k[".name"]


def test_launchers_refuse_bad_arguments_without_a_gpu():
    from driving_dirty_amd import tta
    lib = tta.lib()
    a, m, out = 1 << 20, 2 << 20, 3 << 20      # never dereferenced: every call below is refused on the host

    def refused(rc, *words):
        msg = tta.last_error()
        assert rc != 0 and msg and all(w in msg for w in words), (rc, msg)

    def prob(a=a, m=m, out=out, b=2, h=4, w=8, fl=0):
        return lib.dd_tta_mean_prob(a, m, out, b, h, w, fl, None)

    def gt(a=a, m=m, out=out, b=2, h=4, w=8, fl=0):
        return lib.dd_tta_mean_gt(a, m, 0.5, out, b, h, w, fl, None)

    for fn, who, elem in ((prob, "tta_mean_prob", 4), (gt, "tta_mean_gt", 1)):
        for name in ("a", "m", "out"):
            refused(fn(**{name: None}), who, "NULL")
        for bad in (dict(b=0), dict(b=-3), dict(h=0), dict(h=-1), dict(w=0), dict(w=-8)):
            refused(fn(**bad), who, "non-positive")
        refused(fn(b=1 << 15, h=1 << 8, w=1 << 8), who, "too large", "2^31")      # exactly 2^31 elements
        refused(fn(b=32768, h=800, w=800), who, "too large")
        for bad in (2, -1, 256):
            refused(fn(fl=bad), who, "from_logits", str(bad))
        refused(fn(a=a + 4), who, "16-byte")
        refused(fn(m=m + 8), who, "16-byte")
        refused(fn(out=out + elem), who, "16-byte")
        refused(fn(out=a), who, "in place")
        refused(fn(out=m), who, "in place")
        refused(fn(a=a, m=a, out=a), who, "in place")
        refused(fn(out=a + 2 * 4 * 8 * 4 - 16), who, "in place")      # the output begins inside the last 16 bytes of `a`
        refused(fn(a=out + 16 * elem, b=2, h=4, w=8), who, "in place")      # ... and `a` begins inside the output


def test_resolve_maps_the_argument_to_a_mode():
    from driving_dirty_amd import tta
    off, on = Namespace(hparams=Namespace()), Namespace(hparams=Namespace(tta_mirror=True))
    assert tta.resolve(off, None) is None and tta.resolve(on, None) == "mirror" == tta.MIRROR
    assert tta.resolve(Namespace(hparams=Namespace(tta_mirror=False)), None) is None
    assert tta.resolve(Namespace(), None) is None and tta.resolve(Namespace(hparams=None), None) is None
    for module in (off, on):
        assert tta.resolve(module, False) is None
        assert tta.resolve(module, True) == "mirror" and tta.resolve(module, "mirror") == "mirror"
        for bad in ("flip", "Mirror", "", 1, 0, 2, 1.0, ("mirror",), b"mirror"):
            with pytest.raises(ValueError, match="tta"):
                tta.resolve(module, bad)


def test_the_four_parsers_accept_the_flag_and_default_to_off():
    for cls in models():
        assert cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args(["--tta_mirror"]).tta_mirror is True
        assert cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([]).tta_mirror is False


def test_the_prediction_methods_take_the_mode_as_a_trailing_keyword():
    RoadMapBCE, RoadMap, BBSpatialRoadMap, JointRoadMapBBox = models()
    for fn in (RoadMapBCE.predict_road_map, RoadMap.predict_road_map, BBSpatialRoadMap.predict_boxes, JointRoadMapBBox.predict_road_map,
               JointRoadMapBBox.predict_boxes):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "tta" and last.default is None, fn
    assert inspect.signature(JointRoadMapBBox.predict_mode).parameters["tta"].default is None
    assert list(inspect.signature(JointRoadMapBBox.predict_mode).parameters)[:3] == ["self", "x", "tta"]


def test_the_flag_lives_in_hparams_and_in_the_checkpoint_not_in_the_state_dict(tmp_path):
    from driving_dirty_amd import tta
    for cls in models():
        plain, model = build_model(cls), build_model(cls, tta_mirror=True)
        keys = list(model.state_dict().keys())
        assert keys == list(plain.state_dict().keys()) and "tta" not in "".join(keys)
        assert tta.resolve(plain, None) is None and tta.resolve(model, None) == "mirror"
        path = str(tmp_path / f"{cls.__name__}.ckpt")
        model.save_checkpoint(path)
        loaded = cls.load_from_checkpoint(path)
        assert loaded.hparams.tta_mirror is True and tta.resolve(loaded, None) == "mirror" and list(loaded.state_dict().keys()) == keys
        plain.save_checkpoint(path)
        assert tta.resolve(cls.load_from_checkpoint(path), None) is None


def test_validation_epoch_end_averages_the_new_keys():
    import torch
    RoadMapBCE, RoadMap, BBSpatialRoadMap, JointRoadMapBBox = models()
    one, three = torch.tensor(1.0), torch.tensor(3.0)
    base = {"val_loss": one, "val_ts": one, "val_ts_rounded": one}
    for cls in (RoadMapBCE, RoadMap):
        log = build_model(cls).validation_epoch_end([{**base, "val_ts_tta": one, "val_ts_rounded_tta": three},
                                                     {**base, "val_ts_tta": three, "val_ts_rounded_tta": three}])["log"]
        assert float(log["avg_val_ts_tta"]) == 2.0 and float(log["avg_val_ts_rounded_tta"]) == 3.0
        assert set(build_model(cls).validation_epoch_end([base])["log"]) == {"avg_val_loss", "avg_val_ts_rounded", "avg_val_ts"}
    log = build_model(BBSpatialRoadMap).validation_epoch_end([{"val_loss": one, "val_ats_tta": one, "val_ts_tta": three},
                                                              {"val_loss": one, "val_ats_tta": three, "val_ts_tta": three}])["log"]
    assert float(log["avg_val_ats_tta"]) == 2.0 and float(log["avg_val_ts_tta"]) == 3.0
    joint = {**base, "val_roadmap_loss": one, "val_bbox_loss": one}
    log = build_model(JointRoadMapBBox).validation_epoch_end([{**joint, "val_ts_tta": one, "val_ts_rounded_tta": one, "val_ats_tta": one},
                                                              {**joint, "val_ts_tta": three, "val_ts_rounded_tta": one, "val_ats_tta": three}])["log"]
    assert float(log["avg_val_ts_tta"]) == 2.0 and float(log["avg_val_ts_rounded_tta"]) == 1.0 and float(log["avg_val_ats_tta"]) == 2.0


def test_every_launch_function_of_the_library_has_a_guard_case():
    """The census of tests/test_guard_arena.py for this library: the case table imports without a GPU, names only launch functions of
    dd_tta.h, and every one of them is the subject of a case.  None picks a kernel by alignment."""
    import test_gpu_guard_tta as guard
    from driving_dirty_amd import tta
    assert guard.CASES and len({c.name for c in guard.CASES}) == len(guard.CASES)
    assert {e for c in guard.CASES for e in c.entry} == set(tta.STREAMED) == set(tta.SIGNATURES)
    assert not any(c.picks_kernel_by_alignment or c.crosses for c in guard.CASES)
    for entry in tta.STREAMED:      # the three shapes, each with logits and with probabilities
        assert sum(1 for c in guard.CASES if c.entry == (entry,)) == 2 * len(guard.SHAPES) == 6
