"""The sampled road-map head without a GPU: include/dd_head_mean.h and the library built from it, the third table of build.py, the
launchers' host-side refusals, the binder, the number of draws' resolution, the command line, and where the two values are kept."""
import inspect
import os
from argparse import ArgumentParser, Namespace

import pytest

from _surface import ROOT, exported_symbols, header, kernel_resources

FUNCTIONS = {"dd_head_mean_prob", "dd_head_mean_gt"}
OTHER_HEADERS = ("dd_hotpath.h", "dd_adamw.h", "dd_augment.h", "dd_ema.h", "dd_rm_loss.h", "dd_tta.h")


def small_ae():
    from driving_dirty_amd.autoencoder import BasicAE
    return BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))


def models():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE
    return RoadMapBCE, RoadMap, JointRoadMapBBox


def build_model(cls, **extra):
    return cls(Namespace(pretrained_ae=small_ae(), unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, **extra))


def test_header_declares_the_two_launch_functions_and_the_library_exports_exactly_them():
    from driving_dirty_amd import build, mc
    signatures, streamed = header("dd_head_mean.h")
    assert set(signatures) == FUNCTIONS and set(streamed) == FUNCTIONS, "both are launch functions (void* stream last)"
    assert mc.SIGNATURES == signatures and mc.STREAMED == streamed
    assert mc.OPERANDS == {"dd_head_mean_prob": 8, "dd_head_mean_gt": 9}
    entry = build.PREDICTION_EXTENSIONS["head_mean"]
    assert os.path.exists(entry.lib), "build the HIP libraries first (python __graft_entry__.py)"
    assert {n for n in exported_symbols(entry.lib) if n.startswith("dd_")} == FUNCTIONS
    assert {n for n in exported_symbols(build.LIB) if n.startswith("dd_head_mean")} == set(), "the main library's exports do not change"


def test_the_functions_appear_in_no_other_header():
    from driving_dirty_amd import build
    others = [build.HEADER] + [e.header for e in build.extensions().values()]
    assert sorted(os.path.basename(h) for h in others) == sorted(OTHER_HEADERS), "the six other headers"
    for h in others:
        text = open(h).read()
        assert "dd_head_mean" not in text, h
        assert not FUNCTIONS & set(header(os.path.basename(h))[0])


def test_the_third_table():
    """``PREDICTION_EXTENSIONS`` holds the one entry, made by the constructor of the other five; ``extensions()`` keeps its value;
    ``libraries()`` is all three tables, and what the functions that take a name look it up in."""
    from driving_dirty_amd import build
    assert list(build.PREDICTION_EXTENSIONS) == ["head_mean"]
    assert list(build.extensions()) == list(build.EXTENSIONS) + list(build.OPTIMIZER_EXTENSIONS) and "head_mean" not in build.extensions()
    assert list(build.libraries()) == list(build.extensions()) + ["head_mean"]
    e = build.PREDICTION_EXTENSIONS["head_mean"]
    assert isinstance(e, build.Extension) and e.name == "head_mean" and e.sources == ["head_mean.hip"] and e.what
    assert e.header == os.path.join(ROOT, "include", "dd_head_mean.h") and e.lib == os.path.join(build.CSRC, "libdd_head_mean.so")
    assert build.HEADER in e.headers and e.header in e.headers and all(os.path.exists(h) for h in e.headers)
    assert build.libraries()["head_mean"] is e
    with pytest.raises(KeyError):
        build.extension_needs_build("no_such_library")
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "b.extensions().values()" in text and "b.PREDICTION_EXTENSIONS" in text and "b.EXTENSIONS" not in text


def test_nothing_is_stale_after_a_build():
    from driving_dirty_amd import build
    assert build.build(force=False, verbose=False) == build.LIB
    assert not build.needs_build() and not build.extension_needs_build("head_mean")
    assert build.build_extension("head_mean", verbose=False) == build.PREDICTION_EXTENSIONS["head_mean"].lib


def test_the_kernels_use_no_scratch_and_no_spills():
    from driving_dirty_amd import build
    ks = kernel_resources().kernels(build.PREDICTION_EXTENSIONS["head_mean"].lib)
    assert len(ks) == 4, [k[".name"] for k in ks]      # one and two row tiles, fp32 and bytes
    for k in ks:
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k[".name"]
        assert 0 < k[".group_segment_fixed_size"] <= 64 * 1024, k[".name"]      # the operand tiles, which the gather reuses: static LDS


def test_one_binder_serves_this_library_too():
    from driving_dirty_amd import _lib, build, mc, tta
    for name in ("lib", "launch", "last_error"):
        fn = vars(mc)[name]      # module-level names, so that a monkeypatched ``launch`` takes effect
        assert isinstance(fn.__self__, _lib.Extension) and fn.__func__ is getattr(_lib.Extension, name)
    assert mc.LIB == build.PREDICTION_EXTENSIONS["head_mean"].lib and "call" not in vars(mc) and "size" not in vars(mc)
    assert mc.lib.__self__ is not tta.lib.__self__ and mc.lib() is mc.lib()
    with pytest.raises(mc.HotpathError, match="operands given"):
        mc.launch("dd_head_mean_gt", 1 << 20, 2 << 20, None, 3 << 20, 2, 4, 16, 8)
    with pytest.raises(mc.HotpathError, match="not a function of include/dd_head_mean.h"):
        mc.launch("dd_tta_mean_prob", 1 << 20, 2 << 20, 3 << 20, 2, 4, 8, 0)


def test_launchers_refuse_bad_arguments_without_a_gpu():
    from driving_dirty_amd import mc
    lib = mc.lib()
    x, w, bias, out = 1 << 20, 2 << 20, 3 << 20, 4 << 20      # never dereferenced: every call below is refused on the host

    def refused(rc, *words):
        msg = mc.last_error()
        assert rc != 0 and msg and all(word in msg for word in words), (rc, msg)

    def prob(x=x, w=w, bias=bias, out=out, scenes=2, samples=4, n=16, k=8):
        return lib.dd_head_mean_prob(x, w, bias, out, scenes, samples, n, k, None)

    def gt(x=x, w=w, bias=bias, out=out, scenes=2, samples=4, n=16, k=8):
        return lib.dd_head_mean_gt(x, w, bias, 0.5, out, scenes, samples, n, k, None)

    for fn, who, elem in ((prob, "head_mean_prob", 4), (gt, "head_mean_gt", 1)):
        for name in ("x", "w", "out"):
            refused(fn(**{name: None}), who, "NULL")
        for bad in (dict(scenes=0), dict(scenes=-2), dict(n=0), dict(n=-16), dict(k=0), dict(k=-8)):
            refused(fn(**bad), who, "non-positive")
        for bad in (0, 65, -1, 1 << 20):
            refused(fn(samples=bad), who, "samples", str(bad))
        for bad in (6, 63, 513):
            refused(fn(k=bad), who, "multiple of 4")
        for bad in (516, 1024, 940032):      # dd_linear_fwd would split these over workgroups (or might): not the same bits
            refused(fn(k=bad), who, "splits K", str(bad))
        refused(fn(scenes=1 << 16, n=1 << 15), who, "too large", "2^31")      # exactly 2^31 elements
        refused(fn(scenes=3356, n=640000), who, "too large")
        refused(fn(x=x + 4), who, "16-byte")
        refused(fn(w=w + 8), who, "16-byte")
        refused(fn(out=out + elem), who, "16-byte")
        refused(fn(bias=bias + 2), who, "bias", "4-byte")
        refused(fn(out=x), who, "overlaps")
        refused(fn(out=w), who, "overlaps")
        refused(fn(out=bias), who, "overlaps")
        refused(fn(out=x + 2 * 4 * 8 * 4 - 16), who, "overlaps")      # the output begins inside the last 16 bytes of x
        refused(fn(x=out + 16 * elem), who, "overlaps")                # ... and x begins inside the output


def test_resolve_maps_the_argument_to_a_number_of_draws():
    from driving_dirty_amd import mc
    off, on = Namespace(hparams=Namespace()), Namespace(hparams=Namespace(mc_samples=8, mc_seed=3))
    assert mc.resolve(off, None) == 1 and mc.resolve(on, None) == 8 and mc.seed_of(off) == 0 and mc.seed_of(on) == 3
    assert mc.resolve(Namespace(), None) == 1 and mc.resolve(Namespace(hparams=None), None) == 1
    for module in (off, on):
        assert mc.resolve(module, 1) == 1 and mc.resolve(module, 64) == 64 and mc.resolve(module, 5) == 5
        for bad in (0, 65, -1, 2.0, "4", True, (4,)):
            with pytest.raises(ValueError, match="mc_samples"):
                mc.resolve(module, bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="mc_samples"):
            mc.resolve(Namespace(hparams=Namespace(mc_samples=bad)), None)
    for bad in (-1, 1.5, "7", True):
        with pytest.raises(ValueError, match="mc_seed"):
            mc.seed_of(Namespace(hparams=Namespace(mc_seed=bad)))


def test_the_parsers_take_the_two_flags_and_refuse_bad_values_by_name(capsys):
    for cls in models():
        parse = cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args
        args = parse([])
        assert args.mc_samples == 1 and args.mc_seed == 0
        args = parse(["--mc_samples", "16", "--mc_seed", "12345"])
        assert args.mc_samples == 16 and args.mc_seed == 12345
        for argv, name in ((["--mc_samples", "0"], "mc_samples"), (["--mc_samples", "65"], "mc_samples"), (["--mc_samples", "x"], "mc_samples"),
                           (["--mc_seed", "-1"], "mc_seed")):
            with pytest.raises(SystemExit):
                parse(argv)
            assert name in capsys.readouterr().err
        for bad in (dict(mc_samples=0), dict(mc_samples=65), dict(mc_seed=-1)):      # and the constructor refuses what a checkpoint or a caller hands it
            with pytest.raises(ValueError, match=next(iter(bad))):
                build_model(cls, **bad)


def test_the_prediction_methods_take_the_number_of_draws():
    RoadMapBCE, RoadMap, JointRoadMapBBox = models()
    for fn in (RoadMapBCE.predict_road_map, RoadMap.predict_road_map, JointRoadMapBBox.predict_road_map, JointRoadMapBBox.predict_mode):
        assert inspect.signature(fn).parameters["mc_samples"].default is None, fn
    assert "mc_samples" not in inspect.signature(JointRoadMapBBox.predict).parameters, "its signature is pinned: it follows the hparams"


def test_one_draw_never_reaches_the_library(monkeypatch):
    """``mc_samples = 1`` -- the default, the argument, the hparams -- takes the parent's branch: ``predict_map`` / ``predict_map_tta``, never
    ``predict_map_mc``, and ``mc.launch`` is not entered.  More draws take ``predict_map_mc``."""
    from driving_dirty_amd import mc, roadmap
    seen = []
    monkeypatch.setattr(mc, "launch", lambda *a: pytest.fail("mc.launch reached"))
    monkeypatch.setattr(roadmap, "predict_map", lambda module, latent, threshold: seen.append("plain"))
    monkeypatch.setattr(roadmap, "predict_map_tta", lambda module, encode, x, threshold: seen.append("mirror"))
    monkeypatch.setattr(roadmap, "predict_map_mc", lambda module, pooled, x, threshold, tta, samples: seen.append(("mc", tta, samples)))
    from driving_dirty_amd import joint
    for name in ("predict_map", "predict_map_tta", "predict_map_mc"):
        monkeypatch.setattr(joint, name, getattr(roadmap, name))
    import torch
    x = torch.zeros((1, 6, 3, 16, 22))
    for cls in models():
        del seen[:]
        model = build_model(cls)
        model.predict_road_map(x)
        model.predict_road_map(x, 0.4, mc_samples=1)
        model.predict_road_map(x, tta=True)
        model.predict_road_map(x, mc_samples=1, tta="mirror")
        build_model(cls, mc_samples=1, mc_seed=9).predict_road_map(x)
        assert seen == ["plain", "plain", "mirror", "mirror", "plain"], (cls, seen)
        del seen[:]
        model.predict_road_map(x, mc_samples=4)
        model.predict_road_map(x, mc_samples=4, tta=True)
        flagged = build_model(cls, mc_samples=16)
        flagged.predict_road_map(x)
        flagged.predict_road_map(x, mc_samples=1)      # the argument wins
        assert seen == [("mc", None, 4), ("mc", "mirror", 4), ("mc", None, 16), "plain"], (cls, seen)


def test_the_values_live_in_hparams_and_in_the_checkpoint_not_in_the_state_dict(tmp_path):
    from driving_dirty_amd import mc
    for cls in models():
        plain, model = build_model(cls), build_model(cls, mc_samples=8, mc_seed=41)
        keys = list(model.state_dict().keys())
        assert keys == list(plain.state_dict().keys()) and "mc_" not in "".join(keys)
        assert mc.resolve(plain, None) == 1 and mc.resolve(model, None) == 8
        path = str(tmp_path / f"{cls.__name__}.ckpt")
        model.save_checkpoint(path)
        loaded = cls.load_from_checkpoint(path)
        assert loaded.hparams.mc_samples == 8 and loaded.hparams.mc_seed == 41 and mc.resolve(loaded, None) == 8 and mc.seed_of(loaded) == 41
        assert list(loaded.state_dict().keys()) == keys
        plain.save_checkpoint(path)
        assert mc.resolve(cls.load_from_checkpoint(path), None) == 1


def test_validation_epoch_end_averages_the_new_keys():
    import torch
    RoadMapBCE, RoadMap, JointRoadMapBBox = models()
    one, three = torch.tensor(1.0), torch.tensor(3.0)
    base = {"val_loss": one, "val_ts": one, "val_ts_rounded": one}
    for cls in (RoadMapBCE, RoadMap):
        log = build_model(cls).validation_epoch_end([{**base, "val_ts_mc": one, "val_ts_rounded_mc": three},
                                                     {**base, "val_ts_mc": three, "val_ts_rounded_mc": three}])["log"]
        assert float(log["avg_val_ts_mc"]) == 2.0 and float(log["avg_val_ts_rounded_mc"]) == 3.0
        assert set(build_model(cls).validation_epoch_end([base])["log"]) == {"avg_val_loss", "avg_val_ts_rounded", "avg_val_ts"}
    joint = {**base, "val_roadmap_loss": one, "val_bbox_loss": one}
    log = build_model(JointRoadMapBBox).validation_epoch_end([{**joint, "val_ts_mc": one, "val_ts_rounded_mc": one},
                                                              {**joint, "val_ts_mc": three, "val_ts_rounded_mc": one}])["log"]
    assert float(log["avg_val_ts_mc"]) == 2.0 and float(log["avg_val_ts_rounded_mc"]) == 1.0


def test_the_cpu_restatement_of_the_pinned_order():
    """tests/_head_mean_ref.py against itself: the fp32 order is the left-to-right sum (NOT torch.mean's pairwise one), S = 1 and powers
    of two multiply exactly, and the fp32 restatement stays within the bound of the fp64 reference."""
    import numpy as np
    import torch

    import _head_mean_ref as ref
    rs = np.random.RandomState(5)
    for scenes, samples in ((3, 1), (2, 3), (4, 16), (1, 64), (2, 33)):
        p = torch.from_numpy(rs.random_sample((scenes * samples, 40)).astype(np.float32))
        got = ref.mean_in_draw_order(p, samples)
        want = np.zeros((scenes, 40), np.float32)
        for b in range(scenes):
            acc = p[b * samples].numpy().copy()
            for s in range(1, samples):
                acc = (acc + p[b * samples + s].numpy()).astype(np.float32)
            want[b] = acc * np.float32(1.0 / samples)
        assert np.array_equal(got.numpy(), want)
        exact = p.double().reshape(scenes, samples, 40).mean(1)
        assert float((got.double() - exact).abs().max()) <= samples * 2.0 ** -24
        if samples == 1:
            assert torch.equal(got, p)
    assert ref.inv_samples(3) == float(np.float32(1.0 / 3.0)) and ref.inv_samples(16) == 0.0625
    mean = torch.tensor([0.25, 0.5, float("nan"), 0.75])
    assert ref.gt(mean, 0.5).tolist() == [False, False, False, True]


def test_every_launch_function_of_the_library_has_a_guard_case():
    """The census of tests/test_guard_arena.py for this library: the case table imports without a GPU, names only launch functions of
    dd_head_mean.h, and every one of them is the subject of a case.  None picks a kernel by alignment."""
    import test_gpu_guard_head_mean as guard
    from driving_dirty_amd import mc
    assert guard.CASES and len({c.name for c in guard.CASES}) == len(guard.CASES)
    assert {e for c in guard.CASES for e in c.entry} == set(mc.STREAMED) == set(mc.SIGNATURES)
    assert not any(c.picks_kernel_by_alignment or c.crosses for c in guard.CASES)
    for entry in mc.STREAMED:
        assert sum(1 for c in guard.CASES if c.entry == (entry,)) == len(guard.SHAPES)


def test_the_model_reference_alone_stays_clear_of_the_threshold():
    """tests/_head_mean_cases.py, on the CPU: at its ``TAU`` and seeds at most 1 % of the fp64 mean probabilities lie within the model
    bound of the threshold (the elements tests/test_gpu_head_mean_models.py leaves out of the map comparison), both classes are
    present, and the S-draw mean differs from a single draw by far more than that bound."""
    import torch

    import _head_mean_cases as hc
    from driving_dirty_amd.roadmap import RoadMapBCE
    model = hc.build(RoadMapBCE)
    for samples in hc.DRAWS:
        masks = hc.keeps(samples)
        assert all(tuple(k.shape) == (hc.B * samples, hc.HIDDEN) and set(k.unique().tolist()) == {0.0, 1.0} for k in masks)
        mean = hc.reference64(model, hc.views(), samples, masks)
        assert mean.dtype == torch.float64 and tuple(mean.shape) == (hc.B, 800, 800)
        out = float(hc.band(mean).float().mean())
        assert out <= 0.01, (samples, out)
        assert 0.05 < float((mean > hc.TAU).float().mean()) < 0.95
        one = hc.reference64(model, hc.views(), 1, tuple(k.reshape(hc.B, samples, hc.HIDDEN)[:, 0].contiguous() for k in masks))
        assert float((one - mean).abs().max()) > 100 * hc.MODEL_BOUND
