"""The sampled head's uncertainty without a GPU: include/dd_head_uncert.h and the library built from it, the sixth table of build.py,
the launcher's host-side refusals, the binder, the model surface and the validation step's calls with the flag off."""
import inspect
import os
from argparse import ArgumentParser, Namespace

import pytest

from _surface import ROOT, exported_symbols, header, kernel_resources

FUNCTIONS = {"dd_head_uncert"}
# libdd_head_mean.so's kernels as the commit before this library built them (tools/kernel_resources.py): vgpr, agpr, sgpr, LDS, scratch.
# head_uncert.hip writes the forward contraction out again instead of sharing it, so these must not move.
HEAD_MEAN_KERNELS = {
    "_ZN12_GLOBAL__N_116head_mean_kernelILi1ELb0EEEvPKfS2_S2_fPviifii": (100, 16, 43, 43520, 0),
    "_ZN12_GLOBAL__N_116head_mean_kernelILi1ELb1EEEvPKfS2_S2_fPviifii": (100, 16, 45, 43520, 0),
    "_ZN12_GLOBAL__N_116head_mean_kernelILi2ELb0EEEvPKfS2_S2_fPviifii": (136, 32, 47, 52224, 0),
    "_ZN12_GLOBAL__N_116head_mean_kernelILi2ELb1EEEvPKfS2_S2_fPviifii": (136, 32, 49, 52224, 0),
}


def small_ae():
    from driving_dirty_amd.autoencoder import BasicAE
    return BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))


def build_model(cls, **extra):
    return cls(Namespace(pretrained_ae=small_ae(), unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, **extra))


def test_header_declares_the_one_launch_function_and_the_library_exports_exactly_it():
    from driving_dirty_amd import build, uncertainty
    signatures, streamed = header("dd_head_uncert.h")
    assert set(signatures) == FUNCTIONS and set(streamed) == FUNCTIONS, "a launch function (void* stream last)"
    assert uncertainty.SIGNATURES == signatures and uncertainty.STREAMED == streamed
    assert uncertainty.OPERANDS == {"dd_head_uncert": 13}
    assert uncertainty.BLOCK == 128 and "_bytes" not in open(build.UNCERTAINTY_EXTENSIONS["head_uncert"].header).read(), "a constant, no size query"
    entry = build.UNCERTAINTY_EXTENSIONS["head_uncert"]
    assert os.path.exists(entry.lib), "build the HIP libraries first (python __graft_entry__.py)"
    assert {n for n in exported_symbols(entry.lib) if n.startswith("dd_")} == FUNCTIONS


def test_no_other_library_or_header_knows_the_function():
    from driving_dirty_amd import build
    assert {n for n in exported_symbols(build.LIB) if n.startswith("dd_head_uncert")} == set(), "the main library's exports do not change"
    others = build.all_libraries()
    assert len(others) == 8 and "head_uncert" not in others
    for e in others.values():
        assert {n for n in exported_symbols(e.lib) if n.startswith("dd_head_uncert")} == set(), e.name
        assert "dd_head_uncert" not in open(e.header).read(), e.header
    assert "dd_head_uncert" not in open(build.HEADER).read()


def test_the_sixth_table():
    """``UNCERTAINTY_EXTENSIONS`` holds the one entry, made by the constructor of the others; the five older functions keep their values;
    ``built_libraries()`` is all six tables, and what the functions that take a name look it up in."""
    from driving_dirty_amd import build
    assert list(build.UNCERTAINTY_EXTENSIONS) == ["head_uncert"]
    assert list(build.extensions()) == list(build.EXTENSIONS) + list(build.OPTIMIZER_EXTENSIONS)
    assert list(build.libraries()) == list(build.extensions()) + list(build.PREDICTION_EXTENSIONS)
    assert list(build.every_library()) == list(build.libraries()) + list(build.TRAINING_EXTENSIONS)
    assert list(build.all_libraries()) == list(build.every_library()) + list(build.BOOTSTRAP_EXTENSIONS) and len(build.all_libraries()) == 8
    assert list(build.built_libraries()) == list(build.all_libraries()) + ["head_uncert"]
    e = build.UNCERTAINTY_EXTENSIONS["head_uncert"]
    assert isinstance(e, build.Extension) and e.name == "head_uncert" and e.sources == ["head_uncert.hip"] and e.what
    assert e.header == os.path.join(ROOT, "include", "dd_head_uncert.h") and e.lib == os.path.join(build.CSRC, "libdd_head_uncert.so")
    assert build.HEADER in e.headers and e.header in e.headers and all(os.path.exists(h) for h in e.headers)
    assert build.built_libraries()["head_uncert"] is e
    for fn in (build.extension_needs_build, build.build_extension):
        with pytest.raises(KeyError):
            fn("no_such_library")
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "b.UNCERTAINTY_EXTENSIONS" in text and "b.BOOTSTRAP_EXTENSIONS" in text and "b.extensions().values()" in text


def test_nothing_is_stale_after_a_build():
    from driving_dirty_amd import build
    assert build.build(force=False, verbose=False) == build.LIB
    assert not build.needs_build() and not build.extension_needs_build("head_uncert")
    assert build.build_extension("head_uncert", verbose=False) == build.UNCERTAINTY_EXTENSIONS["head_uncert"].lib


def test_the_kernels_use_no_scratch_and_no_spills():
    from driving_dirty_amd import build
    ks = kernel_resources().kernels(build.UNCERTAINTY_EXTENSIONS["head_uncert"].lib)
    assert len(ks) == 3, [k[".name"] for k in ks]      # one and two row tiles, and the finishing launch
    for k in ks:
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k[".name"]
        assert 0 < k[".group_segment_fixed_size"] <= 64 * 1024, k[".name"]      # static LDS: the operand tiles, which the epilogue reuses


def test_the_sampled_heads_own_kernels_did_not_move():
    from driving_dirty_amd import build
    ks = kernel_resources().kernels(build.PREDICTION_EXTENSIONS["head_mean"].lib)
    got = {k[".name"]: (k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])
           for k in ks}
    assert got == HEAD_MEAN_KERNELS
    assert "head_uncert" not in open(os.path.join(build.CSRC, "head_mean.hip")).read()


def test_one_binder_serves_this_library_too():
    from driving_dirty_amd import _lib, build, mc, uncertainty
    for name in ("lib", "launch", "last_error"):
        fn = vars(uncertainty)[name]      # module-level names, so that a monkeypatched ``launch`` takes effect
        assert isinstance(fn.__self__, _lib.Extension) and fn.__func__ is getattr(_lib.Extension, name)
    assert uncertainty.LIB == build.UNCERTAINTY_EXTENSIONS["head_uncert"].lib and "call" not in vars(uncertainty) and "size" not in vars(uncertainty)
    assert uncertainty.lib.__self__ is not mc.lib.__self__ and uncertainty.lib() is uncertainty.lib()
    with pytest.raises(uncertainty.HotpathError, match="operands given"):
        uncertainty.launch("dd_head_uncert", 1 << 20, 2 << 20, None, 3 << 20, 2, 4, 16, 8)
    with pytest.raises(uncertainty.HotpathError, match="not a function of include/dd_head_uncert.h"):
        uncertainty.launch("dd_head_mean_prob", 1 << 20, 2 << 20, None, 3 << 20, 2, 4, 16, 8)


def test_the_launcher_refuses_bad_arguments_without_a_gpu():
    from driving_dirty_amd import uncertainty
    lib = uncertainty.lib()
    M = 1 << 20      # never dereferenced: every call below is refused on the host
    base = dict(x=1 * M, w=2 * M, bias=3 * M, mean=4 * M, entropy=5 * M, mi=6 * M, var=7 * M, partials=8 * M, scores=9 * M, scenes=2, samples=4,
                n=16, k=8)

    def call(**kw):
        a = {**base, **kw}
        return lib.dd_head_uncert(a["x"], a["w"], a["bias"], a["mean"], a["entropy"], a["mi"], a["var"], a["partials"], a["scores"], a["scenes"],
                                  a["samples"], a["n"], a["k"], None)

    def refused(rc, *words):
        msg = uncertainty.last_error()
        assert rc != 0 and msg and "head_uncert" in msg and all(word in msg for word in words), (rc, msg)

    for name in ("x", "w"):
        refused(call(**{name: None}), "NULL")
    for bad in (dict(scenes=0), dict(scenes=-2), dict(n=0), dict(n=-16), dict(k=0), dict(k=-8)):
        refused(call(**bad), "non-positive")
    for bad in (0, 65, -1, 1 << 20):
        refused(call(samples=bad), "samples", str(bad))
    for bad in (6, 63, 513):
        refused(call(k=bad), "multiple of 4")
    for bad in (516, 1024, 940032):
        refused(call(k=bad), "splits K", str(bad))
    refused(call(scenes=1 << 16, n=1 << 15), "too large", "2^31")
    nothing = dict(mean=None, entropy=None, mi=None, var=None, partials=None, scores=None)
    refused(call(**nothing), "no output")
    refused(call(scores=None), "partials and scores")      # partials without scores
    refused(call(partials=None), "partials and scores")    # ... and the reverse
    for name in ("x", "w", "mean", "entropy", "mi", "var"):
        refused(call(**{name: base[name] + 8}), "16-byte")
    refused(call(bias=base["bias"] + 2), "bias", "4-byte")
    for name in ("partials", "scores"):
        refused(call(**{name: base[name] + 4}), "8-byte")
    for name in ("mean", "entropy", "mi", "var", "partials", "scores"):
        for other in ("x", "w", "bias"):
            refused(call(**{name: base[other]}), "overlaps", name, other)
    refused(call(mean=base["x"] + 2 * 4 * 8 * 4 - 16), "overlaps", "mean")      # the output begins inside the last 16 bytes of x
    refused(call(x=base["var"] + 16), "overlaps", "var")                        # ... and x begins inside an output
    refused(call(entropy=base["mean"] + 2 * 16 * 4 - 16), "overlaps", "mean", "entropy")      # two outputs
    refused(call(scores=base["partials"] + 8), "overlaps", "partials", "scores")
    refused(call(mi=base["var"], mean=None), "overlaps", "mi", "var")
    # a single output of any kind is a request
    for keep in ("mean", "entropy", "mi", "var"):
        refused(call(**{**nothing, keep: base[keep], "samples": 0}), "samples")


def test_head_uncertainty_checks_its_request_before_any_launch():
    from driving_dirty_amd import uncertainty
    assert uncertainty.MAPS == ("mean", "entropy", "mi", "var") and uncertainty.SCORES == ("entropy", "mi", "var")
    sig = inspect.signature(uncertainty.head_uncertainty)
    assert list(sig.parameters) == ["x", "weight", "bias", "samples", "maps", "scores"]
    assert sig.parameters["maps"].default == uncertainty.MAPS and sig.parameters["scores"].default is True
    with pytest.raises(ValueError, match="maps"):
        uncertainty.head_uncertainty(None, None, None, 4, maps=("mean", "median"))
    with pytest.raises(ValueError, match="twice"):
        uncertainty.head_uncertainty(None, None, None, 4, maps=("mi", "mi"))
    with pytest.raises(ValueError, match="no output"):
        uncertainty.head_uncertainty(None, None, None, 4, maps=(), scores=False)
    with pytest.raises(ValueError, match="samples"):
        uncertainty.head_uncertainty(None, None, None, 65)
    import torch
    with pytest.raises(uncertainty.HotpathError, match="device tensor"):
        uncertainty.head_uncertainty(torch.zeros((8, 8)), torch.zeros((16, 8)), None, 4)


def test_the_model_surface():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE
    sig = inspect.signature(RoadMapBCE.predict_uncertainty)
    assert list(sig.parameters) == ["self", "x", "mc_samples", "maps", "scores"]
    assert sig.parameters["mc_samples"].default is None and sig.parameters["maps"].default == ("mi",) and sig.parameters["scores"].default is True
    assert "tta_mirror" in RoadMapBCE.predict_uncertainty.__doc__ and "ignored" in RoadMapBCE.predict_uncertainty.__doc__
    assert not hasattr(RoadMap, "predict_uncertainty") and not hasattr(JointRoadMapBBox, "predict_uncertainty")
    assert not hasattr(build_model(RoadMap), "predict_uncertainty")
    import torch
    x = torch.zeros((1, 6, 3, 16, 22))
    for model, arg in ((build_model(RoadMapBCE), None), (build_model(RoadMapBCE), 1), (build_model(RoadMapBCE, mc_samples=8), 1)):
        with pytest.raises(ValueError, match="mc_samples"):
            model.predict_uncertainty(x, mc_samples=arg)
    with pytest.raises(ValueError, match="mc_samples"):
        build_model(RoadMapBCE).predict_uncertainty(x, mc_samples=65)


def test_the_flag_lives_in_hparams_and_only_one_model_takes_it(tmp_path):
    from driving_dirty_amd import uncertainty
    from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE
    parse = uncertainty.add_uncertainty_args(ArgumentParser(add_help=False)).parse_args
    assert vars(parse([])) == {"mc_uncertainty": False} and vars(parse(["--mc_uncertainty"])) == {"mc_uncertainty": True}
    assert uncertainty.enabled(Namespace()) is False and uncertainty.enabled(Namespace(mc_uncertainty=True)) is True
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="mc_uncertainty"):
            build_model(RoadMapBCE, mc_uncertainty=bad)
    with pytest.raises(ValueError, match="RoadMapBCE"):
        build_model(RoadMap, mc_uncertainty=True)
    build_model(RoadMap, mc_uncertainty=False)
    model, plain = build_model(RoadMapBCE, mc_samples=4, mc_uncertainty=True), build_model(RoadMapBCE)
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    path = str(tmp_path / "u.ckpt")
    model.save_checkpoint(path)
    assert RoadMapBCE.load_from_checkpoint(path).hparams.mc_uncertainty is True


def test_the_module_is_not_imported_until_it_is_asked_for():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); from argparse import Namespace\n"
            "from driving_dirty_amd.autoencoder import BasicAE\n"
            "from driving_dirty_amd import roadmap, joint, train\n"
            "ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))\n"
            "roadmap.RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, mc_samples=8))\n"
            "assert 'driving_dirty_amd.uncertainty' not in sys.modules\n" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)


def test_validation_epoch_end_averages_the_new_keys():
    import torch
    from driving_dirty_amd.roadmap import RoadMapBCE
    one, three = torch.tensor(1.0), torch.tensor(3.0)
    base = {"val_loss": one, "val_ts": one, "val_ts_rounded": one}
    extra = {"val_mc_entropy": one, "val_mc_mi": one, "val_mc_var": one}
    log = build_model(RoadMapBCE).validation_epoch_end([{**base, **extra}, {**base, **extra, "val_mc_mi": three}])["log"]
    assert float(log["avg_val_mc_mi"]) == 2.0 and float(log["avg_val_mc_entropy"]) == 1.0 and float(log["avg_val_mc_var"]) == 1.0
    assert set(build_model(RoadMapBCE).validation_epoch_end([base])["log"]) == {"avg_val_loss", "avg_val_ts_rounded", "avg_val_ts"}


def test_every_launch_function_of_the_library_has_a_guard_case():
    """The census of tests/test_guard_arena.py for this library: the case table imports without a GPU, names only the launch function of
    dd_head_uncert.h, and no case picks a kernel by alignment."""
    import test_gpu_guard_head_uncert as guard
    from driving_dirty_amd import uncertainty
    assert guard.CASES and len({c.name for c in guard.CASES}) == len(guard.CASES)
    assert {e for c in guard.CASES for e in c.entry} == set(uncertainty.STREAMED) == set(uncertainty.SIGNATURES)
    assert not any(c.picks_kernel_by_alignment or c.crosses for c in guard.CASES)
    assert len(guard.CASES) == len(guard.SHAPES) * len(guard.REQUESTS)
