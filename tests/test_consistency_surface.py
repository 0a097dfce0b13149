"""The mirror consistency loss without a GPU: include/dd_consistency.h and the library built from it, the fourth table of build.py, the
launchers' host-side refusals, the binder it shares with the other extension libraries, the hparams' refusals in the three road-map
modules, and a model with the hparams absent."""
import os
import sys
from argparse import Namespace

import pytest

from _surface import ROOT, exported_symbols, header, kernel_resources

FUNCTIONS = {"dd_cons_fwd", "dd_cons_fwd_grad"}
MODULE = "driving_dirty_amd.consistency"


def road_map_models():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE
    return RoadMapBCE, RoadMap, JointRoadMapBBox


def tiny(cls, **hp):
    from driving_dirty_amd.autoencoder import BasicAE
    small = cls.__name__ != "JointRoadMapBBox"      # the joint model's heads fix the reference's view size
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, **(dict(input_height=16, input_width=132) if small else {})))
    return cls(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, **hp))


def test_header_declares_the_two_launch_functions_and_the_library_exports_exactly_them():
    from driving_dirty_amd import build, consistency
    signatures, streamed = header("dd_consistency.h")
    assert set(signatures) == FUNCTIONS and set(streamed) == FUNCTIONS, "both are launch functions (void* stream last): no size query"
    assert consistency.SIGNATURES == signatures and consistency.STREAMED == streamed
    assert consistency.OPERANDS == {"dd_cons_fwd": 9, "dd_cons_fwd_grad": 12}
    entry = build.TRAINING_EXTENSIONS["consistency"]
    assert os.path.exists(entry.lib), "build the HIP libraries first (python __graft_entry__.py)"
    assert {n for n in exported_symbols(entry.lib) if n.startswith("dd_")} == FUNCTIONS
    assert {n for n in exported_symbols(build.LIB) if n.startswith("dd_cons")} == set(), "the main library's exports do not change"


def test_the_functions_appear_in_no_other_header():
    from driving_dirty_amd import build
    others = [build.HEADER] + [e.header for e in build.libraries().values()]
    assert len(others) == 7
    for h in others:
        assert "dd_cons" not in open(h).read(), h
        assert not FUNCTIONS & set(header(os.path.basename(h))[0])


def test_the_fourth_table():
    """``TRAINING_EXTENSIONS`` holds the one entry, made by the constructor of the other six; ``extensions()`` and ``libraries()`` keep their
    values; ``every_library()`` is all four tables, and what the functions that take a name look it up in."""
    from driving_dirty_amd import build
    assert list(build.TRAINING_EXTENSIONS) == ["consistency"]
    assert list(build.extensions()) == list(build.EXTENSIONS) + list(build.OPTIMIZER_EXTENSIONS)
    assert list(build.libraries()) == list(build.extensions()) + list(build.PREDICTION_EXTENSIONS) and "consistency" not in build.libraries()
    assert list(build.every_library()) == list(build.libraries()) + ["consistency"]
    e = build.TRAINING_EXTENSIONS["consistency"]
    assert isinstance(e, build.Extension) and e.name == "consistency" and e.sources == ["consistency.hip"] and e.what == "the consistency loss"
    assert e.header == os.path.join(ROOT, "include", "dd_consistency.h") and e.lib == os.path.join(build.CSRC, "libdd_consistency.so")
    assert build.HEADER in e.headers and e.header in e.headers and all(os.path.exists(h) for h in e.headers)
    assert os.path.join(build.CSRC, "dd_loss_stats.h") in e.headers, "the reduction it shares with the two other losses"
    assert build.every_library()["consistency"] is e
    with pytest.raises(KeyError):
        build.extension_needs_build("no_such_library")
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "b.extensions().values()" in text and "b.PREDICTION_EXTENSIONS" in text and "b.TRAINING_EXTENSIONS" in text


def test_nothing_is_stale_after_a_build(monkeypatch):
    from driving_dirty_amd import build
    assert build.build(force=False, verbose=False) == build.LIB
    assert not build.needs_build() and not build.extension_needs_build("consistency")
    entry = build.TRAINING_EXTENSIONS["consistency"]
    assert build.build_extension("consistency", verbose=False) == entry.lib
    # forced: one compile with the main library's flags, one link against it (``build._run`` records instead of running)
    commands = []
    monkeypatch.setattr(build, "_run", lambda cmd, verbose: commands.append(cmd))
    assert build.build_extension("consistency", force=True, verbose=False) == entry.lib
    compile_, link = commands
    obj = os.path.join(build.OBJ, "consistency.o")
    assert compile_[1:] == build.FLAGS + ["-c", os.path.join(build.CSRC, "consistency.hip"), "-o", obj]
    assert link[1:] == ["--offload-arch=gfx950", "-shared", "-fPIC", "-o", entry.lib, obj, "-L" + build.CSRC, "-l:libdd_hotpath.so", "-Wl,-rpath,$ORIGIN"]


def test_the_kernels_use_no_scratch_and_no_spills():
    from driving_dirty_amd import build
    ks = kernel_resources().kernels(build.TRAINING_EXTENSIONS["consistency"].lib)
    assert len(ks) == 5, [k[".name"] for k in ks]      # the pass with and without the gradient on both paths, one finishing kernel
    assert sum("cons_kernel" in k[".name"] for k in ks) == 4 and sum("cons_final_kernel" in k[".name"] for k in ks) == 1
    for k in ks:
        assert k[".private_segment_fixed_size"] == 0, k[".name"]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k[".name"]
        if "cons_kernel" in k[".name"]:
            assert k[".vgpr_count"] <= 128, (k[".name"], k[".vgpr_count"])      # four waves per SIMD: the pass hides its loads behind other waves


def test_the_binder_is_the_extension_binder():
    from driving_dirty_amd import _lib, build, consistency, rm_loss
    for name in ("lib", "launch", "last_error"):
        fn = vars(consistency)[name]      # module-level names, so that a monkeypatched ``launch`` takes effect
        assert isinstance(fn.__self__, _lib.Extension) and fn.__func__ is getattr(_lib.Extension, name)
        assert fn.__self__ is consistency.lib.__self__
    assert consistency.LIB == build.TRAINING_EXTENSIONS["consistency"].lib and "call" not in vars(consistency) and "size" not in vars(consistency)
    assert consistency.lib.__self__ is not rm_loss.lib.__self__ and consistency.lib() is consistency.lib()
    text = open(os.path.join(ROOT, "include", "dd_consistency.h")).read()
    assert f"#define DD_CONS_CHUNK {consistency.CHUNK}" in text and consistency.CHUNK % 1024 == 0
    with pytest.raises(consistency.HotpathError, match="operands given"):
        consistency.launch("dd_cons_fwd", None, None, 1, 1, 4, None, None, None)
    with pytest.raises(consistency.HotpathError, match="not a function of include/dd_consistency.h"):
        consistency.launch("dd_tta_mean_prob", None, None, None, 1, 1, 4, 0)


def test_launchers_refuse_bad_arguments_without_a_gpu():
    from driving_dirty_amd import consistency
    lib = consistency.lib()
    M = 1 << 24      # never dereferenced: every call below is refused on the host
    A, MM, DA, DM, L, S, WS = 1 * M, 2 * M, 3 * M, 4 * M, 5 * M, 6 * M, 7 * M
    nan, inf = float("nan"), float("inf")

    def refused(rc, *words):
        msg = consistency.last_error()
        assert rc != 0 and msg and all(w in msg for w in words), (rc, msg, words)

    def fwd(a=A, m=MM, batch=2, h=3, w=8, loss=L, stats=S, ws=WS, ws_bytes=32):
        return lib.dd_cons_fwd(a, m, batch, h, w, loss, stats, ws, ws_bytes, None)

    def grad(a=A, m=MM, batch=2, h=3, w=8, gs=1.0, da=DA, dm=DM, loss=L, stats=S, ws=WS, ws_bytes=32):
        return lib.dd_cons_fwd_grad(a, m, batch, h, w, gs, da, dm, loss, stats, ws, ws_bytes, None)

    for fn, who in ((fwd, "cons_fwd:"), (grad, "cons_fwd_grad:")):
        for name, kw, base, align in (("a", "a", A, "4-byte"), ("m", "m", MM, "4-byte"), ("loss", "loss", L, "4-byte"), ("stats", "stats", S, "8-byte"),
                                      ("workspace", "ws", WS, "8-byte")):
            refused(fn(**{kw: None}), who, name, "NULL")
            refused(fn(**{kw: base + 2}), who, name, align)
        refused(fn(stats=S + 4), who, "stats", "8-byte")
        refused(fn(batch=0), who, "batch", "positive")
        refused(fn(h=0), who, "positive")
        refused(fn(w=-4), who, "positive")
        refused(fn(h=1 << 16, w=1 << 15, ws_bytes=1 << 40), who, "2^31")
        refused(fn(batch=1 << 11, h=1 << 15, w=1 << 15, ws_bytes=1 << 40), who, "2^40")
        refused(fn(ws_bytes=31), who, "workspace_bytes", "32")
        refused(fn(h=1, w=consistency.CHUNK + 4, ws_bytes=63), who, "workspace_bytes", "64")
    for name, kw, base in (("da", "da", DA), ("dm", "dm", DM)):
        refused(grad(**{kw: None}), "cons_fwd_grad:", name, "NULL")
        refused(grad(**{kw: base + 1}), "cons_fwd_grad:", name, "4-byte")
        refused(grad(**{kw: A}), "cons_fwd_grad:", name, "overlaps an input")
        refused(grad(**{kw: MM + 2 * 3 * 8 * 4 - 4}), "cons_fwd_grad:", name, "overlaps an input")      # begins inside the last element
    refused(grad(dm=DA + 16), "cons_fwd_grad:", "da overlaps dm")
    for bad in (nan, inf, -inf):
        refused(grad(gs=bad), "cons_fwd_grad:", "grad_scale", "finite")


def test_python_refusals_name_the_operand():
    import torch
    from driving_dirty_amd import consistency
    with pytest.raises(consistency.HotpathError, match="fp32"):
        consistency.mirror_consistency(torch.zeros(2, 2, 4, dtype=torch.float64))
    with pytest.raises(consistency.HotpathError, match=r"\[2B,h,w\]"):
        consistency.mirror_consistency(torch.zeros(3, 2, 4))
    with pytest.raises(consistency.HotpathError, match=r"\[2B,h,w\]"):
        consistency.mirror_consistency(torch.zeros(2, 0, 4))
    with pytest.raises(consistency.HotpathError, match=r"\[2B,h,w\]"):
        consistency.mirror_consistency(torch.zeros(2, 8))
    with pytest.raises(consistency.HotpathError, match="logits"):      # a host tensor never reaches a launcher
        consistency.mirror_consistency(torch.zeros(2, 2, 4))
    with pytest.raises(consistency.HotpathError, match="no empty dimension"):
        consistency.fwd(torch.zeros(0, 2, 4), torch.zeros(0, 2, 4))
    with pytest.raises(consistency.HotpathError, match="consistency.fwd_grad: a: expected a contiguous fp32"):
        consistency.fwd_grad(torch.zeros(1, 2, 4, dtype=torch.bfloat16), torch.zeros(1, 2, 4))


def test_the_hparams_are_refused_where_they_cannot_be_served():
    from driving_dirty_amd.roadmap import cons_config
    RoadMapBCE, RoadMap, Joint = road_map_models()
    assert cons_config(None) is None and cons_config(Namespace()) is None and cons_config(Namespace(cons_weight=0.0, cons_rampup_steps=0)) is None
    assert cons_config(Namespace(cons_weight=0.0, cons_rampup_steps=50)) is None and cons_config(Namespace(cons_weight=None)) is None
    assert cons_config(Namespace(cons_weight=0.5)) == (0.5, 0) and cons_config(Namespace(cons_weight=2, cons_rampup_steps=50)) == (2.0, 50)
    for bad in (dict(cons_weight=-1.0), dict(cons_weight=float("nan")), dict(cons_weight=float("inf")), dict(cons_weight=1.0, cons_rampup_steps=-1),
                dict(cons_rampup_steps=-1)):
        for cls in (RoadMapBCE, RoadMap, Joint):
            with pytest.raises(ValueError, match="cons_"):
                tiny(cls, **bad)
    on = tiny(RoadMapBCE, cons_weight=0.5, cons_rampup_steps=10)
    assert on.cons == (0.5, 10) and on.cons_step == 0
    assert tiny(RoadMapBCE, cons_weight=0.0).cons is None
    with pytest.raises(ValueError, match="RoadMap .roadmap_mse."):
        tiny(RoadMap, cons_weight=0.5)
    with pytest.raises(ValueError, match="JointRoadMapBBox"):
        tiny(Joint, cons_weight=0.5)
    assert tiny(RoadMap, cons_weight=0.0).cons is None and tiny(Joint, cons_weight=0.0) is not None
    # a batch with an unlabelled part under cons_weight 0: refused before anything is looked at
    with pytest.raises(ValueError, match="cons_weight is 0"):
        tiny(RoadMapBCE).training_step((None, None, None, None), 0)


def test_a_checkpoint_carries_the_two_hparams(tmp_path):
    RoadMapBCE = road_map_models()[0]
    model = tiny(RoadMapBCE, cons_weight=0.5, cons_rampup_steps=400)
    model.cons_step = 7
    path = str(tmp_path / "cons.ckpt")
    model.save_checkpoint(path)
    again = RoadMapBCE.load_from_checkpoint(path)
    assert again.cons == model.cons == (0.5, 400) and (again.hparams.cons_weight, again.hparams.cons_rampup_steps) == (0.5, 400)
    assert again.cons_step == 0, "the ramp's step is not checkpointed: a resumed run restarts it"


def test_a_model_with_the_hparams_absent_never_imports_the_module(tmp_path):
    """Building the three modules, their parsers, a checkpoint and its reload with ``cons_weight`` absent or 0 leaves
    ``driving_dirty_amd.consistency`` out of ``sys.modules``; with a positive weight the constructor imports it to check the values."""
    from argparse import ArgumentParser
    import driving_dirty_amd
    saved, had_attr = sys.modules.pop(MODULE, None), hasattr(driving_dirty_amd, "consistency")
    attr = getattr(driving_dirty_amd, "consistency", None)
    if had_attr:
        del driving_dirty_amd.consistency      # ``from . import consistency`` would take the attribute and import nothing
    try:
        for cls in road_map_models():
            cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([])
            for hp in ({}, dict(cons_weight=0.0, cons_rampup_steps=0)):
                model = tiny(cls, **hp)
            path = str(tmp_path / (cls.__name__ + ".ckpt"))
            model.save_checkpoint(path)
            cls.load_from_checkpoint(path)
        assert MODULE not in sys.modules
        assert tiny(road_map_models()[0], cons_weight=0.5).cons == (0.5, 0)
        assert MODULE in sys.modules
    finally:
        if saved is not None:
            sys.modules[MODULE] = saved
        if had_attr:
            driving_dirty_amd.consistency = attr
