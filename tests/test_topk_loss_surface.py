"""The bootstrapped road-map loss without a GPU: include/dd_topk_loss.h and the library built from it, the fifth table of build.py, the
launchers' host-side refusals, the binder it shares with the other extension libraries, the hparams' refusals in the three road-map
modules, and a model with the hparams absent."""
import os
import sys
from argparse import Namespace

import pytest

import _topk_loss_ref as ref
from _surface import ROOT, exported_symbols, header, kernel_resources

FUNCTIONS = {"dd_topk_bce", "dd_topk_bce_u8_ptrs"}
MODULE = "driving_dirty_amd.topk_loss"


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
    from driving_dirty_amd import build, topk_loss
    signatures, streamed = header("dd_topk_loss.h")
    assert set(signatures) == FUNCTIONS and set(streamed) == FUNCTIONS, "both are launch functions (void* stream last): no size query"
    assert topk_loss.SIGNATURES == signatures and topk_loss.STREAMED == streamed
    assert topk_loss.OPERANDS == {"dd_topk_bce": 12, "dd_topk_bce_u8_ptrs": 12}
    entry = build.BOOTSTRAP_EXTENSIONS["topk_loss"]
    assert os.path.exists(entry.lib), "build the HIP libraries first (python __graft_entry__.py)"
    assert {n for n in exported_symbols(entry.lib) if n.startswith("dd_")} == FUNCTIONS
    assert {n for n in exported_symbols(build.LIB) if n.startswith("dd_topk")} == set(), "the main library's exports do not change"


def test_the_functions_appear_in_no_other_header():
    from driving_dirty_amd import build
    others = [build.HEADER] + [e.header for e in build.every_library().values()]
    assert len(others) == 8
    for h in others:
        assert "dd_topk" not in open(h).read(), h
        assert not FUNCTIONS & set(header(os.path.basename(h))[0])


def test_the_fifth_table():
    """``BOOTSTRAP_EXTENSIONS`` holds the one entry, made by the constructor of the other seven; ``extensions()``, ``libraries()`` and
    ``every_library()`` keep their values; ``all_libraries()`` is all five tables, and what the functions that take a name look it up in."""
    from driving_dirty_amd import build
    assert list(build.BOOTSTRAP_EXTENSIONS) == ["topk_loss"]
    assert list(build.extensions()) == list(build.EXTENSIONS) + list(build.OPTIMIZER_EXTENSIONS)
    assert list(build.libraries()) == list(build.extensions()) + list(build.PREDICTION_EXTENSIONS)
    assert list(build.every_library()) == list(build.libraries()) + list(build.TRAINING_EXTENSIONS) and "topk_loss" not in build.every_library()
    assert list(build.all_libraries()) == list(build.every_library()) + ["topk_loss"] and len(build.all_libraries()) == 8
    e = build.BOOTSTRAP_EXTENSIONS["topk_loss"]
    assert isinstance(e, build.Extension) and e.name == "topk_loss" and e.sources == ["topk_loss.hip"] and e.what == "the bootstrapped road-map loss"
    assert e.header == os.path.join(ROOT, "include", "dd_topk_loss.h") and e.lib == os.path.join(build.CSRC, "libdd_topk_loss.so")
    assert build.HEADER in e.headers and e.header in e.headers and all(os.path.exists(h) for h in e.headers)
    assert os.path.join(build.CSRC, "dd_loss_stats.h") in e.headers, "the reductions it shares with the other losses"
    assert build.all_libraries()["topk_loss"] is e
    for fn in (build.extension_needs_build, build.build_extension):
        with pytest.raises(KeyError):
            fn("no_such_library")
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "b.extensions().values()" in text and "b.PREDICTION_EXTENSIONS" in text and "b.TRAINING_EXTENSIONS" in text
    assert "b.BOOTSTRAP_EXTENSIONS" in text


def test_nothing_is_stale_after_a_build(monkeypatch):
    from driving_dirty_amd import build
    assert build.build(force=False, verbose=False) == build.LIB
    assert not build.needs_build() and not build.extension_needs_build("topk_loss")
    entry = build.BOOTSTRAP_EXTENSIONS["topk_loss"]
    assert build.build_extension("topk_loss", verbose=False) == entry.lib
    # forced: one compile with the main library's flags, one link against it (``build._run`` records instead of running)
    commands = []
    monkeypatch.setattr(build, "_run", lambda cmd, verbose: commands.append(cmd))
    assert build.build_extension("topk_loss", force=True, verbose=False) == entry.lib
    compile_, link = commands
    obj = os.path.join(build.OBJ, "topk_loss.o")
    assert compile_[1:] == build.FLAGS + ["-c", os.path.join(build.CSRC, "topk_loss.hip"), "-o", obj]
    assert link[1:] == ["--offload-arch=gfx950", "-shared", "-fPIC", "-o", entry.lib, obj, "-L" + build.CSRC, "-l:libdd_hotpath.so", "-Wl,-rpath,$ORIGIN"]


def test_the_kernels_use_no_scratch_and_no_spills():
    from driving_dirty_amd import build
    ks = kernel_resources().kernels(build.BOOTSTRAP_EXTENSIONS["topk_loss"].lib)
    names = [k[".name"] for k in ks]
    # per target form: three histogram passes, the final pass with and without the gradient; and the three small launches
    assert len(ks) == 13, names
    assert sum("topk_hist_kernel" in n for n in names) == 6 and sum("topk_final_kernel" in n for n in names) == 4
    assert sum("topk_init_kernel" in n for n in names) == 1 and sum("topk_select_kernel" in n for n in names) == 1
    assert sum("topk_finish_kernel" in n for n in names) == 1
    for k in ks:
        assert k[".private_segment_fixed_size"] == 0, k[".name"]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k[".name"]
        # the streams hide their loads behind other waves: eight per SIMD in the histogram passes, seven at least in the final pass
        if "topk_hist_kernel" in k[".name"]:
            assert k[".vgpr_count"] <= 64, (k[".name"], k[".vgpr_count"])
        if "topk_final_kernel" in k[".name"]:
            assert k[".vgpr_count"] <= 72, (k[".name"], k[".vgpr_count"])
        if "topk_hist_kernel" in k[".name"]:
            assert k[".group_segment_fixed_size"] <= 8192, k[".name"]          # the 11-bit digit's counters


def test_the_binder_is_the_extension_binder():
    from driving_dirty_amd import _lib, build, consistency, topk_loss
    for name in ("lib", "launch", "last_error"):
        fn = vars(topk_loss)[name]      # module-level names, so that a monkeypatched ``launch`` takes effect
        assert isinstance(fn.__self__, _lib.Extension) and fn.__func__ is getattr(_lib.Extension, name)
        assert fn.__self__ is topk_loss.lib.__self__
    assert topk_loss.LIB == build.BOOTSTRAP_EXTENSIONS["topk_loss"].lib and "call" not in vars(topk_loss) and "size" not in vars(topk_loss)
    assert topk_loss.lib.__self__ is not consistency.lib.__self__ and topk_loss.lib() is topk_loss.lib()
    text = open(os.path.join(ROOT, "include", "dd_topk_loss.h")).read()
    assert f"#define DD_TOPK_CHUNK {topk_loss.CHUNK}" in text and topk_loss.CHUNK % 1024 == 0
    assert f"#define DD_TOPK_TABLE_MAX {topk_loss.TABLE_MAX}" in text and topk_loss.TABLE_MAX == 64
    with pytest.raises(topk_loss.HotpathError, match="operands given"):
        topk_loss.launch("dd_topk_bce", None, None, 1, 4, 1)
    with pytest.raises(topk_loss.HotpathError, match="not a function of include/dd_topk_loss.h"):
        topk_loss.launch("dd_cons_fwd", None, None, 1, 1, 4, None, None, None, 0)


@pytest.mark.parametrize("batch,per", [(1, 4), (2, ref.CHUNK + 4), (32, 640000)])
def test_workspace_bytes_is_the_headers_formula(batch, per):
    from driving_dirty_amd import topk_loss
    pieces = -(-per // ref.CHUNK)
    assert topk_loss.workspace_bytes(batch, per) == ref.header_workspace_bytes(batch, per) == batch * (24 * pieces + 4 * 5120 + 16)
    assert (topk_loss.CHUNK, topk_loss.BINS, topk_loss.PIECE_BYTES, topk_loss.STATE_BYTES) == (ref.CHUNK, ref.BINS, ref.PIECE_BYTES, ref.STATE_BYTES)
    assert topk_loss.workspace_bytes(batch, per) % 8 == 0


def test_launchers_refuse_bad_arguments_without_a_gpu():
    import ctypes as C
    from driving_dirty_amd import topk_loss
    lib = topk_loss.lib()
    M = 1 << 24      # never dereferenced: every call below is refused on the host
    Z, T, P, D, L, S, WS = 1 * M, 2 * M, 3 * M, 4 * M, 5 * M, 6 * M, 7 * M
    nan, inf = float("nan"), float("inf")
    need = topk_loss.workspace_bytes(2, 8)

    def refused(rc, *words):
        msg = topk_loss.last_error()
        assert rc != 0 and msg and all(w in msg for w in words), (rc, msg, words)

    def stacked(z=Z, t=T, batch=2, per=8, keep=3, gs=1.0, probs=P, dz=D, loss=L, stats=S, ws=WS, ws_bytes=need):
        return lib.dd_topk_bce(z, t, batch, per, keep, gs, probs, dz, loss, stats, ws, ws_bytes, None)

    def table(z=Z, t=(T, T + 64), batch=2, per=8, keep=3, gs=1.0, probs=P, dz=D, loss=L, stats=S, ws=WS, ws_bytes=need):
        ptrs = None if t is None else (C.c_void_p * len(t))(*t)
        return lib.dd_topk_bce_u8_ptrs(z, ptrs, batch, per, keep, gs, probs, dz, loss, stats, ws, ws_bytes, None)

    for fn, who in ((stacked, "topk_bce:"), (table, "topk_bce_u8_ptrs:")):
        for name, kw, base, align in (("logits", "z", Z, "16-byte"), ("loss_out", "loss", L, "4-byte"), ("stats", "stats", S, "8-byte"),
                                      ("workspace", "ws", WS, "8-byte")):
            refused(fn(**{kw: None}), who, name, "NULL")
            refused(fn(**{kw: base + 2}), who, name, align)
        refused(fn(z=Z + 8), who, "logits", "16-byte")
        refused(fn(probs=P + 4), who, "probs", "16-byte")
        refused(fn(dz=D + 8), who, "dlogits", "16-byte")
        refused(fn(stats=S + 4), who, "stats", "8-byte")
        refused(fn(batch=0), who, "batch", "positive")
        refused(fn(per=0), who, "positive")
        refused(fn(per=6, keep=1), who, "multiple of 4")
        refused(fn(per=1 << 31, keep=1, ws_bytes=1 << 50), who, "2^31")
        refused(fn(batch=1 << 11, per=1 << 30, keep=1, ws_bytes=1 << 50), who, "2^40")
        for keep in (0, -1, 9):
            refused(fn(keep=keep), who, "keep", "1 .. per_sample = 8")
        for bad in (nan, inf, -inf):
            refused(fn(gs=bad), who, "grad_scale", "finite")
        refused(fn(ws_bytes=need - 1), who, "workspace_bytes", str(need))
        big = topk_loss.workspace_bytes(2, topk_loss.CHUNK + 4)
        refused(fn(per=topk_loss.CHUNK + 4, ws_bytes=big - 1), who, "workspace_bytes", str(big))
        refused(fn(probs=Z), who, "probs overlaps logits")
        refused(fn(probs=Z + 2 * 8 * 4 - 16), who, "probs overlaps logits")      # begins inside the last vector
        refused(fn(dz=Z), who, "dlogits overlaps logits")
        refused(fn(dz=P + 16), who, "probs overlaps dlogits")
    refused(stacked(t=None), "topk_bce:", "target", "NULL")
    refused(stacked(t=T + 2), "topk_bce:", "target", "4-byte")
    refused(table(t=None), "topk_bce_u8_ptrs:", "target_ptrs", "NULL")
    refused(table(t=(T, 0)), "topk_bce_u8_ptrs:", "target_ptrs[1]", "NULL")
    refused(table(t=(T, T + 66)), "topk_bce_u8_ptrs:", "target_ptrs[1]", "4-byte")
    refused(table(t=(T,) * 65, batch=65, ws_bytes=topk_loss.workspace_bytes(65, 8)), "topk_bce_u8_ptrs:", "at most 64")


def test_python_refusals_name_the_operand():
    import torch
    from driving_dirty_amd import topk_loss
    with pytest.raises(topk_loss.HotpathError, match=r"\[B, P\]"):
        topk_loss.fwd(torch.zeros(2, 2, 4), torch.zeros(2, 2, 4, dtype=torch.uint8), 1)
    with pytest.raises(topk_loss.HotpathError, match="no empty dimension"):
        topk_loss.fwd(torch.zeros(0, 4), torch.zeros(0, 4, dtype=torch.uint8), 1)
    with pytest.raises(topk_loss.HotpathError, match="logits"):      # a host tensor never reaches a launcher
        topk_loss.fwd(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.uint8), 1)


def test_the_hparams_are_checked():
    from driving_dirty_amd import topk_loss
    from driving_dirty_amd.roadmap import topk_config
    assert topk_config(None) is None and topk_config(Namespace()) is None and topk_config(Namespace(rm_topk_frac=1.0, rm_topk_warmup_steps=0)) is None
    assert topk_config(Namespace(rm_topk_frac=1, rm_topk_warmup_steps=50)) is None and topk_config(Namespace(rm_topk_frac=None)) is None
    assert topk_config(Namespace(rm_topk_frac=0.25)) == (0.25, 0) and topk_config(Namespace(rm_topk_frac="0.5", rm_topk_warmup_steps=50)) == (0.5, 50)
    assert topk_loss.check_hparams(Namespace()) == (1.0, 0)
    RoadMapBCE, RoadMap, Joint = road_map_models()
    for bad in (dict(rm_topk_frac=0.0), dict(rm_topk_frac=-0.5), dict(rm_topk_frac=1.5), dict(rm_topk_frac=float("nan")), dict(rm_topk_frac="x"),
                dict(rm_topk_frac=0.5, rm_topk_warmup_steps=-1), dict(rm_topk_warmup_steps=-1)):
        for cls in (RoadMapBCE, RoadMap, Joint):
            with pytest.raises(ValueError, match="rm_topk_"):
                tiny(cls, **bad)
    on = tiny(RoadMapBCE, rm_topk_frac=0.25, rm_topk_warmup_steps=10)
    assert on.topk == (0.25, 10) and on.topk_step == 0
    assert tiny(RoadMapBCE, rm_topk_frac=1.0).topk is None
    parser = topk_loss.add_topk_args(__import__("argparse").ArgumentParser())
    assert vars(parser.parse_args([])) == {"rm_topk_frac": 1.0, "rm_topk_warmup_steps": 0}
    assert vars(parser.parse_args(["--rm_topk_frac", "0.25", "--rm_topk_warmup_steps", "400"])) == {"rm_topk_frac": 0.25, "rm_topk_warmup_steps": 400}


def test_the_other_road_map_modules_refuse_the_flag():
    RoadMapBCE, RoadMap, Joint = road_map_models()
    with pytest.raises(ValueError, match=r"rm_topk_frac.*RoadMap .roadmap_mse."):
        tiny(RoadMap, rm_topk_frac=0.5)
    with pytest.raises(ValueError, match="rm_topk_frac.*JointRoadMapBBox"):
        tiny(Joint, rm_topk_frac=0.5)
    assert tiny(RoadMap, rm_topk_frac=1.0).topk is None and tiny(Joint, rm_topk_frac=1.0) is not None


@pytest.mark.parametrize("rm", [dict(rm_pos_weight="auto"), dict(rm_pos_weight=2.0), dict(rm_ts_weight=0.5), dict(rm_bce_weight=0.5)])
def test_the_combination_with_an_rm_setting_is_refused_by_name(rm):
    RoadMapBCE = road_map_models()[0]
    with pytest.raises(ValueError, match="rm_topk_frac.*rm_pos_weight / rm_bce_weight / rm_ts_weight"):
        tiny(RoadMapBCE, rm_topk_frac=0.5, **rm)
    assert tiny(RoadMapBCE, rm_topk_frac=1.0, **rm).rm_loss is not None
    assert tiny(RoadMapBCE, rm_topk_frac=0.5, cons_weight=0.5).topk == (0.5, 0), "with cons_weight it composes"


def test_a_checkpoint_carries_the_two_hparams(tmp_path):
    RoadMapBCE = road_map_models()[0]
    model = tiny(RoadMapBCE, rm_topk_frac=0.25, rm_topk_warmup_steps=400)
    model.topk_step = 7
    path = str(tmp_path / "topk.ckpt")
    model.save_checkpoint(path)
    again = RoadMapBCE.load_from_checkpoint(path)
    assert again.topk == model.topk == (0.25, 400) and (again.hparams.rm_topk_frac, again.hparams.rm_topk_warmup_steps) == (0.25, 400)
    assert again.topk_step == 0, "the anneal's step is not checkpointed: a resumed run restarts it"


def test_a_model_with_the_setting_off_never_imports_the_module(tmp_path):
    """Building the three modules, their parsers, a checkpoint and its reload with ``rm_topk_frac`` absent or 1 leaves
    ``driving_dirty_amd.topk_loss`` out of ``sys.modules``; with a fraction below 1 the constructor imports it to check the values."""
    from argparse import ArgumentParser
    import driving_dirty_amd
    saved, had_attr = sys.modules.pop(MODULE, None), hasattr(driving_dirty_amd, "topk_loss")
    attr = getattr(driving_dirty_amd, "topk_loss", None)
    if had_attr:
        del driving_dirty_amd.topk_loss      # ``from . import topk_loss`` would take the attribute and import nothing
    try:
        for cls in road_map_models():
            cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([])
            for hp in ({}, dict(rm_topk_frac=1.0, rm_topk_warmup_steps=0), dict(rm_topk_frac=1)):
                model = tiny(cls, **hp)
            path = str(tmp_path / (cls.__name__ + ".ckpt"))
            model.save_checkpoint(path)
            cls.load_from_checkpoint(path)
        assert MODULE not in sys.modules
        assert tiny(road_map_models()[0], rm_topk_frac=0.5).topk == (0.5, 0)
        assert MODULE in sys.modules
    finally:
        if saved is not None:
            sys.modules[MODULE] = saved
        if had_attr:
            driving_dirty_amd.topk_loss = attr
