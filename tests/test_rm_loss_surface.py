"""The road-map loss without a GPU: include/dd_rm_loss.h and the library built from it, the launchers' host-side refusals, the binder
it shares with the other extension libraries, the command line of the three road-map modules, and a model with the flags off."""
import ctypes as C
import os
import sys
from argparse import ArgumentParser, Namespace

import pytest

from _surface import ROOT, exported_symbols, header, kernel_resources

FUNCTIONS = {"dd_rm_loss_fwd", "dd_rm_loss_fwd_u8_ptrs", "dd_rm_loss_bwd", "dd_rm_loss_bwd_u8_ptrs"}
FLAGS_OFF = dict(rm_pos_weight=None, rm_bce_weight=1.0, rm_ts_weight=0.0, rm_ts_eps=1.0)


def road_map_models():
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE
    return RoadMapBCE, RoadMap, JointRoadMapBBox


def tiny(cls, **hp):
    from driving_dirty_amd.autoencoder import BasicAE
    small = cls.__name__ != "JointRoadMapBBox"      # the joint model's heads fix the reference's view size
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, **(dict(input_height=16, input_width=132) if small else {})))
    return cls(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, **hp))


def test_header_declares_the_four_launch_functions_and_the_library_exports_exactly_them():
    from driving_dirty_amd import build, rm_loss
    entry = build.EXTENSIONS["rm_loss"]
    signatures, streamed = header("dd_rm_loss.h")
    assert set(signatures) == FUNCTIONS and set(streamed) == FUNCTIONS, "all four are launch functions (void* stream last): no size query"
    assert rm_loss.SIGNATURES == signatures and rm_loss.STREAMED == streamed
    assert rm_loss.OPERANDS == {"dd_rm_loss_fwd": 15, "dd_rm_loss_fwd_u8_ptrs": 14, "dd_rm_loss_bwd": 8, "dd_rm_loss_bwd_u8_ptrs": 7}
    assert os.path.exists(entry.lib), "build the HIP libraries first (python __graft_entry__.py)"
    assert {n for n in exported_symbols(entry.lib) if n.startswith("dd_")} == FUNCTIONS
    assert build.build(force=False, verbose=False) == build.LIB and not build.needs_build()
    assert build.build_extension("rm_loss", verbose=False) == entry.lib
    assert entry.sources == ["rm_loss.hip"] and entry.header in entry.headers


def test_the_constants_are_the_headers():
    from driving_dirty_amd import ops, rm_loss
    text = open(os.path.join(ROOT, "include", "dd_rm_loss.h")).read()
    assert f"#define DD_RM_LOSS_CHUNK {rm_loss.CHUNK}" in text and f"#define DD_RM_LOSS_TABLE_MAX {rm_loss.TABLE_MAX}" in text
    assert "#define DD_RM_POS_WEIGHT_AUTO (-1.0f)" in text and rm_loss.POS_WEIGHT_AUTO == -1.0 == ops.POS_WEIGHT_AUTO
    assert rm_loss.CHUNK % 1024 == 0 and rm_loss.ACC_TERMS == rm_loss.CHUNK // 256
    assert rm_loss.TABLE_MAX == 64 == ops.PTR_TABLE_MAX      # the models' per-sample branch hands over what fits either table
    hot = open(os.path.join(ROOT, "include", "dd_hotpath.h")).read()
    assert "enum { DD_TARGET_F32 = 0, DD_TARGET_U8 = 1 };" in hot and (rm_loss.TARGET_F32, rm_loss.TARGET_U8) == (0, 1)
    assert rm_loss.workspace_bytes(1, 4) == 40 and rm_loss.workspace_bytes(3, rm_loss.CHUNK + 4) == 3 * 2 * 40
    assert rm_loss.workspace_bytes(32, 640000) == 32 * 79 * 40 if rm_loss.CHUNK == 8192 else True


def test_the_binder_is_the_extension_binder():
    from driving_dirty_amd import _lib, build, ema, rm_loss
    for name in ("lib", "launch", "last_error"):
        fn = vars(rm_loss)[name]      # module-level names, so that a monkeypatched ``launch`` takes effect
        assert isinstance(fn.__self__, _lib.Extension) and fn.__func__ is getattr(_lib.Extension, name)
        assert fn.__self__ is rm_loss.lib.__self__
    assert rm_loss.LIB == build.EXTENSIONS["rm_loss"].lib and "call" not in vars(rm_loss) and "size" not in vars(rm_loss)
    assert rm_loss.lib.__self__ is not ema.lib.__self__ and rm_loss.lib() is rm_loss.lib()
    with pytest.raises(rm_loss.HotpathError, match="operands given"):
        rm_loss.launch("dd_rm_loss_bwd", None, None, 0, 1, 4, None, 1.0)
    with pytest.raises(rm_loss.HotpathError, match="not a function of include/dd_rm_loss.h"):
        rm_loss.launch("dd_box_loss_bwd", None, None, 0, 1, 4, None, 1.0, None)


def test_the_kernels_use_no_scratch_and_no_spills():
    from driving_dirty_amd import build
    ks = kernel_resources().kernels(build.EXTENSIONS["rm_loss"].lib)
    assert len(ks) == 7, [k[".name"] for k in ks]      # statistics and gradient for the three forms of the target, one finalise
    for k in ks:
        assert k[".private_segment_fixed_size"] == 0, k[".name"]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k[".name"]
        if "stats" in k[".name"]:
            assert k[".vgpr_count"] <= 128, (k[".name"], k[".vgpr_count"])      # four waves per SIMD: the pass hides its loads behind other waves


def test_launchers_refuse_bad_arguments_without_a_gpu():
    from driving_dirty_amd import rm_loss
    lib = rm_loss.lib()
    M = 1 << 20      # never dereferenced: every call below is refused on the host
    Z, T, P, L, S, CF, WS, D = 1 * M, 2 * M, 3 * M, 4 * M, 5 * M, 6 * M, 7 * M, 8 * M
    nan, inf = float("nan"), float("inf")

    def refused(rc, *words):
        msg = rm_loss.last_error()
        assert rc != 0 and msg and all(w in msg for w in words), (rc, msg, words)

    def table(values):
        return (C.c_void_p * len(values))(*values)

    def fwd(z=Z, t=T, kind=1, batch=2, per=8, pw=1.0, a=1.0, b=0.0, eps=1.0, probs=P, loss=L, stats=S, coef=CF, ws=WS, ws_bytes=80):
        return lib.dd_rm_loss_fwd(z, t, kind, batch, per, pw, a, b, eps, probs, loss, stats, coef, ws, ws_bytes, None)

    def fwd_ptrs(z=Z, t=(T, T + 64), batch=2, per=8, pw=1.0, a=1.0, b=0.0, eps=1.0, probs=P, loss=L, stats=S, coef=CF, ws=WS, ws_bytes=80):
        return lib.dd_rm_loss_fwd_u8_ptrs(z, t and table(t), batch, per, pw, a, b, eps, probs, loss, stats, coef, ws, ws_bytes, None)

    def bwd(p=P, t=T, kind=1, batch=2, per=8, coef=CF, gs=1.0, dz=D):
        return lib.dd_rm_loss_bwd(p, t, kind, batch, per, coef, gs, dz, None)

    def bwd_ptrs(p=P, t=(T, T + 64), batch=2, per=8, coef=CF, gs=1.0, dz=D):
        return lib.dd_rm_loss_bwd_u8_ptrs(p, t and table(t), batch, per, coef, gs, dz, None)

    for fn, who in ((fwd, "rm_loss_fwd:"), (fwd_ptrs, "rm_loss_fwd_u8_ptrs:")):
        refused(fn(z=None), who, "logits", "NULL")
        refused(fn(z=Z + 4), who, "logits", "16-byte")
        refused(fn(probs=P + 8), who, "probs", "16-byte")
        for name, kw, align in (("loss_out", "loss", "4-byte"), ("stats", "stats", "8-byte"), ("coef", "coef", "16-byte"), ("workspace", "ws", "8-byte")):
            refused(fn(**{kw: None}), who, name, "NULL")
            refused(fn(**{kw: {"loss": L, "stats": S, "coef": CF, "ws": WS}[kw] + 2}), who, name, align)
        refused(fn(batch=0), who, "batch", "positive")
        refused(fn(per=0), who, "per_sample", "positive")
        refused(fn(per=6), who, "per_sample", "multiple of 4")
        refused(fn(batch=2, per=1 << 40), who, "2^40")
        for bad in (0.0, -2.0, nan, inf):
            refused(fn(pw=bad), who, "pos_weight")
        assert rm_loss.POS_WEIGHT_AUTO == -1.0
        for bad in (-0.5, nan, inf):
            refused(fn(eps=bad), who, "ts_eps")
            refused(fn(a=bad), who, "bce_weight")
            refused(fn(b=bad), who, "ts_weight")
        refused(fn(ws_bytes=79), who, "workspace_bytes", "80")
        refused(fn(per=rm_loss.CHUNK + 4, ws_bytes=159), who, "workspace_bytes", "160")
        refused(fn(probs=Z), who, "probs overlaps logits")
        refused(fn(probs=Z + 2 * 8 * 4 - 16), who, "probs overlaps logits")      # begins inside the last 16 bytes
    for fn, who in ((bwd, "rm_loss_bwd:"), (bwd_ptrs, "rm_loss_bwd_u8_ptrs:")):
        refused(fn(p=None), who, "probs", "NULL")
        refused(fn(dz=None), who, "dlogits", "NULL")
        refused(fn(p=P + 4), who, "probs", "16-byte")
        refused(fn(dz=D + 8), who, "dlogits", "16-byte")
        refused(fn(coef=None), who, "coef", "NULL")
        refused(fn(coef=CF + 4), who, "coef", "16-byte")
        refused(fn(per=10), who, "per_sample", "multiple of 4")
        refused(fn(batch=-1), who, "batch", "positive")
        refused(fn(gs=nan), who, "grad_scale", "NaN")
        refused(fn(dz=P), who, "dlogits overlaps probs")
        refused(fn(dz=P - 16), who, "dlogits overlaps probs")
    for fn, who in ((fwd, "rm_loss_fwd:"), (bwd, "rm_loss_bwd:")):
        refused(fn(t=None), who, "target", "NULL")
        refused(fn(kind=2), who, "unknown target kind 2")
        refused(fn(kind=1, t=T + 2), who, "target", "4-byte")
        refused(fn(kind=0, t=T + 4), who, "target", "16-byte")
    for fn, who in ((fwd_ptrs, "rm_loss_fwd_u8_ptrs:"), (bwd_ptrs, "rm_loss_bwd_u8_ptrs:")):
        refused(fn(t=None), who, "target_ptrs", "NULL")
        refused(fn(t=(T, None)), who, "target_ptrs[1]", "NULL")
        refused(fn(t=(T + 1, T + 64)), who, "target_ptrs[0]", "4-byte")
        refused(fn(batch=65, per=4, t=tuple(T + 4 * i for i in range(65)), **({"ws_bytes": 65 * 40} if fn is fwd_ptrs else {})), who, "65", "at most 64")


def test_python_refusals_name_the_operand():
    import torch
    from driving_dirty_amd import rm_loss
    with pytest.raises(rm_loss.HotpathError, match="logits must be fp32, got torch.float64"):
        rm_loss.road_map_loss(torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2, 8))
    with pytest.raises(rm_loss.HotpathError, match="logits must be fp32, got torch.bfloat16"):
        rm_loss.fwd(torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(2, 8))
    with pytest.raises(rm_loss.HotpathError, match=r"logits must be \[B, P\]"):
        rm_loss.fwd(torch.zeros(2, 2, 4), torch.zeros(2, 2, 4))
    with pytest.raises(rm_loss.HotpathError, match="pos_weight"):
        rm_loss.fwd(torch.zeros(2, 8), torch.zeros(2, 8), pos_weight="road")
    with pytest.raises(rm_loss.HotpathError, match="pos_weight"):
        rm_loss.fwd(torch.zeros(2, 8), torch.zeros(2, 8), pos_weight=-1.0)
    with pytest.raises(rm_loss.HotpathError, match="logits"):      # a host tensor never reaches a launcher
        rm_loss.fwd(torch.zeros(2, 8), torch.zeros(2, 8))


def test_the_parsers_take_the_four_flags_and_default_to_off():
    from driving_dirty_amd.roadmap import rm_loss_config
    for cls in road_map_models():
        args = cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([])
        assert {k: getattr(args, k) for k in FLAGS_OFF} == FLAGS_OFF, cls
        assert rm_loss_config(args) is None
        args = cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args(
            ["--rm_pos_weight", "auto", "--rm_bce_weight", "0.7", "--rm_ts_weight", "1.3", "--rm_ts_eps", "0"])
        assert rm_loss_config(args) == {"pos_weight": "auto", "bce_weight": 0.7, "ts_weight": 1.3, "ts_eps": 0.0}
        args = cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args(["--rm_pos_weight", "2.5"])
        assert rm_loss_config(args) == {"pos_weight": 2.5, "bce_weight": 1.0, "ts_weight": 0.0, "ts_eps": 1.0}
    assert rm_loss_config(Namespace()) is None and rm_loss_config(None) is None
    assert rm_loss_config(Namespace(rm_ts_weight=1)) == {"pos_weight": None, "bce_weight": 1.0, "ts_weight": 1.0, "ts_eps": 1.0}
    for bad in (dict(rm_pos_weight="road"), dict(rm_pos_weight=0), dict(rm_pos_weight=-1.0), dict(rm_pos_weight=float("inf")), dict(rm_pos_weight=True),
                dict(rm_ts_weight=-1), dict(rm_bce_weight=float("nan")), dict(rm_ts_eps=-0.1), dict(rm_ts_eps="x"),
                dict(rm_bce_weight=0.0), dict(rm_bce_weight=0, rm_ts_weight=0.0, rm_pos_weight="auto")):
        with pytest.raises(ValueError, match="rm_"):
            rm_loss_config(Namespace(**bad))


def test_the_models_hold_the_setting_and_road_map_refuses_it():
    RoadMapBCE, RoadMap, Joint = road_map_models()
    on = dict(rm_pos_weight="auto", rm_ts_weight=1.0)
    for cls in (RoadMapBCE, Joint):
        assert tiny(cls).rm_loss is None and tiny(cls, **FLAGS_OFF).rm_loss is None
        assert tiny(cls, **on).rm_loss == {"pos_weight": "auto", "bce_weight": 1.0, "ts_weight": 1.0, "ts_eps": 1.0}
        with pytest.raises(ValueError, match="both 0"):
            tiny(cls, rm_bce_weight=0.0)
    assert tiny(RoadMap).rm_loss is None and tiny(RoadMap, **FLAGS_OFF).rm_loss is None
    for flags in (on, dict(rm_pos_weight=2.0), dict(rm_bce_weight=0.5), dict(rm_ts_weight=0.25)):
        with pytest.raises(ValueError, match="RoadMapBCE"):
            tiny(RoadMap, **flags)
    with pytest.raises(ValueError, match="both 0"):
        tiny(RoadMap, rm_bce_weight=0.0)


def test_a_model_with_the_flags_off_never_imports_the_module(tmp_path):
    """Building the three modules, their parsers, a checkpoint and its reload with the flags off leaves ``driving_dirty_amd.rm_loss`` out
    of ``sys.modules``; with them on the module is imported by the first step, not by the constructor.  (That the step of a model with
    the flags off makes the parent's calls is tests/test_gpu_rm_loss_models.py.)"""
    import driving_dirty_amd
    name = "driving_dirty_amd.rm_loss"
    saved, had_attr = sys.modules.pop(name, None), hasattr(driving_dirty_amd, "rm_loss")
    attr = getattr(driving_dirty_amd, "rm_loss", None)
    try:
        for cls in road_map_models():
            cls.add_model_specific_args(ArgumentParser(add_help=False)).parse_args([])
            model = tiny(cls, **FLAGS_OFF)
            path = str(tmp_path / (cls.__name__ + ".ckpt"))
            model.save_checkpoint(path)
            assert cls.load_from_checkpoint(path).rm_loss is None
        on = tiny(road_map_models()[0], rm_ts_weight=1.0)
        assert on.rm_loss is not None
        assert name not in sys.modules
    finally:
        if saved is not None:
            sys.modules[name] = saved
        if had_attr:
            driving_dirty_amd.rm_loss = attr


def test_a_checkpoint_carries_the_setting(tmp_path):
    RoadMapBCE, _, Joint = road_map_models()
    flags = dict(rm_pos_weight="auto", rm_bce_weight=0.7, rm_ts_weight=1.3, rm_ts_eps=0.5)
    for cls in (RoadMapBCE, Joint):
        model = tiny(cls, **flags)
        path = str(tmp_path / (cls.__name__ + ".ckpt"))
        model.save_checkpoint(path)
        again = cls.load_from_checkpoint(path)
        assert again.rm_loss == model.rm_loss == {"pos_weight": "auto", "bce_weight": 0.7, "ts_weight": 1.3, "ts_eps": 0.5}
        assert {k: getattr(again.hparams, k) for k in flags} == flags
