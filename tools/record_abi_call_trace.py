"""Record every call that crosses the C ABI (include/dd_hotpath.h) during a few tiny training steps, as the fixture of
tests/test_gpu_abi_call_trace.py.

    python tools/record_abi_call_trace.py [--out tests/golden/abi_call_trace.json]

Every name of _lib.SIGNATURES is replaced on the CDLL object by a recorder (setattr, the mechanism of bench.py's AbiTimer) for the
duration of the steps.  A call is stored as [symbol, [per argument: "ptr", "null", a descriptor's field list, or the scalar]]: what
reaches the library and in which order, without the addresses.  Run this ONCE, on a GPU, at the commit whose calls a refactor of
the Python side of the boundary has to keep; the test replays STEPS on the code under test and requires the identical lists.

STEPS (the smallest models of the suite): RoadMapBCE in fp32 and the bf16 BasicAE on 16 x 22-pixel views at batch 3, two
TrainStep calls each (the first holds the lazy packing and workspace queries, the second is the steady step), and one TrainStep
call of BBSpatialRoadMap at the reference's view size, batch 2, frozen encoder, in exact fp32 and once more with split products.
Then the paths those leave out: the fp32 BasicAE at the same tiny size (the decoder's narrow path: dc3 by four phase launches, dc4 on
the generic engine), BoxesMergingCNN alone at batch 1 (the k8 d8 / k6 d6 output_padding layers, forward and backward), and the
BBSpatialRoadMap step at batch 1 with every A/B switch of gconv and heads off (each layer's fallback on the generic engine).

    python tools/record_abi_call_trace.py --schedule [--out tests/golden/backward_schedule_trace.json]

records the fixture of tests/test_gpu_backward_schedule.py instead: names only, of the optimizer passes and the conv stack's kernels
in one steady TrainStep call, for each of ARRANGEMENTS of the optimizer beside the backward (``record_schedule``)."""
import argparse
import ctypes
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import _lib, synth  # noqa: E402

_SCALARS = (ctypes.c_int32, ctypes.c_int64, ctypes.c_float)


def describe(arg, argtype):
    obj = getattr(arg, "_obj", None)                      # ctypes.byref(struct)
    if isinstance(obj, (_lib.ConvDesc, _lib.GConvDesc)):
        return [getattr(obj, n) for n, _ in obj._fields_]
    if argtype in _SCALARS:
        return int(arg) if isinstance(arg, bool) else arg
    if arg is None:
        return "null"
    if isinstance(arg, ctypes.c_void_p):
        arg = arg.value
    return "ptr" if not isinstance(arg, int) or arg else "null"


class Recorder:
    """``with Recorder() as calls:`` -- `calls` fills with [symbol, arguments] in call order; the entry points are restored on exit."""

    def __enter__(self):
        lib, self.calls, self._saved = _lib.lib(), [], {}
        for symbol, (_, argtypes) in _lib.SIGNATURES.items():
            inner = getattr(lib, symbol)
            self._saved[symbol] = inner

            def recorded(*a, _inner=inner, _symbol=symbol, _types=argtypes):
                self.calls.append([_symbol, [describe(x, t) for x, t in zip(a, _types)]])
                return _inner(*a)
            setattr(lib, symbol, recorded)
        return self.calls

    def __exit__(self, *exc):
        for symbol, inner in self._saved.items():
            setattr(_lib.lib(), symbol, inner)


def _train(model, batches, **kw):
    from driving_dirty_amd.train import TrainStep
    ts = TrainStep(model, scheduler=False, **kw)
    try:
        for i, batch in enumerate(batches):
            ts(batch, i)
        torch.cuda.synchronize()
    finally:
        ts.close()


def roadmap_fp32(dev):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8, input_height=16, input_width=132))
    model = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-2, output_img_freq=500))
    synth.fill_module(model, seed=77)
    model = model.to(dev)
    np.random.seed(5)                                     # the dropout masks
    batches = [(tuple(synth.camera_batch(3, 16, 22, seed=100 + 10 * s).to(dev)), None, tuple(synth.road_maps(3, seed=100 + 10 * s).to(dev)))
               for s in range(2)]
    _train(model, batches, lr=1e-2, big_numel=4096)


def autoencoder_bf16(dev):
    from driving_dirty_amd.autoencoder import BasicAE
    ae = BasicAE(Namespace(precision="bf16", learning_rate=1e-3, output_img_freq=10 ** 9, hidden_dim=16, latent_dim=8, input_height=16,
                           input_width=132, output_height=16, output_width=22))
    synth.fill_module(ae, seed=31)
    ae = ae.to(dev)
    np.random.seed(7)                                     # the masked view of six_to_one_task, the dropout masks
    _train(ae, [synth.camera_batch(3, 16, 22, seed=31 + s).to(dev) for s in range(2)], lr=1e-3, big_numel=4096)


def bbox_spatial(dev, precision=None, batch=2):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8))
    model = BBSpatialRoadMap(Namespace(pretrained_ae=ae, unfreeze_epoch_no=5, learning_rate=1e-3, output_img_freq=500, mse_loss=False))
    synth.fill_module(model, seed=17)
    model = model.to(dev)
    if precision is not None:
        model.box_merge.precision = precision             # the documented mode switch (hparams.precision sets the same attribute)
    views, road = synth.camera_batch(batch, seed=17).to(dev), synth.road_maps(batch, seed=17).to(dev)
    tgt = (synth.hash_uniform((batch, 800, 800), synth.key_salt("bbt"), 0.0, 1.0) < 0.02).float().to(dev)
    np.random.seed(9)
    _train(model, [(tuple(views), tuple({"bb_map": tgt[i]} for i in range(batch)), tuple(road))], lr=1e-3)


def bbox_split_products(dev):
    """The same step in precision mode "fp32x3": up_conv_1 / up_conv_2 on the split-product kernels (dd_dconv_split_*, dd_dconv_fwd_split,
    dd_dconv_wgrad_split)."""
    bbox_spatial(dev, precision="fp32x3")


def autoencoder_fp32(dev):
    """The fp32 BasicAE at autoencoder_bf16's sizes: the decoder's narrow path (dc3 by four phase launches, dc4 on the generic engine)."""
    from driving_dirty_amd.autoencoder import BasicAE
    ae = BasicAE(Namespace(learning_rate=1e-3, output_img_freq=10 ** 9, hidden_dim=16, latent_dim=8, input_height=16, input_width=132,
                           output_height=16, output_width=22))
    synth.fill_module(ae, seed=31)
    ae = ae.to(dev)
    np.random.seed(7)
    _train(ae, [synth.camera_batch(3, 16, 22, seed=31 + s).to(dev) for s in range(2)], lr=1e-3, big_numel=4096)


def box_merge_plain(dev):
    """BoxesMergingCNN alone, forward + backward, batch 1: the k8 d8 / k6 d6 output_padding up-convs."""
    from driving_dirty_amd.spatial import BoxesMergingCNN
    bm = synth.fill_module(BoxesMergingCNN(), seed=7).to(dev)
    ssr = synth.hash_uniform((1, 32, 128, 918), synth.key_salt("ssr"), 0.0, 1.0).to(dev).requires_grad_(True)
    space = synth.hash_uniform((1, 32, 256, 256), synth.key_salt("space"), 0.0, 1.0).to(dev).requires_grad_(True)
    pred = bm(ssr, space)
    (pred * synth.hash_uniform(tuple(pred.shape), synth.key_salt("sp_wy")).to(dev)).sum().backward()
    torch.cuda.synchronize()


def bbox_generic_engine(dev):
    """The bbox_spatial step at batch 1 with every A/B switch off: phased data gradients, the four-phase k2 s2 weight gradient, the
    64-channel chunk loop (cin = 96), the role-swapped and flipped weight gradients, the six strip convs one by one."""
    from driving_dirty_amd import gconv, heads
    switches = [(gconv, n) for n in ("DCONV", "K2S2_WGRAD", "SSCONV_FWD", "SSCONV_DGRAD", "STRIP6")] + \
               [(heads, n) for n in ("WINO_OUT", "WINO_DC2", "WINO_RM2")]
    saved = [getattr(m, n) for m, n in switches]
    try:
        for m, n in switches:
            setattr(m, n, False)
        bbox_spatial(dev, batch=1)
    finally:
        for (m, n), v in zip(switches, saved):
            setattr(m, n, v)


STEPS = (roadmap_fp32, autoencoder_bf16, bbox_spatial, bbox_split_products, autoencoder_fp32, box_merge_plain, bbox_generic_engine)


def record(dev=None):
    """{step name: [[symbol, arguments], ...]} of STEPS, in order."""
    dev = dev or torch.device("cuda:0")
    out = {}
    for step in STEPS:
        torch.manual_seed(0)
        with Recorder() as calls:
            step(dev)
        out[step.__name__] = calls
    return json.loads(json.dumps(out))                    # what the fixture holds: tuples as lists


# ---- the order of optimizer passes and conv kernels in one step -------------------------------------------------------------------
SCHEDULE_SYMBOLS = ("dd_adam_", "dd_conv_")               # the Adam passes; the entry points of c1 / c2 / c3, both Winograd families included
ARRANGEMENTS = {"default": {}, "passes_first": dict(passes_last=False), "after_backward": dict(adam_overlap=False),
                "materialised": dict(fuse_linear_wgrad=False)}


def schedule_of(ts, batch, batch_idx):
    """The SCHEDULE_SYMBOLS calls of ``ts(batch, batch_idx)``, names only, in call order."""
    with Recorder() as calls:
        ts(batch, batch_idx)
        torch.cuda.synchronize()
    return [symbol for symbol, _ in calls if symbol.startswith(SCHEDULE_SYMBOLS)]


def _tiny():
    """``_tiny_model`` / ``_tiny_batch`` of tests/test_gpu_round5.py: the suite's tiny RoadMapBCE and its batches."""
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_round5
    return test_gpu_round5._tiny_model, test_gpu_round5._tiny_batch


def tiny_train_step(dev, **kw):
    """TrainStep over the tiny model with the head and the encoder's fc1 on rank-B passes (big_numel = 4096): the smallest
    arrangement in which ``passes_last`` engages."""
    from driving_dirty_amd.train import TrainStep
    return TrainStep(_tiny()[0](dev), lr=1e-2, big_numel=4096, scheduler=False, **kw)


def record_schedule(dev=None):
    """{arrangement: [symbol, ...]} of the steady (second) TrainStep call in each of ARRANGEMENTS."""
    dev = dev or torch.device("cuda:0")
    batch = _tiny()[1]
    out = {}
    for name, kw in ARRANGEMENTS.items():
        ts = tiny_train_step(dev, **kw)
        try:
            ts(batch(dev, 0, 0), 0)
            out[name] = schedule_of(ts, batch(dev, 1, 0), 1)
        finally:
            ts.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schedule", action="store_true", help="record backward_schedule_trace.json (record_schedule) instead")
    ap.add_argument("--out", default=None, help="default: abi_call_trace.json, or backward_schedule_trace.json, under tests/golden")
    ap.add_argument("--check", action="store_true", help="record twice and require the same lists before writing")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_abi_call_trace: needs a GPU")
    rec = record_schedule if args.schedule else record
    args.out = args.out or os.path.join(ROOT, "tests", "golden", "backward_schedule_trace.json" if args.schedule else "abi_call_trace.json")
    out = rec()
    if args.check and rec() != out:
        raise SystemExit("record_abi_call_trace: two recordings in one process differ")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in out.items()}, f"{os.path.getsize(args.out)} bytes -> {args.out}")


if __name__ == "__main__":
    main()
