"""Record every call that crosses the C ABI (include/dd_hotpath.h) during a few tiny training steps, as the fixture of
tests/test_gpu_abi_call_trace.py.

    python tools/record_abi_call_trace.py [--out tests/golden/abi_call_trace.json]

Every name of _lib.SIGNATURES is replaced on the CDLL object by a recorder (setattr, the mechanism of bench.py's AbiTimer) for the
duration of the steps.  A call is stored as [symbol, [per argument: "ptr", "null", a descriptor's field list, or the scalar]]: what
reaches the library and in which order, without the addresses.  Run this ONCE, on a GPU, at the commit whose calls a refactor of
the Python side of the boundary has to keep; the test replays STEPS on the code under test and requires the identical lists.

STEPS (the smallest models of the suite): RoadMapBCE in fp32 and the bf16 BasicAE on 16 x 22-pixel views at batch 3, two
TrainStep calls each (the first holds the lazy packing and workspace queries, the second is the steady step), and one TrainStep
call of BBSpatialRoadMap at the reference's view size, batch 2, frozen encoder, in exact fp32 and once more with split products."""
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


def bbox_spatial(dev, precision=None):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    ae = BasicAE(Namespace(hidden_dim=16, latent_dim=8))
    model = BBSpatialRoadMap(Namespace(pretrained_ae=ae, unfreeze_epoch_no=5, learning_rate=1e-3, output_img_freq=500, mse_loss=False))
    synth.fill_module(model, seed=17)
    model = model.to(dev)
    if precision is not None:
        model.box_merge.precision = precision             # the documented mode switch (hparams.precision sets the same attribute)
    views, road = synth.camera_batch(2, seed=17).to(dev), synth.road_maps(2, seed=17).to(dev)
    tgt = (synth.hash_uniform((2, 800, 800), synth.key_salt("bbt"), 0.0, 1.0) < 0.02).float().to(dev)
    np.random.seed(9)
    _train(model, [(tuple(views), tuple({"bb_map": tgt[i]} for i in range(2)), tuple(road))], lr=1e-3)


def bbox_split_products(dev):
    """The same step in precision mode "fp32x3": up_conv_1 / up_conv_2 on the split-product kernels (dd_dconv_split_*, dd_dconv_fwd_split,
    dd_dconv_wgrad_split)."""
    bbox_spatial(dev, precision="fp32x3")


STEPS = (roadmap_fp32, autoencoder_bf16, bbox_spatial, bbox_split_products)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "abi_call_trace.json"))
    ap.add_argument("--check", action="store_true", help="record twice and require the same lists before writing")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_abi_call_trace: needs a GPU")
    out = record()
    if args.check and record() != out:
        raise SystemExit("record_abi_call_trace: two recordings in one process differ")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in out.items()}, f"{os.path.getsize(args.out)} bytes -> {args.out}")


if __name__ == "__main__":
    main()
