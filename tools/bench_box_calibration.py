"""What ``--calibrate_box_threshold`` adds to a validation step, measured.

    python tools/bench_box_calibration.py [--module joint|box] [--batch 16] [--rounds 15] [--warmup 3] [--out profiles/box_calibration_timing.json]

``validation_step`` of the module at the reference's sizes (hidden 128 / latent 64, closed-form weights and inputs, the box head's map
centred on 0.5 and widened so that every threshold of the grid cuts it somewhere) on one batch in the collate's per-sample form, between
two device events: with ``--box_metrics`` alone, and with ``--calibrate_box_threshold`` added.  The two take turns for ``--rounds``
rounds after ``--warmup`` calls of each, so both see the same machine; reported: the median with the fastest and the slowest round.
Then ``spatial.box_ats_sweep`` alone, on that same map (an UNTRAINED head's map is noise: thousands of components per sample at most
thresholds, the expensive end) and on the rasterised targets (clean blobs: what a trained head's map approaches), per threshold.

On a commit from before the flag existed the script times the ``--box_metrics`` step alone (the flag is then an hparam nobody reads):
the figure to hold this commit's against."""
import argparse
import json
import math
import os
import sys
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import ops, spatial, synth  # noqa: E402
from driving_dirty_amd.autoencoder import BasicAE  # noqa: E402

HAS_SWEEP = hasattr(spatial, "box_ats_sweep")
GAIN = 48.0      # tests/test_gpu_box_calibration.py: the filled head's centred map then spans 0.02 .. 0.998


def build(kind, args, dev):
    from driving_dirty_amd.joint import JointRoadMapBBox
    ae = BasicAE(Namespace(hidden_dim=args.hidden_dim, latent_dim=args.latent_dim))
    hp = Namespace(pretrained_ae=ae, learning_rate=1e-3, output_img_freq=500, unfreeze_epoch_no=5, box_metrics=True)
    model = (JointRoadMapBBox if kind == "joint" else spatial.BBSpatialRoadMap)(hp)
    synth.fill_module(model, seed=29)
    if kind == "joint":
        with torch.no_grad():
            model.fc1.weight.mul_(4.0)
            model.fc1.bias.mul_(4.0)
        model.ae.encoder.fc1.drop_p = model.ae.encoder.fc2.drop_p = 0.0
    return model.to(dev).eval()


def box_map(model, x, rm):
    with torch.no_grad():
        out = model(x, rm)
    return out[1] if isinstance(out, tuple) else out


def summary(ms):
    s = sorted(ms)
    return {"ms_median": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1]}


def timed_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def take_turns(paths, warmup, rounds):
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            ms[k].append(timed_ms(fn))
    return {k: summary(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--module", default="joint", choices=("joint", "box"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--boxes", type=int, default=30, help="target boxes per sample")
    ap.add_argument("--hidden_dim", type=int, default=128)
    ap.add_argument("--latent_dim", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_calibration: needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    model = build(args.module, args, dev)
    b = args.batch
    x, rm = tuple(synth.camera_batch(b, seed=17).to(dev)), tuple(synth.road_maps(b, seed=17).to(dev))
    targets = tuple({"bounding_box": synth.car_boxes(args.boxes, seed=100 + i)} for i in range(b))
    with torch.no_grad():      # widen, then centre (tests/_joint_cases.py: centre_box_map)
        model.box_merge.up_conv_5.weight.mul_(GAIN)
        m = float(box_map(model, x[:2], rm[:2]).median())
        model.box_merge.up_conv_5.bias -= math.log(m / (1.0 - m))
    batch = (x, targets, rm)

    def step(calibrate):
        def run():
            model.hparams.calibrate_box_threshold = calibrate
            with torch.no_grad():
                return model.validation_step(batch, 0)
        return run

    paths = {"box_metrics": step(False)}
    if HAS_SWEEP:
        paths["box_metrics_and_calibrate_box_threshold"] = step(True)
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "argv": sys.argv[1:], "module": args.module, "batch": b, "target_boxes_per_sample": args.boxes, "rounds": args.rounds,
              "warmup": args.warmup, "has_sweep": HAS_SWEEP}
    result["validation_step"] = take_turns(paths, args.warmup, args.rounds)
    if HAS_SWEEP:
        grid = spatial.box_threshold_grid(model.hparams)
        noise = box_map(model, x, rm).contiguous()
        clean = ops.boxes_to_binary_map([t["bounding_box"] for t in targets], dev).float()
        sweeps = take_turns({"untrained_map": lambda: spatial.box_ats_sweep(model.hparams, noise, targets, grid),
                             "rasterised_targets": lambda: spatial.box_ats_sweep(model.hparams, clean, targets, grid)}, args.warmup, args.rounds)
        for k, v in sweeps.items():
            v["ms_median_per_threshold"] = v["ms_median"] / len(grid)
        v = result["validation_step"]
        result.update(thresholds=len(grid), box_ats_sweep=sweeps,
                      added_ms_median=v["box_metrics_and_calibrate_box_threshold"]["ms_median"] - v["box_metrics"]["ms_median"],
                      components_per_sample_untrained_map={f"{t:.4f}": float(ops.component_boxes(noise, t, 1, 256)[1].float().mean()) for t in grid})
    for k, v in result["validation_step"].items():
        print(f"validation_step, {k}: {v['ms_median']:.3f} ms per batch of {b} (rounds {v['ms_min']:.3f} .. {v['ms_max']:.3f})")
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
