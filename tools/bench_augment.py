"""Time the train-time augmentation (csrc/augment.hip) beside the parent's like-for-like byte shuffle, and the config-2 step with it.

    python tools/bench_augment.py [--batch 32] [--reps 20] [--step_reps 7] [--step_rounds 3] [--window 5] [--no-step] [--out profiles/augment_timing.json]

Kernels, at the workload's B = 32 and 256 x 306: dd_aug_views_u8_ptrs, dd_aug_views_ptrs and dd_aug_masks_u8_ptrs with every second
sample mirrored, jitter on every view and one view dropped in every fourth sample, against dd_stitch6_u8_ptrs on the same frames
(3 bytes in, 16 out per pixel: the gather the step already runs).  HIP events around single ABI calls on preallocated buffers, a
warm-up, then `reps` ROUNDS in which every candidate runs once, so that clock drift falls on all alike; medians.  Bytes moved are
computed from the shapes (every input byte once, every output byte once; a dropped view is not read) and given with the achieved
GB/s and its share of the HBM peak.

Step: train.TrainStep on config 2 (RoadMapBCE, hidden 128 / latent 64, the collate's tuples of fp32 views and bool masks) with
aug_mirror = 0.5 plus jitter against the same step with the augmentation off: `step_rounds` rounds in one process, the two forms
taking turns (each builds its model, warms up, times `step_reps` windows of `window` steps and closes); a host clock around a window
that ends in a device synchronise, per step, medians over all rounds.  ``extra_pass_fraction_of_step`` is the difference over the
plain step.  (With a synchronise behind EVERY step the host side of ``apply`` -- the draw, the ctypes tables -- is not hidden behind
the previous step's kernels and is measured too: ``--window 1``.)"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import augment, synth  # noqa: E402
from driving_dirty_amd._lib import call  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X: 8 TB/s
H, W = 256, 306


def median_ms(times):
    times = sorted(times)
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": len(times)}


def time_rounds(candidates, reps, warmup=3):
    """{name: fn} -> {name: timing}; every round runs each candidate once, in turn."""
    for _ in range(warmup):
        for fn in candidates.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in candidates}
    for _ in range(reps):
        for name, fn in candidates.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {k: median_ms(v) for k, v in times.items()}


def bench_kernels(args, dev):
    b = args.batch
    frames = (synth.hash_uniform((b, 6, H, W, 3), 11, 0.0, 1.0) * 255).round().to(torch.uint8).to(dev)
    views = frames.permute(0, 1, 4, 2, 3).float().div(255).contiguous()
    road = (synth.hash_uniform((b, 800, 800), 12, 0.0, 1.0) < 0.3).to(dev)
    flags = [(i % 2) | ((1 << (8 + i % 6)) if i % 4 == 0 else 0) for i in range(b)]
    color = torch.tensor([[1.0 + 0.01 * ((i + v) % 7 - 3), 0.005 * (i % 5 - 2)] for i in range(b) for v in range(6)]).reshape(b, 6, 2)
    cflags, ccolor = augment._host_arrays(flags, color, b)
    tab_u8, tab_f32 = (C.c_void_p * b)(*[t.data_ptr() for t in frames]), (C.c_void_p * b)(*[t.data_ptr() for t in views])
    tab_m = (C.c_void_p * b)(*[t.data_ptr() for t in road])
    out = torch.empty((b, 6, 3, H, W), device=dev)
    wide4 = torch.empty((b, H, 6 * W, 4), device=dev)
    out_m = torch.empty((b, 800, 800), device=dev, dtype=torch.uint8)
    timing = time_rounds({
        "stitch6_u8_ptrs": lambda: call("dd_stitch6_u8_ptrs", tab_u8, wide4, None, b, H, W, -1),
        "aug_views_u8_ptrs": lambda: augment.launch("dd_aug_views_u8_ptrs", tab_u8, cflags, ccolor, out, b, H, W),
        "aug_views_ptrs": lambda: augment.launch("dd_aug_views_ptrs", tab_f32, cflags, ccolor, out, b, H, W),
        "aug_masks_u8_ptrs": lambda: augment.launch("dd_aug_masks_u8_ptrs", tab_m, cflags, out_m, b, 800, 800)}, args.reps)
    kept = sum(6 - bin(f >> 8).count("1") for f in flags)      # views that are read
    px = H * W
    nbytes = {"stitch6_u8_ptrs": b * 6 * px * (3 + 16), "aug_views_u8_ptrs": kept * px * 3 + b * 6 * px * 12,
              "aug_views_ptrs": kept * px * 12 + b * 6 * px * 12, "aug_masks_u8_ptrs": 2 * b * 800 * 800}
    for k, v in timing.items():
        v["bytes"] = nbytes[k]
        v["GB_per_s"] = v["bytes"] / v["median_ms"] / 1e6
        v["share_of_hbm_peak"] = v["GB_per_s"] / HBM_PEAK_GBS
    return {"batch": b, "height": H, "width": W, "mirrored": sum(f & 1 for f in flags), "views_dropped": b * 6 - kept,
            "hbm_peak_GB_per_s": HBM_PEAK_GBS, "timing": timing,
            "aug_views_u8_over_stitch6_u8": timing["aug_views_u8_ptrs"]["median_ms"] / timing["stitch6_u8_ptrs"]["median_ms"]}


def bench_step(args, dev):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    from driving_dirty_amd.train import TrainStep
    b = args.batch
    torch.manual_seed(20200505)
    views = torch.rand(b, 6, 3, H, W, device=dev)
    road = torch.rand(b, 800, 800, device=dev) < 0.3
    batch = (tuple(views), tuple({} for _ in range(b)), tuple(road))
    forms = {"off": {}, "on": dict(aug_mirror=0.5, aug_brightness=0.2, aug_contrast=0.2, aug_per_view=0.1, aug_seed=1)}
    times, rounds = {k: [] for k in forms}, []
    for r in range(args.step_rounds):      # one TrainStep alive at a time (tools/bench_clip.py's arrangement), the two forms taking turns
        for name, extra in forms.items():
            torch.manual_seed(20200505)
            model = RoadMapBCE(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=128, latent_dim=64)), unfreeze_epoch_no=0,
                                         learning_rate=1e-3, output_img_freq=500, batch_size=b, **extra)).to(dev)
            ts = TrainStep(model)
            for _ in range(3):
                ts(batch, 0)
            torch.cuda.synchronize()
            mine = []
            for _ in range(args.step_reps):      # a window of steps between two synchronises, as bench.py times them: the host runs ahead
                t0 = time.perf_counter()
                for _ in range(args.window):
                    ts(batch, 0)
                torch.cuda.synchronize()
                mine.append((time.perf_counter() - t0) * 1e3 / args.window)
            ts.close()
            del ts, model
            torch.cuda.empty_cache()
            times[name] += mine
            rounds.append({"round": r, "form": name, **median_ms(mine)})
    out = {k: median_ms(v) for k, v in times.items()}
    out["rounds"] = rounds
    out["on_minus_off_ms"] = out["on"]["median_ms"] - out["off"]["median_ms"]
    out["extra_pass_fraction_of_step"] = out["on_minus_off_ms"] / out["off"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step_reps", type=int, default=7)
    ap.add_argument("--step_rounds", type=int, default=3)
    ap.add_argument("--window", type=int, default=5, help="steps per timed window (one synchronise behind each window)")
    ap.add_argument("--no-step", action="store_true", help="kernels only: skip the config-2 step with the augmentation off and on")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), **bench_kernels(args, dev)}
    if not args.no_step:
        result["config2_step_ms"] = bench_step(args, dev)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
