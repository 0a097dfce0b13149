"""Time the box-level validation ops on the GPU against the CPU reference of tests/_box_eval_ref.py, on the same inputs.

    python tools/bench_box_eval.py [--batch 32] [--boxes 60] [--reps 20] [--out profiles/box_eval_timing.json]
    python tools/bench_box_eval.py --fit oriented --out profiles/box_fit_timing.json
    python tools/bench_box_eval.py --split_px 4 [--grow_iters 8] --out profiles/box_split_timing.json

``component_boxes`` on [batch,800,800] rasterised targets and ``ats_bounding_boxes`` on `batch` samples of about boxes x boxes pairs:
HIP events around `reps` calls after a warm-up (allocation of the workspace included: it is what a validation step pays).  The CPU
side is what a user without these ops would run: scipy labelling + the Python IoU loop, once, on the cores this process may use.
``--fit oriented`` instead times ``component_boxes(fit="oriented")`` beside the extent fit, on the same maps in the same run (no CPU
side: the question there is what the second pass over the labels and the 64-bit atomics cost).  ``--split_px N`` times the split decode
(``component_boxes(fit="oriented", split_px=N)``: erode, label, grow, label, merge, then the fit of the label image) beside the unsplit
oriented fit on the same maps in the same run, and scores both against the boxes the maps were painted from."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _box_eval_ref as ref  # noqa: E402
from driving_dirty_amd import ops, synth  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def report(result, out):
    print(json.dumps(result))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def bench_fit(args):
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_eval: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    targets = [synth.car_boxes(args.boxes, seed=100 + i) for i in range(args.batch)]
    maps = ops.boxes_to_binary_map(targets, dev)
    extent = timed(lambda: ops.component_boxes(maps, 0.5, 1, 256), args.reps)
    oriented = timed(lambda: ops.component_boxes(maps, 0.5, 1, 256, fit="oriented"), args.reps)
    moments = timed(lambda: ops.component_boxes(maps, 0.5, 1, 256, fit="oriented", want_moments=True), args.reps)
    extent_again = timed(lambda: ops.component_boxes(maps, 0.5, 1, 256), args.reps)      # brackets the oriented runs: drift shows here
    _, counts = ops.component_boxes(maps, 0.5, 1, 256)
    boxes, counts2 = ops.component_boxes(maps, 0.5, 1, 256, fit="oriented")
    assert torch.equal(counts, counts2)
    counts = counts.tolist()
    ats = {}
    for name, bx in (("extent", ops.component_boxes(maps, 0.5, 1, 256)[0]), ("oriented", boxes),
                     ("oriented_pad0", ops.component_boxes(maps, 0.5, 1, 256, fit="oriented", pad_px=0.0)[0])):
        ats[name] = float(ops.ats_bounding_boxes([bx[i, :min(c, 256)] for i, c in enumerate(counts)], targets).mean())
    report({"device": torch.cuda.get_device_name(0), "batch": args.batch, "boxes_per_sample": args.boxes,
            "components_per_sample_mean": float(np.mean(counts)),
            "gpu_component_boxes_extent_ms": extent, "gpu_component_boxes_oriented_ms": oriented,
            "gpu_component_boxes_oriented_with_moments_ms": moments, "gpu_component_boxes_extent_again_ms": extent_again,
            "oriented_over_extent": oriented["median_ms"] / extent["median_ms"], "ats_mean_of_the_rasterised_targets": ats}, args.out)


def bench_split(args):
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_eval: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    r, g = args.split_px, 2 * args.split_px if args.grow_iters is None else args.grow_iters
    targets = [synth.car_boxes(args.boxes, seed=100 + i) for i in range(args.batch)]
    maps = ops.boxes_to_binary_map(targets, dev)
    unsplit = timed(lambda: ops.component_boxes(maps, 0.5, 1, 256, fit="oriented"), args.reps)
    split = timed(lambda: ops.component_boxes(maps, 0.5, 1, 256, fit="oriented", split_px=r, grow_iters=g), args.reps)
    labels_only = timed(lambda: ops.split_components(maps, 0.5, r, g), args.reps)
    labels = ops.split_components(maps, 0.5, r, g)
    fit_only = timed(lambda: ops.labelled_boxes(labels, 1, 256, fit="oriented"), args.reps)
    plain_labels = timed(lambda: ops.label_components(maps, 0.5), args.reps)
    unsplit_again = timed(lambda: ops.component_boxes(maps, 0.5, 1, 256, fit="oriented"), args.reps)      # brackets the run: drift shows here
    ats, counts = {}, {}
    for pad_name, pad_px in (("", 0.5), ("_pad0", 0.0)):
        for name, kw in (("unsplit", {}), ("split", {"split_px": r, "grow_iters": g})):
            bx, n = ops.component_boxes(maps, 0.5, 1, 256, fit="oriented", pad_px=pad_px, **kw)
            n = n.tolist()
            counts[name] = float(np.mean(n))
            ats[name + pad_name] = float(ops.ats_bounding_boxes([bx[i, :min(c, 256)] for i, c in enumerate(n)], targets).mean())
    report({"device": torch.cuda.get_device_name(0), "batch": args.batch, "boxes_per_sample": args.boxes, "split_px": r, "grow_iters": g,
            "components_per_sample_mean": counts["unsplit"], "regions_per_sample_mean": counts["split"],
            "gpu_component_boxes_oriented_ms": unsplit, "gpu_component_boxes_oriented_split_ms": split,
            "gpu_split_components_ms": labels_only, "gpu_labelled_boxes_oriented_ms": fit_only, "gpu_label_components_ms": plain_labels,
            "gpu_component_boxes_oriented_again_ms": unsplit_again, "split_over_unsplit": split["median_ms"] / unsplit["median_ms"],
            "ats_mean_of_the_rasterised_targets": ats}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--boxes", type=int, default=60)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--fit", default="extent", choices=("extent", "oriented"), help="oriented: time the oriented fit beside the extent fit")
    ap.add_argument("--split_px", type=int, default=0, help="> 0: time the split decode beside the unsplit oriented fit")
    ap.add_argument("--grow_iters", type=int, default=None, help="with --split_px: rounds of growth (default 2 * split_px)")
    args = ap.parse_args()
    if args.split_px > 0:
        return bench_split(args)
    if args.fit == "oriented":
        return bench_fit(args)
    # the CPU workers are forked BEFORE this process touches the GPU, so none of them holds the device open
    import multiprocessing
    workers = min(16, len(os.sched_getaffinity(0)))
    pool = multiprocessing.get_context("fork").Pool(workers)
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_eval: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    targets = [synth.car_boxes(args.boxes, seed=100 + i) for i in range(args.batch)]
    maps = ops.boxes_to_binary_map(targets, dev)

    gpu_boxes = timed(lambda: ops.component_boxes(maps, 0.5, 1, 256), args.reps)
    boxes, counts = ops.component_boxes(maps, 0.5, 1, 256)
    counts = counts.tolist()
    preds = [boxes[i, :min(c, 256)] for i, c in enumerate(counts)]
    gpu_ats = timed(lambda: ops.ats_bounding_boxes(preds, targets), args.reps)
    gpu_labels = timed(lambda: ops.label_components(maps, 0.5), args.reps)
    got = ops.ats_bounding_boxes(preds, targets).cpu().numpy()

    masks = (maps > 0.5).cpu().numpy()
    preds_np, targets_np = [p.cpu().numpy() for p in preds], [t.numpy() for t in targets]
    with pool:
        t0 = time.perf_counter()
        cpu_boxes = pool.map(ref.component_boxes, masks)
        t1 = time.perf_counter()
        cpu_ats = pool.starmap(ref.ats, zip(preds_np, targets_np))
        t2 = time.perf_counter()
    assert [n for _, n in cpu_boxes] == counts
    assert float(np.abs(np.array(cpu_ats) - got).max()) <= 1e-6
    result = {
        "device": torch.cuda.get_device_name(0), "batch": args.batch, "boxes_per_sample": args.boxes,
        "components_per_sample_mean": float(np.mean(counts)),
        "gpu_label_components_ms": gpu_labels, "gpu_component_boxes_ms": gpu_boxes, "gpu_ats_bounding_boxes_ms": gpu_ats,
        "cpu_workers": workers, "cpu_component_boxes_ms": (t1 - t0) * 1e3, "cpu_ats_bounding_boxes_ms": (t2 - t1) * 1e3,
        "ats_mean": float(got.mean()),
    }
    report(result, args.out)


if __name__ == "__main__":
    main()
