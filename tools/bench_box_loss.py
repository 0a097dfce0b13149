"""Time the class-balanced box-map loss (csrc/box_loss.hip) beside dd_bce_probs on the same operands, and the box-head step with it.

    python tools/bench_box_loss.py [--batch 32] [--boxes 60] [--reps 20] [--step] [--out profiles/box_loss_timing.json]

probs [batch, 640000] uniform in [0.02, 0.98], targets rasterised from `boxes` cars per sample; pos_weight "auto", bce_weight = ts_weight = 1.
HIP events around single ABI calls on preallocated buffers (the kernels, not the allocator), a warm-up, then `reps` ROUNDS in which every
candidate runs once -- dd_bce_probs (loss + gradient), dd_box_loss_fwd, fwd + bwd, each of the two with an fp32 and a byte target -- so
that clock drift falls on all alike; medians.  Bytes per element: dd_bce_probs reads p and t and writes the gradient (12); the two-pass form
reads p and t twice and writes the gradient (20 with an fp32 target, 14 with a byte one).  Each pass's share of the HBM peak is printed.
``--step``: also the config-3 step (BBSpatialRoadMap, frozen encoder, HipAdam on the heads; tools/bench_models.py's) with the loss off and
on, alternating in one run."""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import ops, synth  # noqa: E402
from driving_dirty_amd._lib import call, size  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X: 8 TB/s


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
    b, per = args.batch, 640000
    n = b * per
    probs = synth.hash_uniform((b, per), 7, 0.02, 0.98).to(dev)
    t32 = ops.boxes_to_binary_map([synth.car_boxes(args.boxes, seed=100 + i) for i in range(b)], dev).reshape(b, per)
    t8 = t32.to(torch.uint8)
    grad = torch.empty_like(probs)
    loss, losses = torch.empty((), device=dev), torch.empty(3, device=dev)
    stats, coef = torch.empty((b, 5), device=dev, dtype=torch.float64), torch.empty((b, 4), device=dev)
    ws_bce = torch.empty(size("dd_loss_workspace_bytes", n), device=dev, dtype=torch.uint8)
    ws_box = torch.empty(size("dd_box_loss_workspace_bytes", b), device=dev, dtype=torch.uint8)

    def fwd(t, kind):
        call("dd_box_loss_fwd", probs, t, kind, b, per, ops.POS_WEIGHT_AUTO, 1.0, 1.0, 1.0, losses, stats, coef, ws_box)

    def both(t, kind):
        fwd(t, kind)
        call("dd_box_loss_bwd", probs, t, kind, b, per, coef, 1.0, grad)

    timing = time_rounds({
        "bce_probs": lambda: call("dd_bce_probs", probs, t32, loss, grad, n, 1.0, ws_bce),
        "box_loss_fwd_f32": lambda: fwd(t32, 0), "box_loss_fwd_bwd_f32": lambda: both(t32, 0),
        "box_loss_fwd_u8": lambda: fwd(t8, 1), "box_loss_fwd_bwd_u8": lambda: both(t8, 1)}, args.reps)
    bytes_per_element = {"bce_probs": 12, "box_loss_fwd_f32": 8, "box_loss_fwd_bwd_f32": 20, "box_loss_fwd_u8": 5, "box_loss_fwd_bwd_u8": 14}
    for k, v in timing.items():
        v["bytes"] = bytes_per_element[k] * n
        v["GB_per_s"] = v["bytes"] / v["median_ms"] / 1e6
        v["share_of_hbm_peak"] = v["GB_per_s"] / HBM_PEAK_GBS
    for kind in ("f32", "u8"):      # the gradient pass by difference: 12 / 9 bytes per element
        ms = timing[f"box_loss_fwd_bwd_{kind}"]["median_ms"] - timing[f"box_loss_fwd_{kind}"]["median_ms"]
        nbytes = (12 if kind == "f32" else 9) * n
        timing[f"box_loss_bwd_{kind}_by_difference"] = {"median_ms": ms, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6,
                                                        "share_of_hbm_peak": nbytes / ms / 1e6 / HBM_PEAK_GBS}
    base = timing["bce_probs"]["median_ms"]
    return {"batch": b, "per_sample": per, "boxes_per_sample": args.boxes, "positive_fraction": float(t32.mean()), "hbm_peak_GB_per_s": HBM_PEAK_GBS,
            "losses": losses.tolist(), "timing": timing,
            "fwd_bwd_f32_over_bce_probs": timing["box_loss_fwd_bwd_f32"]["median_ms"] / base,
            "fwd_bwd_u8_over_fwd_bwd_f32": timing["box_loss_fwd_bwd_u8"]["median_ms"] / timing["box_loss_fwd_bwd_f32"]["median_ms"]}


def bench_step(args, dev):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.optim import HipAdam
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    b = args.batch
    torch.manual_seed(20200505)
    views = torch.rand(b, 6, 3, 256, 306, device=dev)
    road = torch.rand(b, 800, 800, device=dev) < 0.3
    tgt = tuple({"bb_map": m} for m in ops.boxes_to_binary_map([synth.car_boxes(args.boxes, seed=100 + i) for i in range(b)], dev))
    batch = (tuple(views), tgt, tuple(road))
    steps = {}
    for name, extra in (("off", {}), ("on", {"box_pos_weight": "auto", "box_ts_weight": 1.0})):
        torch.manual_seed(20200505)
        m = BBSpatialRoadMap(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=128, latent_dim=64)), unfreeze_epoch_no=10 ** 9, learning_rate=1e-3,
                                       output_img_freq=500, mse_loss=False, **extra)).to(dev)
        opt = HipAdam([p for p in m.parameters() if p.requires_grad], lr=1e-3)

        def step(m=m, opt=opt):
            m.zero_grad(set_to_none=True)
            m.training_step(batch, 0)["loss"].backward()
            opt.step()
        steps[name] = step
    for _ in range(2):
        for step in steps.values():
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(args.step_reps):
        for name, step in steps.items():
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = {k: median_ms(v) for k, v in times.items()}
    out["on_minus_off_ms"] = out["on"]["median_ms"] - out["off"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--boxes", type=int, default=60)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="also time the box-head step (config 3) with the loss off and on")
    ap.add_argument("--step_reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_loss: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), **bench_kernels(args, dev)}
    if args.step:
        result["box_head_step_ms"] = bench_step(args, dev)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
