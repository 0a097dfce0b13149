"""Time the sampled road-map head (csrc/head_mean.hip) beside the unfused composition it replaces, and the predictions with and without it.

    python tools/bench_head_mean.py [--batch 32] [--samples 1,4,8,16] [--reps 15] [--predict_batch 8] [--predict_rounds 11] [--no-predict]
                                    [--out profiles/head_mean_bench.json]

Kernels, at the head's real shape (N = 640000, K = 64), B scenes of S latents: ``dd_head_mean_gt`` and ``dd_head_mean_prob`` against the
same result from the pieces the package had before -- ``ops.linear`` on the ``[B * S, 64]`` latents, ``ops.sigmoid``, the mean over a
scene's draws (and ``>``) -- on the same tensors in this process; at S = 1 also ``dd_linear_sigmoid_gt``, the same tiles.  HIP events
around single calls on preallocated inputs, a warm-up, then ``reps`` ROUNDS in which every candidate runs once, so that clock drift
falls on all alike; the median with the fastest and the slowest round beside it.  THE CONDITION, which the exit status reports: each
kernel is no slower than its composition beyond the spread of the rounds (tools/bench_tta.py's condition).  Bytes moved are computed
from the shapes: the 164 MB weight once per launch of at most 64 rows, the latents, the output once.

Predictions (unless ``--no-predict``), at the reference's sizes (hidden 128 / latent 64, seeded, dropout as in eval mode):
``RoadMapBCE.predict_road_map`` at S = 1, 8 and 16, the forms taking turns for ``--predict_rounds`` rounds; milliseconds per call and
the time S > 1 adds.  The conv stack and ``fc1`` run once either way.  No bound is set on it."""
import argparse
import json
import os
import sys
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import mc, ops, synth  # noqa: E402

N, K = 800 * 800, 64
TAU = 0.5


def summary(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


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
    return {k: summary(v) for k, v in times.items()}


def not_slower(kernel, composition):
    spread = max(kernel["max_ms"] - kernel["min_ms"], composition["max_ms"] - composition["min_ms"])
    return spread, bool(kernel["median_ms"] <= composition["median_ms"] + spread)


def bench_kernels(args, dev, samples):
    b = args.batch
    x = synth.hash_uniform((b * samples, K), 31, -1.0, 1.0).to(dev)
    w = synth.hash_uniform((N, K), 32, -0.375, 0.375).to(dev)
    bias = synth.hash_uniform((N,), 33, -0.5, 0.5).to(dev)
    inv = torch.tensor(1.0 / samples, dtype=torch.float32, device=dev)

    def unfused_prob():
        with torch.no_grad():
            p = ops.sigmoid(ops.linear(x, w, bias)).reshape(b, samples, N)
        if samples == 1:
            return p[:, 0]
        total = p[:, 0].clone()
        for s in range(1, samples):      # the pinned order; torch.sum over the draws (another order) is timed beside it
            total += p[:, s]
        return total * inv

    def unfused_prob_torch_sum():
        with torch.no_grad():
            return ops.sigmoid(ops.linear(x, w, bias)).reshape(b, samples, N).sum(1) * inv

    candidates = {"head_mean_gt": lambda: mc.mean_gt(x, w, bias, TAU, samples), "unfused_gt": lambda: unfused_prob() > TAU,
                  "head_mean_prob": lambda: mc.mean_prob(x, w, bias, samples), "unfused_prob": unfused_prob,
                  "unfused_prob_torch_sum": unfused_prob_torch_sum}
    if samples == 1:
        candidates["linear_sigmoid_gt"] = lambda: ops.linear_sigmoid_gt(x, w, bias, TAU)
    same = bool(torch.equal(candidates["head_mean_gt"](), candidates["unfused_gt"]())
                and torch.equal(candidates["head_mean_prob"]().view(torch.int32), candidates["unfused_prob"]().contiguous().view(torch.int32)))
    timing = time_rounds(candidates, args.reps)
    launches = -(-b // (64 // samples))
    moved = launches * N * K * 4 + b * samples * K * 4
    for name, out_bytes in (("head_mean_gt", b * N), ("head_mean_prob", 4 * b * N)):
        timing[name]["bytes"] = moved + out_bytes
        timing[name]["GB_per_s"] = (moved + out_bytes) / timing[name]["median_ms"] / 1e6
    out = {"scenes": b, "samples": samples, "rows": b * samples, "launches": launches, "same_bits_as_the_composition": same, "timing": timing}
    ok = same
    for kernel, comp in (("head_mean_gt", "unfused_gt"), ("head_mean_prob", "unfused_prob")):
        spread, fine = not_slower(timing[kernel], timing[comp])
        out[kernel + "_vs_composition"] = {"speedup_median": timing[comp]["median_ms"] / timing[kernel]["median_ms"], "spread_ms": spread,
                                           "kernel_not_slower": fine}
        ok = ok and fine
    if samples == 1:
        spread, fine = not_slower(timing["head_mean_gt"], timing["linear_sigmoid_gt"])
        out["head_mean_gt_vs_linear_sigmoid_gt"] = {"ratio_median": timing["head_mean_gt"]["median_ms"] / timing["linear_sigmoid_gt"]["median_ms"],
                                                    "spread_ms": spread, "equal_within_the_spread": fine}
    del x, w, bias
    torch.cuda.empty_cache()
    return out, ok


def bench_predictions(args, dev):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    b = args.predict_batch
    x = synth.camera_batch(b, seed=5).to(dev)
    torch.manual_seed(20200505)
    model = RoadMapBCE(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=128, latent_dim=64)), unfreeze_epoch_no=0, learning_rate=1e-3,
                                 output_img_freq=500)).to(dev).eval()
    timing = time_rounds({f"S{s}": (lambda s=s: model.predict_road_map(x, TAU, mc_samples=s, tta=False)) for s in (1, 8, 16)}, args.predict_rounds)
    out = {"batch": b, "hidden_dim": 128, "latent_dim": 64, "rounds": args.predict_rounds, **timing}
    for s in (8, 16):
        out[f"S{s}_added_ms_median"] = timing[f"S{s}"]["median_ms"] - timing["S1"]["median_ms"]
        out[f"S{s}_over_S1_median"] = timing[f"S{s}"]["median_ms"] / timing["S1"]["median_ms"]
    out["spread_ms"] = max(t["max_ms"] - t["min_ms"] for t in timing.values())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=str, default="1,4,8,16")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--predict_batch", type=int, default=8)
    ap.add_argument("--predict_rounds", type=int, default=11)
    ap.add_argument("--no-predict", action="store_true", help="kernels only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_mean: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "argv": sys.argv[1:], "n": N, "k": K, "tau": TAU, "kernels": {}}
    ok = True
    for s in (int(t) for t in args.samples.split(",")):
        result["kernels"][f"S{s}"], fine = bench_kernels(args, dev, s)
        ok = ok and fine
    if not args.no_predict:
        result["predictions"] = bench_predictions(args, dev)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not ok:
        raise SystemExit("bench_head_mean: a kernel is slower than the unfused composition beyond the spread of the rounds, or their bits differ")


if __name__ == "__main__":
    main()
