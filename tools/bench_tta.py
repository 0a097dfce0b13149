"""Time mirror test-time averaging (csrc/tta.hip) beside the unfused composition it replaces, and the predictions with and without it.

    python tools/bench_tta.py [--batch 32] [--reps 25] [--predict_batch 8] [--predict_rounds 15] [--no-predict] [--out profiles/tta_timing.json]

Kernels, at B = 32 and 800 x 800, logits in: ``dd_tta_mean_gt`` and ``dd_tta_mean_prob`` against the same result from the pieces the
package had before -- ``ops.sigmoid`` twice, ``flip``, add, halve (and compare) -- on the same tensors in this process.  HIP events
around single calls on preallocated inputs, a warm-up, then ``reps`` ROUNDS in which every candidate runs once, so that clock drift
falls on all alike; the median with the fastest and the slowest round beside it.  THE CONDITION, which the exit status reports: each
kernel is no slower than its composition beyond the spread of the rounds (tools/predict_joint.py's condition).  Bytes moved are
computed from the shapes (every input element once, every output element once) and given with the resulting rate.  These working
sets (184 MB and 246 MB) lie below the 256 MiB Infinity Cache and the inputs are re-read round after round: the rate compares the
kernels with each other and is NOT an HBM figure.  ``byte_form_columns`` times the byte form's two vector kernels through the
public entry point: 800 columns (16 per lane, one 16-byte store) against 804 (4 per lane, a 4-byte store), per output element.

Predictions (unless ``--no-predict``), at B = 8 and the reference's sizes (hidden 128 / latent 64, seeded, dropout as in eval mode):
``RoadMapBCE.predict_road_map`` and ``JointRoadMapBBox.predict`` with the averaging off and on, the forms taking turns for
``--predict_rounds`` rounds; milliseconds per call and the ratio on / off, which is expected near 2 (two forward passes plus the
mirror and mean kernels).  No bound is set on it."""
import argparse
import json
import os
import sys
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import ops, synth, tta  # noqa: E402

H = W = 800
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


def bench_kernels(args, dev):
    b = args.batch
    a = synth.hash_uniform((b, H, W), 21, -12.0, 12.0).to(dev)
    m = synth.hash_uniform((b, H, W), 22, -12.0, 12.0).to(dev)

    def unfused_prob():
        return (ops.sigmoid(a) + ops.sigmoid(m).flip(1)) * 0.5

    candidates = {"tta_mean_gt": lambda: tta.mean_gt(a, m, TAU, True), "unfused_gt": lambda: unfused_prob() > TAU,
                  "tta_mean_prob": lambda: tta.mean_prob(a, m, True), "unfused_prob": unfused_prob}
    same = bool(torch.equal(candidates["tta_mean_gt"](), candidates["unfused_gt"]())
                and torch.equal(candidates["tta_mean_prob"]().view(torch.int32), candidates["unfused_prob"]().view(torch.int32)))
    timing = time_rounds(candidates, args.reps)
    n = b * H * W
    nbytes = {"tta_mean_gt": 2 * 4 * n + n, "tta_mean_prob": 2 * 4 * n + 4 * n}
    for k, v in nbytes.items():
        timing[k]["bytes"] = v
        timing[k]["GB_per_s"] = v / timing[k]["median_ms"] / 1e6
    out = {"batch": b, "height": H, "width": W, "from_logits": True, "tau": TAU, "same_bits_as_the_composition": same, "timing": timing,
           "rate_note": "working sets below the 256 MiB Infinity Cache, inputs re-read every round: compares kernels, not an HBM figure"}
    ok = same
    for kernel, comp in (("tta_mean_gt", "unfused_gt"), ("tta_mean_prob", "unfused_prob")):
        spread, fine = not_slower(timing[kernel], timing[comp])
        out[kernel + "_vs_composition"] = {"speedup_median": timing[comp]["median_ms"] / timing[kernel]["median_ms"], "spread_ms": spread,
                                           "kernel_not_slower": fine}
        ok = ok and fine
    # the byte form's two vector kernels, through the public entry point: the shape alone picks
    wide = {w: (synth.hash_uniform((b, H, w), 23, -12.0, 12.0).to(dev), synth.hash_uniform((b, H, w), 24, -12.0, 12.0).to(dev)) for w in (800, 804)}
    cols = time_rounds({f"w{w}": (lambda p=p: tta.mean_gt(p[0], p[1], TAU, True)) for w, p in wide.items()}, args.reps)
    out["byte_form_columns"] = {"16_per_lane_w800": cols["w800"], "4_per_lane_w804": cols["w804"],
                                "ns_per_1e6_elements_16": 1e6 * cols["w800"]["median_ms"] / (b * H * 800) * 1e6,
                                "ns_per_1e6_elements_4": 1e6 * cols["w804"]["median_ms"] / (b * H * 804) * 1e6}
    return out, ok


def bench_predictions(args, dev):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.roadmap import RoadMapBCE
    b = args.predict_batch
    x = synth.camera_batch(b, seed=5).to(dev)
    out = {"batch": b, "hidden_dim": 128, "latent_dim": 64, "rounds": args.predict_rounds}
    for name, cls, call in (("predict_road_map", RoadMapBCE, lambda model, mode: model.predict_road_map(x, TAU, tta=mode)),
                            ("joint_predict", JointRoadMapBBox, lambda model, mode: model.predict_mode(x, mode, TAU, 0.5))):
        torch.manual_seed(20200505)
        model = cls(Namespace(pretrained_ae=BasicAE(Namespace(hidden_dim=128, latent_dim=64)), unfreeze_epoch_no=0, learning_rate=1e-3,
                              output_img_freq=500)).to(dev).eval()
        timing = time_rounds({"off": lambda: call(model, False), "mirror": lambda: call(model, "mirror")}, args.predict_rounds)
        ratios = sorted((timing["mirror"]["min_ms"] / timing["off"]["max_ms"], timing["mirror"]["max_ms"] / timing["off"]["min_ms"]))
        out[name] = {**timing, "mirror_over_off_median": timing["mirror"]["median_ms"] / timing["off"]["median_ms"],
                     "mirror_over_off_range": ratios}
        del model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--predict_batch", type=int, default=8)
    ap.add_argument("--predict_rounds", type=int, default=15)
    ap.add_argument("--no-predict", action="store_true", help="kernels only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    kernels, ok = bench_kernels(args, dev)
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "argv": sys.argv[1:], "kernels": kernels}
    if not args.no_predict:
        result["predictions"] = bench_predictions(args, dev)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not ok:
        raise SystemExit("bench_tta: a kernel is slower than the unfused composition beyond the spread of the rounds, or their bits differ")


if __name__ == "__main__":
    main()
