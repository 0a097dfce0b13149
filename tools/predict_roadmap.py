"""Predict binary road maps from a trained road-map checkpoint: the reference README's "Predicting test images" step
(``run_test.py --rm_ckpt_path ...``) on the HIP hot path.

    python tools/predict_roadmap.py --rm_ckpt_path rm.ckpt --out maps/ [--model roadmap_bce|roadmap_mse] [--frames frames.npy]
                                    [--scenes 32] [--batch_size 32] [--threshold 0.4] [--tta_mirror] [--mc_samples 16] [--mc_seed 0]
                                    [--timing profiles/predict_timing.json]

Input: ``--frames`` a .npy of decoded camera frames, uint8 [S,6,H,W,3], or of views as ToTensor delivers them, fp32 [S,6,3,H,W];
without it ``--scenes`` closed-form synthetic scenes (driving_dirty_amd/synth.py) at the size the checkpoint's encoder was built
for.  Output: ``<out>/road_map_00000.npy`` ... one bool [800,800] map per scene, from ``predict_road_map`` at ``--threshold``
(default: the threshold the checkpoint was calibrated to, else 0.5).  ``--tta_mirror``: the maps are predicted with mirror test-time
averaging (the mean of the scene's and the mirrored scene's probabilities, driving_dirty_amd/tta.py); without it the checkpoint's own
``tta_mirror`` flag decides.  The timing below then has a third path, ``predict_road_map_tta``.  ``--mc_samples S``: the maps are the
mean of S dropout draws of the encoder's tail per scene (driving_dirty_amd/mc.py), seeded by ``--mc_seed``, so the same command writes
the same maps; without them the checkpoint's own ``mc_samples`` / ``mc_seed`` decide.  The timing then has the path ``predict_road_map_mc``.

Then the first batch is timed both ways in this process: ``predict_road_map`` (encoder -> dd_linear_sigmoid_gt) and ``forward``
followed by ``> tau`` in torch.  A window is ``--iters`` calls between two ``torch.cuda.synchronize()``; after ``--warmup``
calls of each path the two paths take turns for ``--windows`` windows each, so both see the same machine.  Printed and, with
``--timing``, written as JSON: scenes/s per path (median window, fastest and slowest beside it: the spread to read a difference
against)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import mc, synth, tta  # noqa: E402
from driving_dirty_amd.roadmap import RoadMap, RoadMapBCE  # noqa: E402

MODELS = {"roadmap_bce": RoadMapBCE, "roadmap_mse": RoadMap}      # the reference's registry names


def load_scenes(args, model, dev):
    """-> list of batches, each what ``forward`` takes."""
    if args.frames:
        a = np.load(args.frames)
        if a.ndim != 5 or a.shape[1] != 6 or not ((a.dtype == np.uint8 and a.shape[4] == 3) or (a.dtype == np.float32 and a.shape[2] == 3)):
            raise SystemExit(f"predict_roadmap: {args.frames}: expected uint8 [S,6,H,W,3] or float32 [S,6,3,H,W], got {a.dtype} {a.shape}")
        scenes = torch.from_numpy(a)
    else:
        enc = model.ae.encoder
        scenes = synth.camera_batch(args.scenes, enc.input_height, enc.input_width // 6, seed=args.seed)
    batches = []
    for i in range(0, scenes.size(0), args.batch_size):
        chunk = scenes[i:i + args.batch_size].to(dev)
        batches.append(tuple(chunk) if chunk.dtype == torch.uint8 else chunk.contiguous())      # frames go per sample, as the collate leaves them
    return batches


def unfused(model, x, tau):
    with torch.no_grad():
        out = model(x)
        return (out[1] if isinstance(out, tuple) else out) > tau


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rm_ckpt_path", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--model", choices=sorted(MODELS), default="roadmap_bce")
    ap.add_argument("--frames", default="")
    ap.add_argument("--scenes", type=int, default=32)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--tta_mirror", action="store_true", help="mirror test-time averaging (default: as the checkpoint's hparams say)")
    ap.add_argument("--mc_samples", type=int, default=None, help="dropout draws per scene the map is averaged over, 1 .. 64 (default: as the checkpoint's hparams say)")
    ap.add_argument("--mc_seed", type=int, default=None, help="seed of those draws (default: as the checkpoint's hparams say, else 0)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--timing", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_roadmap: needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    model = MODELS[args.model].load_from_checkpoint(args.rm_ckpt_path).to(dev).eval()
    tau = args.threshold if args.threshold is not None else (model.rm_threshold if model.rm_threshold is not None else 0.5)
    batches = load_scenes(args, model, dev)
    mode = tta.resolve(model, True if args.tta_mirror else None)
    if args.mc_seed is not None:
        model.hparams.mc_seed = args.mc_seed
        mc.seed_of(model)      # refuses a negative one by name
    draws = mc.resolve(model, args.mc_samples)

    os.makedirs(args.out, exist_ok=True)
    n = 0
    for x in batches:
        for m in model.predict_road_map(x, tau, mc_samples=draws, tta=mode is not None).cpu().numpy():
            np.save(os.path.join(args.out, f"road_map_{n:05d}.npy"), m)
            n += 1

    x = batches[0]
    b = len(x)
    paths = {"predict_road_map": lambda: model.predict_road_map(x, tau, mc_samples=1, tta=False), "forward_then_torch_threshold": lambda: unfused(model, x, tau)}
    if mode is not None:
        paths["predict_road_map_tta"] = lambda: model.predict_road_map(x, tau, mc_samples=1, tta=True)
    if draws > 1:
        paths["predict_road_map_mc"] = lambda: model.predict_road_map(x, tau, mc_samples=draws, tta=False)
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    secs = {k: [] for k in paths}
    for _ in range(args.windows):
        for k, fn in paths.items():
            secs[k].append(window(fn, args.iters))
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "argv": sys.argv[1:], "model": args.model, "precision": model.ae.encoder.precision, "threshold": tau, "tta": mode, "mc_samples": draws, "mc_seed": mc.seed_of(model), "scenes_written": n,
              "batch": b, "iters_per_window": args.iters, "windows": args.windows}
    for k, v in secs.items():
        rate = sorted(b * args.iters / s for s in v)
        result[k] = {"scenes_per_s_median": rate[len(rate) // 2], "scenes_per_s_min": rate[0], "scenes_per_s_max": rate[-1],
                     "ms_per_batch_median": 1e3 * sorted(v)[len(v) // 2] / args.iters}
        print(f"{k}: {result[k]['scenes_per_s_median']:.1f} scenes/s (windows {rate[0]:.1f} .. {rate[-1]:.1f}), "
              f"{result[k]['ms_per_batch_median']:.3f} ms per batch of {b}")
    if mode is not None:
        result["tta_over_plain"] = result["predict_road_map_tta"]["ms_per_batch_median"] / result["predict_road_map"]["ms_per_batch_median"]
    if draws > 1:
        result["mc_over_plain"] = result["predict_road_map_mc"]["ms_per_batch_median"] / result["predict_road_map"]["ms_per_batch_median"]
    print(json.dumps(result))
    if args.timing:
        os.makedirs(os.path.dirname(os.path.abspath(args.timing)), exist_ok=True)
        with open(args.timing, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
