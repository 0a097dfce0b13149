"""Rank scenes by how unsure a trained road-map model is about them: the mutual information between prediction and weights (BALD) of S
dropout draws per scene, from ``RoadMapBCE.predict_uncertainty`` (driving_dirty_amd/uncertainty.py) -- the score by which unlabelled
scenes are chosen for labelling or inspection.

    python tools/rank_uncertainty.py --rm_ckpt_path rm.ckpt --out ranked/ [--frames frames.npy] [--scenes 32] [--batch_size 32]
                                     [--mc_samples 16] [--mc_seed 0] [--maps] [--timing profiles/head_uncert_timing.json]

Input: ``--frames`` a .npy of decoded camera frames, uint8 [S,6,H,W,3], or of views as ToTensor delivers them, fp32 [S,6,3,H,W];
without it ``--scenes`` closed-form synthetic scenes (driving_dirty_amd/synth.py) at the size the checkpoint's encoder was built for.
``--mc_samples`` / ``--mc_seed``: the draws per scene (at least 2) and their seed; without them the checkpoint's own decide.  Output:
``<out>/scores.json``, the scenes ordered by their mean mutual information, largest first, each with its three scores (mean entropy,
mean mutual information, mean variance over the 640000 pixels, in nats); with ``--maps`` also ``<out>/mi_00000.npy`` ..., one fp32
[800,800] mutual-information map per scene.  The same command writes the same files.

``--timing FILE`` (needs no checkpoint: ``--rm_ckpt_path`` may be left out) times the launch alone at the head's shape (N = 640000,
K = 64), ``--batch_size`` scenes of S latents for S in ``--timing_samples``: ``dd_head_uncert`` with the scores only and with the scores
plus the mutual-information map, against its two bases on the same buffers in this process -- the torch composition (``ops.linear`` +
``ops.sigmoid`` on the ``B * S`` rows, then the same statistics in torch) and ``dd_head_mean_prob``, the same pass without the extra
epilogue.  A window is ``--iters`` calls between two ``torch.cuda.synchronize()``; after ``--warmup`` calls of each the candidates take
turns for ``--windows`` windows each, so all see the same machine; the median window with the fastest and the slowest beside it: the
spread to read a difference against."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import mc, ops, synth, uncertainty  # noqa: E402
from driving_dirty_amd.roadmap import RoadMapBCE  # noqa: E402

N, K = 800 * 800, 64


def load_scenes(args, model, dev):
    """-> list of batches, each what ``forward`` takes."""
    if args.frames:
        a = np.load(args.frames)
        if a.ndim != 5 or a.shape[1] != 6 or not ((a.dtype == np.uint8 and a.shape[4] == 3) or (a.dtype == np.float32 and a.shape[2] == 3)):
            raise SystemExit(f"rank_uncertainty: {args.frames}: expected uint8 [S,6,H,W,3] or float32 [S,6,3,H,W], got {a.dtype} {a.shape}")
        scenes = torch.from_numpy(a)
    else:
        enc = model.ae.encoder
        scenes = synth.camera_batch(args.scenes, enc.input_height, enc.input_width // 6, seed=args.seed)
    batches = []
    for i in range(0, scenes.size(0), args.batch_size):
        chunk = scenes[i:i + args.batch_size].to(dev)
        batches.append(tuple(chunk) if chunk.dtype == torch.uint8 else chunk.contiguous())      # frames go per sample, as the collate leaves them
    return batches


def rank(args, dev):
    model = RoadMapBCE.load_from_checkpoint(args.rm_ckpt_path).to(dev).eval()
    if args.mc_seed is not None:
        model.hparams.mc_seed = args.mc_seed
        mc.seed_of(model)      # refuses a negative one by name
    draws = mc.resolve(model, args.mc_samples)
    os.makedirs(args.out, exist_ok=True)
    rows = []
    for x in load_scenes(args, model, dev):
        got = model.predict_uncertainty(x, mc_samples=draws, maps=("mi",) if args.maps else (), scores=True)
        for i, s in enumerate(got.scores.cpu().tolist()):
            if args.maps:
                np.save(os.path.join(args.out, f"mi_{len(rows):05d}.npy"), got.mi[i].cpu().numpy())
            rows.append({"scene": len(rows), **dict(zip(uncertainty.SCORES, s))})
    rows.sort(key=lambda r: (-r["mi"], r["scene"]))
    result = {"model": "roadmap_bce", "mc_samples": draws, "mc_seed": mc.seed_of(model), "unit": "nats, mean over 640000 pixels",
              "ranked_by": "mi", "scenes": rows}
    with open(os.path.join(args.out, "scores.json"), "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(f"rank_uncertainty: {len(rows)} scenes, S = {draws}; most unsure: scene {rows[0]['scene']} (mi {rows[0]['mi']:.4g}), "
          f"least: scene {rows[-1]['scene']} (mi {rows[-1]['mi']:.4g})")


def composition(x, w, bias, b, samples, inv, want_map):
    """The statistics from the pieces the package had: B * S probability maps through memory, then torch."""
    with torch.no_grad():
        z = ops.linear(x, w, bias)
        p = ops.sigmoid(z).reshape(b, samples, N)
        a = z.abs().reshape(b, samples, N)
        h = torch.nn.functional.softplus(-a) + a * torch.sigmoid(-a)
        mean = p.sum(1) * inv
        entropy = -(torch.xlogy(mean, mean) + torch.xlogy(1 - mean, 1 - mean))
        mi = (entropy - h.sum(1) * inv).clamp_(min=0)
        var = ((p - mean[:, None]) ** 2).sum(1) * inv
        scores = torch.stack([entropy.double().mean(1), mi.double().mean(1), var.double().mean(1)], dim=1)
    return (mi, scores) if want_map else scores


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timing(args, dev):
    b = args.batch_size
    w = synth.hash_uniform((N, K), 32, -0.375, 0.375).to(dev)
    bias = synth.hash_uniform((N,), 33, -0.5, 0.5).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "argv": sys.argv[1:], "shape": {"n": N, "k": K, "batch": b}, "iters_per_window": args.iters, "windows": args.windows, "cases": []}
    for samples in args.timing_samples:
        x = synth.hash_uniform((b * samples, K), 31, -1.0, 1.0).to(dev)
        inv = torch.tensor(1.0 / samples, dtype=torch.float32, device=dev)
        mean = torch.empty((b, N), device=dev)
        mi = torch.empty((b, N), device=dev)
        partials = torch.empty(((N + uncertainty.BLOCK - 1) // uncertainty.BLOCK, b, 3), device=dev, dtype=torch.float64)
        scores = torch.empty((b, 3), device=dev, dtype=torch.float64)
        paths = {
            "head_uncert_scores": lambda: uncertainty.launch("dd_head_uncert", x, w, bias, None, None, None, None, partials, scores, b, samples, N, K),
            "head_uncert_scores_mi_map": lambda: uncertainty.launch("dd_head_uncert", x, w, bias, None, None, mi, None, partials, scores, b, samples, N, K),
            "head_mean_prob": lambda: mc.launch("dd_head_mean_prob", x, w, bias, mean, b, samples, N, K),
            "torch_composition_scores": lambda: composition(x, w, bias, b, samples, inv, False),
            "torch_composition_scores_mi_map": lambda: composition(x, w, bias, b, samples, inv, True),
        }
        for fn in paths.values():
            for _ in range(args.warmup):
                fn()
        secs = {k: [] for k in paths}
        for _ in range(args.windows):
            for k, fn in paths.items():
                secs[k].append(window(fn, args.iters))
        case = {"samples": samples}
        for k, v in secs.items():
            ms = sorted(1e3 * s / args.iters for s in v)
            case[k] = {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}
            print(f"S = {samples:2d} {k}: {case[k]['ms_median']:.3f} ms per call (windows {ms[0]:.3f} .. {ms[-1]:.3f})")
        for name in ("head_uncert_scores", "head_uncert_scores_mi_map"):
            case[name + "_over_head_mean_prob"] = case[name]["ms_median"] / case["head_mean_prob"]["ms_median"]
            case[name + "_over_torch_composition"] = case[name]["ms_median"] / case["torch_composition" + name[len("head_uncert"):]]["ms_median"]
        result["cases"].append(case)
        del x, mean, mi, partials, scores
        torch.cuda.empty_cache()
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.timing)), exist_ok=True)
    with open(args.timing, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rm_ckpt_path", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", default="")
    ap.add_argument("--scenes", type=int, default=32)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--mc_samples", type=int, default=None, help="dropout draws per scene, 2 .. 64 (default: as the checkpoint's hparams say)")
    ap.add_argument("--mc_seed", type=int, default=None, help="seed of those draws (default: as the checkpoint's hparams say, else 0)")
    ap.add_argument("--maps", action="store_true", help="also write each scene's mutual-information map")
    ap.add_argument("--timing", default="")
    ap.add_argument("--timing_samples", type=lambda t: [int(v) for v in t.split(",")], default=[4, 8, 16])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    if not args.rm_ckpt_path and not args.timing:
        ap.error("give --rm_ckpt_path (and --out) to rank scenes, or --timing FILE to time the launch")
    if args.rm_ckpt_path and not args.out:
        ap.error("--rm_ckpt_path needs --out")
    if not torch.cuda.is_available():
        raise SystemExit("rank_uncertainty: needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    if args.rm_ckpt_path:
        rank(args, dev)
    if args.timing:
        timing(args, dev)


if __name__ == "__main__":
    main()
