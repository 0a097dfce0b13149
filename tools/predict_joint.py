"""Road maps AND boxes from six camera frames alone, with the joint model (``JointRoadMapBBox.predict``), and what the one pass saves.

    python tools/predict_joint.py [--ckpt joint.ckpt] [--frames frames.npy] [--scenes 16] [--batch_size 8] [--threshold 0.4]
                                  [--box_threshold 0.3] [--tta_mirror] [--mc_samples 16] [--mc_seed 0] [--out preds/]
                                  [--timing profiles/joint_predict_timing.json]

Model: ``--ckpt`` a checkpoint ``JointRoadMapBBox.save_checkpoint`` wrote (its calibrated ``rm_threshold`` and ``box_threshold`` are
the default operating points of ``--threshold`` and ``--box_threshold``, 0.5 where it has none), else a freshly initialised model at
the reference's sizes (hidden 128 / latent 64, seeded).  Input: ``--frames`` a .npy of
decoded camera frames, uint8 [S,6,H,W,3], or of views as ToTensor delivers them, fp32 [S,6,3,H,W]; without it ``--scenes``
closed-form synthetic scenes (driving_dirty_amd/synth.py).  Printed per batch: the road fraction of the predicted map and the number of
boxes per scene; with ``--out``, ``road_map_00000.npy`` (bool [800,800]) and ``boxes_00000.npy`` ([n,2,4]) per scene.
``--tta_mirror``: the scenes are predicted with mirror test-time averaging (driving_dirty_amd/tta.py); without it the checkpoint's own
``tta_mirror`` flag decides.  The three timed paths below always run with the averaging off (they compare one pass with two); in the
averaged mode a fourth, ``predict_tta``, is timed beside them and its ratio to ``predict`` is reported.  ``--mc_samples S`` /
``--mc_seed N``: the road map is the mean of S dropout draws of the encoder's tail per scene (driving_dirty_amd/mc.py) and the box head
reads it thresholded; without them the checkpoint's own values decide.  The timed paths run with one draw; with S > 1 ``predict_mc`` is
timed beside them.

Then the first batch is timed three ways in this process, between two device events each, after ``--warmup`` calls of each: ``predict(x)``;
the composition ``predict_road_map(x)`` followed by ``predict_boxes(x, masks)``, which is what the model offered before ``predict``
existed (two passes of the encoder's conv stack); and the encoder's conv stack forward alone, the work the one pass should save.  The three
take turns for ``--rounds`` rounds, so all see the same machine.  Printed and, with ``--timing``, written as JSON: milliseconds per
call, median with the fastest and the slowest round beside it (the spread to read a difference against), and whether ``predict`` is
no slower than the composition beyond that spread; the exit status says the same."""
import argparse
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import mc, ops, synth, tta  # noqa: E402
from driving_dirty_amd.autoencoder import BasicAE  # noqa: E402
from driving_dirty_amd.joint import JointRoadMapBBox  # noqa: E402


def load_model(args, dev):
    if args.ckpt:
        return JointRoadMapBBox.load_from_checkpoint(args.ckpt).to(dev).eval()
    torch.manual_seed(args.seed)
    ae = BasicAE(Namespace(hidden_dim=args.hidden_dim, latent_dim=args.latent_dim))
    return JointRoadMapBBox(Namespace(pretrained_ae=ae, learning_rate=1e-3, output_img_freq=500)).to(dev).eval()


def load_scenes(args, model, dev):
    """-> list of batches, each what ``forward`` takes."""
    if args.frames:
        a = np.load(args.frames)
        if a.ndim != 5 or a.shape[1] != 6 or not ((a.dtype == np.uint8 and a.shape[4] == 3) or (a.dtype == np.float32 and a.shape[2] == 3)):
            raise SystemExit(f"predict_joint: {args.frames}: expected uint8 [S,6,H,W,3] or float32 [S,6,3,H,W], got {a.dtype} {a.shape}")
        scenes = torch.from_numpy(a)
    else:
        enc = model.ae.encoder
        scenes = synth.camera_batch(args.scenes, enc.input_height, enc.input_width // 6, seed=args.seed)
    batches = []
    for i in range(0, scenes.size(0), args.batch_size):
        chunk = scenes[i:i + args.batch_size].to(dev)
        batches.append(tuple(chunk) if chunk.dtype == torch.uint8 else chunk.contiguous())      # frames go per sample, as the collate leaves them
    return batches


def timed_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def summary(ms):
    s = sorted(ms)
    return {"ms_median": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ckpt", default="")
    ap.add_argument("--frames", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--hidden_dim", type=int, default=128)
    ap.add_argument("--latent_dim", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--box_threshold", type=float, default=None)
    ap.add_argument("--tta_mirror", action="store_true", help="mirror test-time averaging (default: as the checkpoint's hparams say)")
    ap.add_argument("--mc_samples", type=int, default=None, help="dropout draws per scene the road map is averaged over, 1 .. 64 (default: as the checkpoint's hparams say)")
    ap.add_argument("--mc_seed", type=int, default=None, help="seed of those draws (default: as the checkpoint's hparams say, else 0)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--timing", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_joint: needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    model = load_model(args, dev)
    tau = args.threshold if args.threshold is not None else (model.rm_threshold if model.rm_threshold is not None else 0.5)
    box_tau = args.box_threshold if args.box_threshold is not None else (model.box_threshold if model.box_threshold is not None else 0.5)
    batches = load_scenes(args, model, dev)
    mode = tta.resolve(model, True if args.tta_mirror else None)
    if args.mc_seed is not None:
        model.hparams.mc_seed = args.mc_seed
        mc.seed_of(model)      # refuses a negative one by name
    draws = mc.resolve(model, args.mc_samples)

    if args.out:
        os.makedirs(args.out, exist_ok=True)
    n, counts, road_px = 0, [], 0
    for x in batches:
        pred = model.predict_mode(x, mode is not None, tau, box_tau, mc_samples=draws)
        counts += [int(t.shape[0]) for t in pred.boxes]
        road_px += int(pred.road_map.sum())
        print(f"scenes {n} .. {n + len(pred.boxes) - 1}: road fraction {float(pred.road_map.float().mean()):.4f}, "
              f"boxes per scene {[int(t.shape[0]) for t in pred.boxes]}")
        for m, bx in zip(pred.road_map.cpu().numpy(), pred.boxes):
            if args.out:
                np.save(os.path.join(args.out, f"road_map_{n:05d}.npy"), m)
                np.save(os.path.join(args.out, f"boxes_{n:05d}.npy"), bx.cpu().numpy())
            n += 1

    x = batches[0]
    b = len(x)
    enc = model.ae.encoder
    with torch.no_grad():
        wide4 = ops.wide_image(tuple(t.contiguous() for t in x) if isinstance(x, tuple) else x)

    def composition():
        masks = model.predict_road_map(x, tau, mc_samples=1, tta=False)
        return model.predict_boxes(x, tuple(masks), box_tau, tta=False)

    def conv_stack():
        with torch.no_grad():
            return ops.encoder_conv_stack(wide4, enc.c1, enc.c2, enc.c3, 2, enc.rows_per_task)

    paths = {"predict": lambda: model.predict_mode(x, False, tau, box_tau, mc_samples=1), "road_map_then_boxes": composition, "encoder_conv_forward": conv_stack}
    torch.manual_seed(args.seed)      # the dense blocks' dropout is on in eval mode too (components.py:108): the same masks both ways
    one = paths["predict"]()
    torch.manual_seed(args.seed)
    two = composition()
    same = len(one.boxes) == len(two) and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(one.boxes, two))
    if mode is not None:
        paths["predict_tta"] = lambda: model.predict_mode(x, True, tau, box_tau, mc_samples=1)
    if draws > 1:
        paths["predict_mc"] = lambda: model.predict_mode(x, False, tau, box_tau, mc_samples=draws)
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, fn in paths.items():
            ms[k].append(timed_ms(fn))
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "argv": sys.argv[1:], "hidden_dim": enc.hidden_dim, "latent_dim": enc.latent_dim, "batch": b, "rounds": args.rounds,
              "warmup": args.warmup, "threshold": tau, "box_threshold": box_tau, "tta": mode, "mc_samples": draws, "mc_seed": mc.seed_of(model), "scenes_predicted": n,
              "road_fraction": road_px / (n * 800 * 800), "boxes_per_scene_mean": sum(counts) / max(n, 1), "same_boxes_both_ways": same}
    for k, v in ms.items():
        result[k] = summary(v)
        print(f"{k}: {result[k]['ms_median']:.3f} ms per batch of {b} (rounds {result[k]['ms_min']:.3f} .. {result[k]['ms_max']:.3f})")
    if mode is not None:
        result["tta_over_plain"] = result["predict_tta"]["ms_median"] / result["predict"]["ms_median"]
    if draws > 1:
        result["mc_over_plain"] = result["predict_mc"]["ms_median"] / result["predict"]["ms_median"]
    p, c = result["predict"], result["road_map_then_boxes"]
    spread = max(p["ms_max"] - p["ms_min"], c["ms_max"] - c["ms_min"])
    result["saving_ms_median"] = c["ms_median"] - p["ms_median"]
    result["spread_ms"] = spread
    result["predict_not_slower"] = bool(p["ms_median"] <= c["ms_median"] + spread)
    print(f"one pass saves {result['saving_ms_median']:.3f} ms of {c['ms_median']:.3f} (encoder conv forward alone: "
          f"{result['encoder_conv_forward']['ms_median']:.3f} ms; spread of the rounds {spread:.3f} ms); same boxes both ways: {same}")
    print(json.dumps(result))
    if args.timing:
        os.makedirs(os.path.dirname(os.path.abspath(args.timing)), exist_ok=True)
        with open(args.timing, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not (same and result["predict_not_slower"]):
        raise SystemExit("predict_joint: predict is slower than the two-call composition, or the two disagree")


if __name__ == "__main__":
    main()
