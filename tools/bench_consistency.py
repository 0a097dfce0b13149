"""Time the mirror consistency loss kernels (csrc/consistency.hip) beside the torch composition they stand in for, and the training
step without an unlabelled part and with one.

    python tools/bench_consistency.py [--reps 25] [--step_rounds 6] [--block 4] [--no-step] [--out profiles/consistency_timing.json]

THE PASS, at (16,800,800) and (32,800,800) pairs of logit maps: ``dd_cons_fwd`` and ``dd_cons_fwd_grad`` against the same loss and the
same two gradients from torch ops (``sigmoid``, ``flip``, a mean of squares, autograd) on the same buffers.  HIP events around single
calls on preallocated tensors, a warm-up, then ``reps`` ROUNDS in which every candidate runs once, so that clock drift falls on all
alike; the median with the fastest and the slowest round beside it.  A kernel call is one pass and one small finishing launch.  Bytes are
computed from the sizes -- the forward reads 2 maps, with the gradient it also writes 2: ``4 B P 4`` bytes -- and given with the resulting
rate.  At 16 pairs the four maps are 164 MB, less than the 256 MiB Infinity Cache, at 32 pairs 328 MB: the rates are NOT pure HBM
figures, and the composition in the same rounds is the yardstick, not a datasheet.

THE YARDSTICK: the kernel pair must not be slower than the torch composition beyond the spread of the rounds observed in this run
(``bench_ema.not_slower``); it moves a fraction of the composition's bytes.  Reported per shape; ``--strict`` exits non-zero on a miss.

THE STEP (unless ``--no-step``): ``train.TrainStep`` on config 2 with ``cons_weight`` 1, ONE model taking three batches in turn -- 32
labelled scenes alone (the parent's step, call for call), 16 + 2 x 16 rows and 32 + 2 x 16 rows -- in blocks of ``--block`` steps between
two HIP events; milliseconds per step as the median over ``--step_rounds`` rounds.  Only reported."""
import argparse
import json
import os
import sys
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402  (config 2's model and batch)
from bench_ema import not_slower, rate, time_rounds  # noqa: E402
from driving_dirty_amd import consistency  # noqa: E402

H = W = 800
SHAPES = (16, 32)


def bench_pass(args, dev, b):
    g = torch.Generator(device=dev).manual_seed(bench.SEED + b)
    a = (torch.rand(b, H, W, generator=g, device=dev) * 16.0 - 8.0).requires_grad_(True)
    m = (torch.rand(b, H, W, generator=g, device=dev) * 16.0 - 8.0).requires_grad_(True)
    da, dm = torch.empty_like(a), torch.empty_like(m)
    loss, stats = torch.empty(1, device=dev), torch.empty((b, 2), device=dev, dtype=torch.float64)
    nbytes = consistency.workspace_bytes(b, H * W)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    ad, md = a.detach(), m.detach()

    def composition():
        d = torch.sigmoid(a) - torch.flip(torch.sigmoid(m), dims=(1,))
        return (d * d).mean()

    def torch_fwd():
        with torch.no_grad():
            return composition()

    def torch_fwd_grad():
        return torch.autograd.grad(composition(), (a, m))

    def fwd():
        consistency.launch("dd_cons_fwd", ad, md, b, H, W, loss, stats, ws, nbytes)

    def fwd_grad():
        consistency.launch("dd_cons_fwd_grad", ad, md, b, H, W, 1.0, da, dm, loss, stats, ws, nbytes)

    # the same function?  reported with the timing: the kernels' loss and gradients against the composition's
    fwd_grad()
    ta, tm = torch_fwd_grad()
    agreement = {"loss_rel": abs(float(loss) - float(torch_fwd())) / float(torch_fwd()),
                 "da_of_peak": float((da - ta).abs().max() / ta.abs().max()), "dm_of_peak": float((dm - tm).abs().max() / tm.abs().max())}
    del ta, tm
    timing = time_rounds({"dd_cons_fwd": fwd, "torch_fwd": torch_fwd, "dd_cons_fwd_grad": fwd_grad, "torch_fwd_grad": torch_fwd_grad}, args.reps)
    n = b * H * W
    rate(timing["dd_cons_fwd"], 2 * n * 4)
    rate(timing["dd_cons_fwd_grad"], 4 * n * 4)
    out = {"pairs": b, "h": H, "w": W, "chunk": consistency.CHUNK, "workspace_bytes": nbytes, "agreement_with_the_composition": agreement, "timing": timing,
           "rate_note": "four maps are 164 MB at 16 pairs and 328 MB at 32, about the 256 MiB Infinity Cache: not pure HBM figures"}
    for kernel, torch_name in (("dd_cons_fwd", "torch_fwd"), ("dd_cons_fwd_grad", "torch_fwd_grad")):
        spread, ok = not_slower(timing[kernel], timing[torch_name])
        out[kernel + "_vs_composition"] = {"composition_over_kernel": timing[torch_name]["median_ms"] / timing[kernel]["median_ms"], "spread_ms": spread,
                                           "not_slower_within_spread": ok}
    return out


def bench_step(args, dev):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    from driving_dirty_amd.train import TrainStep
    torch.manual_seed(bench.SEED)
    ae = BasicAE(Namespace(hidden_dim=bench.HIDDEN, latent_dim=bench.LATENT))
    model = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, cons_weight=1.0)).to(dev)
    step = TrainStep(model, scheduler=False)
    full, half = bench.synthetic_batch(dev, 32, 0), bench.synthetic_batch(dev, 16, 1)
    unlabelled = bench.synthetic_batch(dev, 16, 2)[0]
    batches = {"labelled_32": full, "labelled_16_unlabelled_16": half + (unlabelled,), "labelled_32_unlabelled_16": full + (unlabelled,)}
    counter = [0]

    def block(batch):
        for _ in range(args.block):
            step(batch, counter[0])
            counter[0] += 1

    timing = time_rounds({k: (lambda v=v: block(v)) for k, v in batches.items()}, args.step_rounds, warmup=2)
    per_step = {k: {kk: (vv / args.block if kk.endswith("_ms") else vv) for kk, vv in t.items()} for k, t in timing.items()}
    rows = {"labelled_32": 32, "labelled_16_unlabelled_16": 48, "labelled_32_unlabelled_16": 64}
    out = {"steps_per_block": args.block, "rounds": args.step_rounds, "rows": rows, "ms_per_step": per_step,
           "ms_per_row": {k: per_step[k]["median_ms"] / rows[k] for k in rows},
           "rank_b_pass_kept": bool(step.fused) and model.fc1.weight.grad is None,
           "spread_ms": max(t["max_ms"] - t["min_ms"] for t in per_step.values())}
    step.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step_rounds", type=int, default=6)
    ap.add_argument("--block", type=int, default=4, help="steps per timed block")
    ap.add_argument("--no-step", action="store_true", help="the pass only")
    ap.add_argument("--strict", action="store_true", help="exit 1 when a kernel is slower than the composition beyond the spread of the rounds")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "args": {k: v for k, v in vars(args).items() if k != "out"}, "pass": {}}
    for b in SHAPES:
        result["pass"][str(b)] = bench_pass(args, dev, b)
        print(json.dumps({"pass": {str(b): result["pass"][str(b)]}}), flush=True)
        torch.cuda.empty_cache()
    if not args.no_step:
        result["step"] = bench_step(args, dev)
        print(json.dumps({"step": result["step"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ok = all(p[k + "_vs_composition"]["not_slower_within_spread"] for p in result["pass"].values() for k in ("dd_cons_fwd", "dd_cons_fwd_grad"))
    if args.strict and not ok:
        raise SystemExit("bench_consistency: a kernel is slower than the torch composition beyond the spread of the rounds")


if __name__ == "__main__":
    main()
