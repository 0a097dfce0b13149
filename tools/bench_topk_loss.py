"""Time the bootstrapped road-map loss (csrc/topk_loss.hip) beside the parent's one-pass mean BCE and the torch composition it stands in
for, and the training step with the setting off and on.

    python tools/bench_topk_loss.py [--reps 25] [--step_rounds 6] [--block 4] [--no-step] [--out profiles/topk_loss_timing.json]

THE CALL, at (32, 640000) with keep / P = 1, 0.5, 0.25, 0.1: ``dd_topk_bce`` (loss, probabilities and gradient; with keep < P three
histogram passes, three small selection launches, the final pass and the finishing launch) against
  * the parent's ``dd_bce_logits_u8`` on the same buffers (one pass: loss, probabilities, gradient): the cost of turning the feature on;
  * the torch composition (``topk`` on the margins, masked ``softplus``, autograd): what a user would otherwise write.
On two distributions of logits: ``N(0, 2^2)``, and a concentrated one -- every margin inside one binade, [1, 2), so that the leading
digit of every element of a wave falls into one bin: the case the wave aggregation in the histogram pass is there for.

The protocol is tools/bench_consistency.py's: HIP events around single calls on preallocated tensors, 3 warm-up rounds, then ``reps``
ROUNDS in which every candidate runs once, so that clock drift falls on all alike; the median with the fastest and the slowest round
beside it.  The logits and the masks are about 100 MB and stay in the 256 MiB Infinity Cache between the passes of one call: this
compares KERNELS on cache-resident operands and is not an HBM figure.  No figure was set in advance; the ratios and their spread are
reported.

THE STEP (unless ``--no-step``): ``train.TrainStep`` on config 2, ONE model taking the same 32-scene batch with the setting off (the
parent's step, call for call) and at ``rm_topk_frac`` 0.25, in blocks of ``--block`` steps between two HIP events; milliseconds per step
as the median over ``--step_rounds`` rounds.  What the loss does to a trained model's threat score cannot be measured without the data."""
import argparse
import json
import os
import sys
from argparse import Namespace

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402  (config 2's model and batch)
from bench_ema import time_rounds  # noqa: E402
from driving_dirty_amd import _lib, topk_loss  # noqa: E402

B, P = 32, 640000
FRACTIONS = (1.0, 0.5, 0.25, 0.1)


def logits_and_target(dev, which):
    g = torch.Generator(device=dev).manual_seed(bench.SEED)
    t = torch.rand(B, P, generator=g, device=dev) < 1.0 / 3.0
    if which == "normal":
        z = torch.randn(B, P, generator=g, device=dev) * 2.0
    else:      # every margin in [1, 2): one binade
        u = 1.0 + torch.rand(B, P, generator=g, device=dev)
        z = torch.where(t, -u, u)
    return z.contiguous().requires_grad_(True), t.to(torch.uint8).contiguous()


def bench_call(args, dev, which):
    z, t = logits_and_target(dev, which)
    zd, tb = z.detach(), t.bool()
    n = B * P
    probs, dz = torch.empty_like(zd), torch.empty_like(zd)
    losses, stats = torch.empty(2, device=dev), torch.empty((B, 4), device=dev, dtype=torch.float64)
    nbytes = topk_loss.workspace_bytes(B, P)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    loss1 = torch.empty((), device=dev)
    ws1 = torch.empty(_lib.size("dd_loss_workspace_bytes", n), device=dev, dtype=torch.uint8)

    def parent():
        _lib.call("dd_bce_logits_u8", zd, t, loss1, dz, probs, n, 1.0, ws1)

    def kernel(keep):
        return lambda: topk_loss.launch("dd_topk_bce", zd, t, B, P, keep, 1.0, probs, dz, losses, stats, ws, nbytes)

    def composition(keep):
        def fn():
            u = torch.where(tb, -z, z)
            tau = torch.topk(u.detach(), keep, dim=1).values[:, -1:]
            mask = u.detach() >= tau
            loss = ((F.softplus(u) * mask).sum(1) / mask.sum(1)).mean()
            return loss, torch.autograd.grad(loss, z)[0]
        return fn

    out = {"distribution": which, "batch": B, "per_sample": P, "workspace_bytes": nbytes, "keep": {}}
    candidates = {"dd_bce_logits_u8": parent}
    for frac in FRACTIONS:
        keep = max(1, int(round(frac * P)))
        kernel(keep)()
        w_loss, w_grad = composition(keep)()
        out["keep"][str(frac)] = {"keep": keep, "agreement_with_the_composition": {
            "loss_rel": abs(float(losses[0]) - float(w_loss)) / float(w_loss), "grad_of_peak": float((dz - w_grad).abs().max() / w_grad.abs().max()),
            "kept_share": float(stats[:, 0].sum()) / n}}
        del w_loss, w_grad
        candidates[f"dd_topk_bce@{frac}"] = kernel(keep)
        candidates[f"torch@{frac}"] = composition(keep)
    timing = time_rounds(candidates, args.reps)
    out["timing"] = timing
    base = timing["dd_bce_logits_u8"]
    for frac in FRACTIONS:
        k, c = timing[f"dd_topk_bce@{frac}"], timing[f"torch@{frac}"]
        out["keep"][str(frac)].update({
            "over_parent_pass": k["median_ms"] / base["median_ms"], "extra_ms_over_parent_pass": k["median_ms"] - base["median_ms"],
            "composition_over_kernel": c["median_ms"] / k["median_ms"],
            "spread_ms": max(k["max_ms"] - k["min_ms"], base["max_ms"] - base["min_ms"], c["max_ms"] - c["min_ms"])})
    out["note"] = ("logits and masks are about 100 MB and stay in the 256 MiB Infinity Cache between the passes of a call: a comparison of kernels on "
                   "cache-resident operands, not an HBM figure")
    return out


def bench_step(args, dev):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    from driving_dirty_amd.train import TrainStep
    torch.manual_seed(bench.SEED)
    ae = BasicAE(Namespace(hidden_dim=bench.HIDDEN, latent_dim=bench.LATENT))
    model = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, rm_topk_frac=0.25)).to(dev)
    on = model.topk
    step = TrainStep(model, scheduler=False)
    batch = bench.synthetic_batch(dev, 32, 0)
    counter = [0]

    def block(setting):
        model.topk = setting      # None: the parent's step, call for call
        for _ in range(args.block):
            step(batch, counter[0])
            counter[0] += 1

    timing = time_rounds({"off": lambda: block(None), "rm_topk_frac_0.25": lambda: block(on)}, args.step_rounds, warmup=2)
    per_step = {k: {kk: (vv / args.block if kk.endswith("_ms") else vv) for kk, vv in t.items()} for k, t in timing.items()}
    out = {"steps_per_block": args.block, "rounds": args.step_rounds, "ms_per_step": per_step,
           "on_over_off": per_step["rm_topk_frac_0.25"]["median_ms"] / per_step["off"]["median_ms"],
           "extra_ms_per_step": per_step["rm_topk_frac_0.25"]["median_ms"] - per_step["off"]["median_ms"],
           "rank_b_pass_kept": bool(step.fused) and model.fc1.weight.grad is None,
           "spread_ms": max(t["max_ms"] - t["min_ms"] for t in per_step.values())}
    step.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step_rounds", type=int, default=6)
    ap.add_argument("--block", type=int, default=4, help="steps per timed block")
    ap.add_argument("--no-step", action="store_true", help="the call only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk_loss: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "args": {k: v for k, v in vars(args).items() if k != "out"}, "call": {}}
    for which in ("normal", "one_binade"):
        result["call"][which] = bench_call(args, dev, which)
        print(json.dumps({"call": {which: result["call"][which]}}), flush=True)
        torch.cuda.empty_cache()
    if not args.no_step:
        result["step"] = bench_step(args, dev)
        print(json.dumps({"step": result["step"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
