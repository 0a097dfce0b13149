"""Time the road-map loss kernels (csrc/rm_loss.hip) beside the pass they stand in for, and the training step with the loss off and on.

    python tools/bench_rm_loss.py [--reps 25] [--step_rounds 8] [--block 8] [--batch 32] [--no-step] [--out profiles/rm_loss_timing.json]

THE PASS, at (batch, 640000) with the collate's per-sample masks read through a pointer table: the parent's ``dd_bce_logits_u8_ptrs``
(loss, probabilities and gradient in ONE pass: what ``ops.BceWithLogitsProbs`` runs for forward + backward) against
``dd_rm_loss_fwd_u8_ptrs`` and ``dd_rm_loss_bwd_u8_ptrs``, alone and one after the other.  HIP events around single calls on preallocated
tensors, a warm-up, then ``reps`` ROUNDS in which every candidate runs once, so that clock drift falls on all alike; the median with the
fastest and the slowest round beside it.  Every call is a big kernel and one small launch behind it (the parent's final sum, the
forward's finalise) except the backward, which is one kernel.  Bytes are computed from the sizes -- per element the parent reads 4 + 1
and writes 4 + 4, each new pass reads 4 + 1 and writes 4 -- and given with the resulting rate.  At batch 32 a call moves 184 to 266 MB
and the logits, probabilities and gradient together are 246 MB: about the 256 MiB Infinity Cache, so the rates are NOT pure HBM figures;
the parent's call in the same rounds is the yardstick, not a datasheet.

THE YARDSTICK: each new pass should reach the parent kernel's bytes/s to within the spread of the parent's own rounds, and forward +
backward should cost about the traffic ratio (368 / 266) of the parent's call plus two launches.  Both are reported, neither is enforced.

THE STEP (unless ``--no-step``): ``train.TrainStep`` on config 2 at bs 32, two twins taking turns -- ``rm_ts_weight`` 0 (the parent's
step, call for call) and 1 -- in blocks of ``--block`` steps between two HIP events; milliseconds per step as the median over
``--step_rounds`` rounds, and the difference.  No bound is set on it."""
import argparse
import ctypes as C
import json
import os
import sys
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402  (config 2's model and batch)
from bench_ema import rate, time_rounds  # noqa: E402
from driving_dirty_amd import ops, rm_loss  # noqa: E402

PER = 640000


def bench_pass(args, dev):
    b, per = args.batch, PER
    logits = (torch.rand(b, per, device=dev) * 16.0 - 8.0).contiguous()
    masks = tuple((torch.rand(b, per, device=dev) < 0.3).unbind(0))
    table = (C.c_void_p * b)(*[m.data_ptr() for m in masks])
    loss, dz, probs = torch.empty((), device=dev), torch.empty_like(logits), torch.empty_like(logits)
    ws_old = ops._loss_ws(b * per, dev)
    losses, stats, coef = torch.empty(3, device=dev), torch.empty((b, 5), device=dev, dtype=torch.float64), torch.empty((b, 4), device=dev)
    nbytes = rm_loss.workspace_bytes(b, per)
    ws_new = torch.empty(nbytes, device=dev, dtype=torch.uint8)

    def parent():
        ops.call("dd_bce_logits_u8_ptrs", logits, table, b, per, loss, dz, probs, 1.0, ws_old)

    def fwd():
        rm_loss.launch("dd_rm_loss_fwd_u8_ptrs", logits, table, b, per, rm_loss.POS_WEIGHT_AUTO, 1.0, 1.0, 1.0, probs, losses, stats, coef, ws_new, nbytes)

    def bwd():
        rm_loss.launch("dd_rm_loss_bwd_u8_ptrs", probs, table, b, per, coef, 1.0, dz)

    def both():
        fwd()
        bwd()

    timing = time_rounds({"parent_bce_logits_u8_ptrs": parent, "rm_loss_fwd": fwd, "rm_loss_bwd": bwd, "rm_loss_fwd_bwd": both}, args.reps)
    n = b * per
    rate(timing["parent_bce_logits_u8_ptrs"], 13 * n)
    rate(timing["rm_loss_fwd"], 9 * n)
    rate(timing["rm_loss_bwd"], 9 * n)
    rate(timing["rm_loss_fwd_bwd"], 18 * n)
    old = timing["parent_bce_logits_u8_ptrs"]
    spread_ms = old["max_ms"] - old["min_ms"]
    # the parent's rate at the slow end of its own rounds: what "within the spread" means as a rate
    floor = old["bytes"] / old["max_ms"] / 1e6
    out = {"batch": b, "per_sample": per, "chunk": rm_loss.CHUNK, "workspace_bytes": nbytes, "timing": timing,
           "parent_spread_ms": spread_ms, "parent_GB_per_s_at_its_slowest_round": floor,
           "traffic_ratio": 18.0 / 13.0, "time_ratio_fwd_bwd_over_parent": timing["rm_loss_fwd_bwd"]["median_ms"] / old["median_ms"],
           "rate_note": "logits + probabilities + gradient are about the size of the Infinity Cache at batch 32: not pure HBM figures"}
    for k in ("rm_loss_fwd", "rm_loss_bwd"):
        out[k + "_rate_over_parent_rate"] = timing[k]["GB_per_s"] / old["GB_per_s"]
        out[k + "_reaches_parent_rate_within_spread"] = bool(timing[k]["GB_per_s"] >= floor)
    return out


def bench_step(args, dev):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    from driving_dirty_amd.train import TrainStep
    batch = bench.synthetic_batch(dev, args.batch, 0)
    steps = {}
    for name, hp in (("rm_ts_weight_0", {"rm_ts_weight": 0.0}), ("rm_ts_weight_1", {"rm_ts_weight": 1.0})):
        torch.manual_seed(bench.SEED)
        ae = BasicAE(Namespace(hidden_dim=bench.HIDDEN, latent_dim=bench.LATENT))
        model = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500, **hp)).to(dev)
        steps[name] = TrainStep(model, scheduler=False)
    assert steps["rm_ts_weight_0"].model.rm_loss is None and steps["rm_ts_weight_1"].model.rm_loss is not None
    counter = [0]

    def block(step):
        for _ in range(args.block):
            step(batch, counter[0])
            counter[0] += 1

    timing = time_rounds({k: (lambda s=s: block(s)) for k, s in steps.items()}, args.step_rounds, warmup=2)
    per_step = {k: {kk: (vv / args.block if kk.endswith("_ms") else vv) for kk, vv in t.items()} for k, t in timing.items()}
    out = {"batch": args.batch, "steps_per_block": args.block, "rounds": args.step_rounds, "ms_per_step": per_step,
           "on_minus_off_ms": per_step["rm_ts_weight_1"]["median_ms"] - per_step["rm_ts_weight_0"]["median_ms"],
           "spread_ms": max(t["max_ms"] - t["min_ms"] for t in per_step.values())}
    for s in steps.values():
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step_rounds", type=int, default=8)
    ap.add_argument("--block", type=int, default=8, help="steps per timed block")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-step", action="store_true", help="the pass only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not 1 <= args.batch <= rm_loss.TABLE_MAX:
        raise SystemExit(f"bench_rm_loss: --batch is 1 .. {rm_loss.TABLE_MAX} (the pointer table)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rm_loss: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "args": {k: v for k, v in vars(args).items() if k != "out"}, "pass": bench_pass(args, dev)}
    print(json.dumps({"pass": result["pass"]}), flush=True)
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
