"""Time the decoupled-weight-decay kernels (csrc/adamw.hip) beside the pass they are a mode of and beside torch.optim.AdamW, and the
training step with the decay off and on.

    python tools/bench_adamw.py [--reps 25] [--step_rounds 8] [--block 8] [--batch 32] [--no-step] [--out profiles/adamw_timing.json]

THE PASS, at the extractor's fc1 weight (128 x 940032, 481 MB; p, g, m, v 1.9 GB, seven times the 256 MiB Infinity Cache, every byte
touched once per call: the rates are HBM figures): ``dd_adamw_step`` against the parent's ``dd_adam_step`` ON THE SAME BUFFERS -- both
move 28 bytes per element --, each with one persistent workgroup per CU (the setting beside the backward) and with four (the setting
behind it); ``torch.optim.AdamW`` with ``fused=True`` and with ``foreach=True`` on buffers of their own; and ``dd_decay``, 8 bytes per
element, on fc1's weight and on the head's.  HIP events around single calls on preallocated tensors, a warm-up, then ``reps`` ROUNDS in
which every candidate runs once, so that clock drift falls on all alike; the median with the fastest and the slowest round beside it.
THE CONDITION, which the exit status reports: the fused pass is no slower than the parent's pass beyond the spread of the rounds, at
either setting.

THE STEP (unless ``--no-step``): ``train.TrainStep`` on config 2 (``bench.build_model``, ``bench.BATCH``, TrainStep's defaults), twins
taking turns: the decay off and on, and both once more with ``fuse_linear_wgrad=False`` -- there no tensor takes the rank-B pass, so
the decay is the fused kernels alone and costs no byte; with the defaults fc1 and the head are pre-scaled by ``dd_decay`` in front of
their rank-B pass, 8 bytes per element more.  A turn is a block of ``--block`` steps between two HIP events; milliseconds per step as the
median over ``--step_rounds`` rounds, the differences, and beside them what the pre-scale's bytes cost when nothing hides them (the
``dd_decay`` medians above).  No bound is set on the step."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (config 2's model and batch)
from driving_dirty_amd import _lib, adamw, ops  # noqa: E402

LR, WD = 1e-3, 1e-2
CFG = (LR, 0.9, 0.999, 1e-8)
FC1 = (128, 940032)
HEAD = (640000, 64)


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


def not_slower(kernel, parent):
    spread = max(kernel["max_ms"] - kernel["min_ms"], parent["max_ms"] - parent["min_ms"])
    return spread, bool(kernel["median_ms"] <= parent["median_ms"] + spread)


def rate(timing, nbytes):
    timing["bytes"] = nbytes
    timing["GB_per_s"] = nbytes / timing["median_ms"] / 1e6


def bench_pass(args, dev):
    n = FC1[0] * FC1[1]
    keep = adamw.keep_of(LR, WD)
    gen = torch.Generator(device=dev).manual_seed(bench.SEED)
    p = torch.rand(n, generator=gen, device=dev) - 0.5
    g, m, v = torch.full_like(p, 1e-4), torch.zeros_like(p), torch.zeros_like(p)
    head = torch.rand(HEAD[0] * HEAD[1], generator=gen, device=dev) - 0.5
    step = [0]

    def ours(fused, blocks):
        def fn():
            _lib.call("dd_set_adam_blocks_per_cu", blocks)
            step[0] += 1
            if fused:
                adamw.step_flat(p, g, m, v, *CFG, step[0], 1.0, keep)
            else:
                ops.adam_step_flat(p, g, m, v, *CFG, step[0], 1.0)
        return fn

    def torch_adamw(**kw):
        q = torch.nn.Parameter(p.clone())
        q.grad = g.clone()
        opt = torch.optim.AdamW([q], lr=LR, weight_decay=WD, **kw)
        return opt.step

    def decay_of(t):
        def fn():
            _lib.call("dd_set_adam_blocks_per_cu", 1)
            adamw.decay(t, keep)
        return fn

    candidates = {}
    for blocks in (1, 4):
        candidates[f"dd_adamw_step_{blocks}_per_cu"] = ours(True, blocks)
        candidates[f"dd_adam_step_{blocks}_per_cu"] = ours(False, blocks)
    candidates["torch_adamw_fused"] = torch_adamw(fused=True)
    candidates["torch_adamw_foreach"] = torch_adamw(foreach=True)
    candidates["dd_decay_fc1"] = decay_of(p)
    candidates["dd_decay_head"] = decay_of(head)
    try:
        timing = time_rounds(candidates, args.reps)
    finally:
        _lib.call("dd_set_adam_blocks_per_cu", 1)
    for name, t in timing.items():
        rate(t, 8 * (head.numel() if name == "dd_decay_head" else n) if name.startswith("dd_decay") else 28 * n)
    out = {"tensor": f"fc1 weight {FC1[0]} x {FC1[1]}", "elements": n, "head_elements": head.numel(), "lr": LR, "weight_decay": WD, "keep": keep,
           "timing": timing,
           "rate_note": "p, g, m, v are 1.9 GB, seven times the 256 MiB Infinity Cache, every byte touched once per call: HBM figures "
                        "(torch's foreach form makes several passes: its rate is of the 28 B/element it has to move, not of what it moves)"}
    ok = True
    for blocks in (1, 4):
        fused, parent = timing[f"dd_adamw_step_{blocks}_per_cu"], timing[f"dd_adam_step_{blocks}_per_cu"]
        spread, fine = not_slower(fused, parent)
        out[f"fused_vs_parent_{blocks}_per_cu"] = {"fused_over_parent_median": fused["median_ms"] / parent["median_ms"], "spread_ms": spread,
                                                    "fused_not_slower": fine}
        ok = ok and fine
    best = min(timing["dd_adamw_step_1_per_cu"]["median_ms"], timing["dd_adamw_step_4_per_cu"]["median_ms"])
    out["speedup_over_torch_fused"] = timing["torch_adamw_fused"]["median_ms"] / best
    out["speedup_over_torch_foreach"] = timing["torch_adamw_foreach"]["median_ms"] / best
    return out, ok


def bench_step(args, dev, passes):
    from driving_dirty_amd.train import TrainStep
    batch = bench.synthetic_batch(dev, args.batch, 0)
    counter = [0]

    def block(step):
        for _ in range(args.block):
            step(batch, counter[0])
            counter[0] += 1

    # one arrangement at a time: live optimizers share the backward's schedule (ops.BACKWARD_OBSERVERS), so twins of two arrangements
    # in one process would run each other's
    per_step, fused = {}, []
    for suffix, kw in (("", {}), ("_materialised", {"fuse_linear_wgrad": False})):
        steps = {"off" + suffix: TrainStep(bench.build_model(dev), scheduler=False, **kw),
                 "on" + suffix: TrainStep(bench.build_model(dev), scheduler=False, weight_decay=WD, **kw)}
        timing = time_rounds({k: (lambda s=s: block(s)) for k, s in steps.items()}, args.step_rounds, warmup=2)
        per_step.update({k: {kk: (vv / args.block if kk.endswith("_ms") else vv) for kk, vv in t.items()} for k, t in timing.items()})
        fused = fused or [list(w.shape) for w in steps["on" + suffix].fused]
        for s in steps.values():
            s.close()
        del steps
        torch.cuda.empty_cache()
    rankb = sum(a * b for a, b in fused)
    out = {"batch": args.batch, "weight_decay": WD, "steps_per_block": args.block, "rounds": args.step_rounds, "ms_per_step": per_step,
           "rankb_tensors": fused, "rankb_elements": rankb, "prescale_bytes": 8 * rankb,
           "on_minus_off_ms": per_step["on"]["median_ms"] - per_step["off"]["median_ms"],
           "on_minus_off_materialised_ms": per_step["on_materialised"]["median_ms"] - per_step["off_materialised"]["median_ms"],
           "spread_ms": max(t["max_ms"] - t["min_ms"] for t in per_step.values()),
           "prescale_alone_ms": passes["timing"]["dd_decay_fc1"]["median_ms"] + passes["timing"]["dd_decay_head"]["median_ms"]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step_rounds", type=int, default=8)
    ap.add_argument("--block", type=int, default=8, help="steps per timed block")
    ap.add_argument("--batch", type=int, default=bench.BATCH)
    ap.add_argument("--no-step", action="store_true", help="the pass only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    passes, ok = bench_pass(args, dev)
    torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "args": {k: v for k, v in vars(args).items() if k != "out"}, "pass": passes}
    if not args.no_step:
        result["step"] = bench_step(args, dev, passes)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not ok:
        raise SystemExit("bench_adamw: the fused pass is slower than the parent's pass beyond the spread of the rounds")


if __name__ == "__main__":
    main()
