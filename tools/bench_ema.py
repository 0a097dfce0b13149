"""Time the weight-averaging kernels (csrc/ema.hip) beside the torch compositions they replace, and the training step with the
average off, on and on every fourth step.

    python tools/bench_ema.py [--reps 25] [--step_rounds 8] [--block 8] [--batch 32] [--no-step] [--out profiles/ema_timing.json]

THE PASS, over config 2's real parameter list at the reference's sizes (bench.build_model: hidden 128 / latent 64, 161 M parameters):
``dd_ema_update_ptrs`` against ``torch._foreach_lerp_(shadows, params, alpha)`` on the same tensors in this process, and
``dd_ema_swap_ptrs`` against the exchange through a temporary, three ``torch._foreach_copy_`` calls.  HIP events around single calls
on preallocated tensors, a warm-up, then ``reps`` ROUNDS in which every candidate runs once, so that clock drift falls on all alike;
the median with the fastest and the slowest round beside it.  THE CONDITION, which the exit status reports: each kernel is no slower
than its composition beyond the spread of the rounds.  Bytes are computed from the sizes -- the update reads the average and the
parameter and writes the average, 12 bytes per element; the exchange reads and writes both, 16 -- and given with the resulting rate.
Weights plus shadows are 1.3 GB, five times the 256 MiB Infinity Cache, and every byte is touched once per call: the rate IS an HBM
figure.  Beside it, with no bound set: the rate ``dd_adam_step`` reaches on the extractor's fc1 weight in the same rounds (28 bytes
per element), the project's own streaming yardstick.

THE STEP (unless ``--no-step``): ``train.TrainStep`` on config 2 at bs 32, three twins taking turns -- the average off, on, and on with
``every=4`` -- once with the extractor trained and once with it frozen.  A turn is a block of ``--block`` steps between two HIP
events (a multiple of 4, so that a block holds its share of updates); milliseconds per step as the median over ``--step_rounds``
rounds, and the differences to "off".  No bound is set on them."""
import argparse
import json
import os
import sys
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (config 2's model and batch)
from driving_dirty_amd import ema, ops  # noqa: E402

ALPHA = 1e-3
DECAY = 0.999


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


def rate(timing, nbytes):
    timing["bytes"] = nbytes
    timing["GB_per_s"] = nbytes / timing["median_ms"] / 1e6


def bench_pass(args, dev):
    model = bench.build_model(dev)
    params = [p.detach() for p in model.parameters()]
    shadows = [p.clone().add_(1e-3) for p in params]
    temps = [torch.empty_like(p) for p in params]
    update_table, swap_table = ema.pointer_tables(shadows, params), ema.pointer_tables(params, shadows)
    fc1 = max(params, key=lambda p: p.numel()).clone().reshape(-1)
    g, m, v = torch.full_like(fc1, 1e-4), torch.zeros_like(fc1), torch.zeros_like(fc1)

    def swap_through_a_temporary():
        torch._foreach_copy_(temps, params)
        torch._foreach_copy_(params, shadows)
        torch._foreach_copy_(shadows, temps)

    # the same bits?  the composition rounds alpha * (w - e) on its own where the kernel does not: reported, not required
    e_kernel = [s.clone() for s in shadows]
    ema.launch("dd_ema_update_ptrs", *ema.pointer_tables(e_kernel, params), ALPHA)
    e_torch = [s.clone() for s in shadows]
    torch._foreach_lerp_(e_torch, params, ALPHA)
    differing = sum(int((a != b).sum()) for a, b in zip(e_kernel, e_torch))
    del e_kernel, e_torch
    candidates = {"dd_ema_update_ptrs": lambda: ema.launch("dd_ema_update_ptrs", *update_table, ALPHA),
                  "foreach_lerp": lambda: torch._foreach_lerp_(shadows, params, ALPHA),
                  "dd_ema_swap_ptrs": lambda: ema.launch("dd_ema_swap_ptrs", *swap_table),
                  "foreach_copy_x3": swap_through_a_temporary,
                  "dd_adam_step_fc1": lambda: ops.adam_step_flat(fc1, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0)}
    timing = time_rounds(candidates, args.reps)
    n = sum(p.numel() for p in params)
    rate(timing["dd_ema_update_ptrs"], 12 * n)
    rate(timing["foreach_lerp"], 12 * n)
    rate(timing["dd_ema_swap_ptrs"], 16 * n)
    rate(timing["foreach_copy_x3"], 24 * n)
    rate(timing["dd_adam_step_fc1"], 28 * fc1.numel())
    out = {"model": "config 2 (RoadMapBCE, hidden 128 / latent 64)", "tensors": len(params), "elements": n, "launches_per_call": -(-len(params) // ema.TABLE_MAX),
           "largest_tensor_elements": fc1.numel(), "alpha": ALPHA, "elements_whose_bits_differ_from_foreach_lerp": differing, "timing": timing,
           "rate_note": "weights + shadows are 1.3 GB, five times the 256 MiB Infinity Cache, every byte touched once per call: an HBM figure"}
    ok = True
    for kernel, comp in (("dd_ema_update_ptrs", "foreach_lerp"), ("dd_ema_swap_ptrs", "foreach_copy_x3")):
        spread, fine = not_slower(timing[kernel], timing[comp])
        out[kernel + "_vs_composition"] = {"speedup_median": timing[comp]["median_ms"] / timing[kernel]["median_ms"], "spread_ms": spread,
                                           "kernel_not_slower": fine}
        ok = ok and fine
    out["update_rate_over_adam_rate"] = timing["dd_ema_update_ptrs"]["GB_per_s"] / timing["dd_adam_step_fc1"]["GB_per_s"]
    return out, ok


def bench_step(args, dev):
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.roadmap import RoadMapBCE
    from driving_dirty_amd.train import TrainStep
    batch = bench.synthetic_batch(dev, args.batch, 0)
    out = {"batch": args.batch, "decay": DECAY, "steps_per_block": args.block, "rounds": args.step_rounds}
    for state, unfreeze in (("extractor_trained", 0), ("extractor_frozen", 10 ** 9)):
        steps = {}
        for name, kw in (("off", {}), ("on", {"ema_decay": DECAY}), ("every_4", {"ema_decay": DECAY, "ema_every": 4})):
            torch.manual_seed(bench.SEED)
            ae = BasicAE(Namespace(hidden_dim=bench.HIDDEN, latent_dim=bench.LATENT))
            model = RoadMapBCE(Namespace(pretrained_ae=ae, unfreeze_epoch_no=unfreeze, learning_rate=1e-3, output_img_freq=500)).to(dev)
            steps[name] = TrainStep(model, scheduler=False, **kw)
        counter = [0]

        def block(step):
            for _ in range(args.block):
                step(batch, counter[0])
                counter[0] += 1

        timing = time_rounds({k: (lambda s=s: block(s)) for k, s in steps.items()}, args.step_rounds, warmup=2)
        per_step = {k: {kk: (vv / args.block if kk.endswith("_ms") else vv) for kk, vv in t.items()} for k, t in timing.items()}
        trainable = sum(p.numel() for p in steps["on"].model.parameters() if p.requires_grad)
        out[state] = {"ms_per_step": per_step, "trainable_elements": trainable, "update_bytes": 12 * trainable,
                      "on_minus_off_ms": per_step["on"]["median_ms"] - per_step["off"]["median_ms"],
                      "every_4_minus_off_ms": per_step["every_4"]["median_ms"] - per_step["off"]["median_ms"],
                      "spread_ms": max(t["max_ms"] - t["min_ms"] for t in per_step.values())}
        for s in steps.values():
            s.close()
        del steps
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step_rounds", type=int, default=8)
    ap.add_argument("--block", type=int, default=8, help="steps per timed block, a multiple of 4")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-step", action="store_true", help="the pass only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.block < 4 or args.block % 4:
        raise SystemExit("bench_ema: --block is a multiple of 4 (every=4 then makes block / 4 updates in each)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: needs a GPU (a CPU run says nothing about these kernels)")
    dev = torch.device("cuda:0")
    passes, ok = bench_pass(args, dev)
    torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__,
              "args": {k: v for k, v in vars(args).items() if k != "out"}, "chunk": ema.CHUNK, "table_max": ema.TABLE_MAX, "pass": passes}
    if not args.no_step:
        result["step"] = bench_step(args, dev)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not ok:
        raise SystemExit("bench_ema: a kernel is slower than its torch composition beyond the spread of the rounds")


if __name__ == "__main__":
    main()
