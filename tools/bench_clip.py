#!/usr/bin/env python3
"""The cost of clipping by global gradient norm in the headline step (config 2, bs 32, one GPU), three forms in one process, interleaved:

    (a) after     TrainStep(adam_overlap=False)                          optimizer passes after the backward
    (b) clipped   TrainStep(adam_overlap=False, gradient_clip_val=1.0)   (a) + the norm kernels + the _dev optimizer entry points
    (c) overlap   TrainStep()                                            the default: passes beside the backward

    python tools/bench_clip.py --steps 10 --warmup 3 [--rounds 2] [--out profiles/clip_step_timing.json]

(b) - (a) is what clipping costs; (a) - (c) is the known worth of the overlap.  One JSON line per form and round.
DD_HOTPATH_LIB=other/libdd_hotpath.so runs (a) and (c) on another build (the parent's: it has no (b))."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from driving_dirty_amd.train import TrainStep  # noqa: E402

FORMS = {"after": dict(adam_overlap=False), "clipped": dict(adam_overlap=False, gradient_clip_val=1.0), "overlap": dict()}


def run(form, dev, steps, warmup):
    model = bench.build_model(dev)
    batch = bench.synthetic_batch(dev, bench.BATCH, 0)
    ts = TrainStep(model, scheduler=False, **FORMS[form])
    for i in range(warmup):
        ts(batch, i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ts(batch, warmup + i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    line = {"form": form, "step_ms": round(ms, 4), "steps": steps, "warmup": warmup, "batch": bench.BATCH,
            "fc1_grad_is_none": model.ae.encoder.fc1.fc1.weight.grad is None}
    if form == "clipped":
        line["grad_norm"], line["clip_coef"] = float(ts.optimizer.grad_norm), float(ts.optimizer.clip_coef)
    ts.close()
    del ts, model, batch
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--forms", default="after,clipped,overlap")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for r in range(a.rounds):
        for form in a.forms.split(","):
            line = dict(run(form, dev, a.steps, a.warmup), round=r, lib=os.environ.get("DD_HOTPATH_LIB", "tree"))
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
