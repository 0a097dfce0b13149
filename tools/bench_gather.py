#!/usr/bin/env python3
"""The camera-gather entry points (csrc/camera_gather.hip: dd_stitch6*, dd_view_to_nhwc4*) timed one by one at the workload's shape
(batch 32, 256 x 306 views; HIP events around 50 calls, 7 repeats), called directly through the C ABI.

    python tools/bench_gather.py                                   # this tree's library (or DD_HOTPATH_LIB): one JSON line
    python tools/bench_gather.py --alternate OTHER_LIB --rounds 6  # OTHER_LIB and this tree's in turn, a fresh process each: A/B of two builds
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

B, H, W, ITERS, REPEATS = 32, 256, 306, 50, 7


def measure():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from driving_dirty_amd import _lib
    from driving_dirty_amd.ops import _p, _stream as s
    dev, lib, g = torch.device("cuda:0"), _lib.lib(), torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (B, 6, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    views = torch.rand((B, 6, 3, H, W), generator=g).to(dev)
    v_s, f_s = [v.clone() for v in views], [f.clone() for f in frames]      # the collate's tuple: one allocation per sample
    tab_v, tab_f = ((C.c_void_p * B)(*[t.data_ptr() for t in ts]) for ts in (v_s, f_s))
    w32, wbf = torch.empty((B, H, 6 * W, 4), device=dev), torch.empty((B, H, 6 * W, 4), device=dev, dtype=torch.bfloat16)
    tgt, one = torch.empty((B, 3, H, W), device=dev), torch.empty((B, W, H, 4), device=dev)
    cases = {
        "dd_stitch6": lambda: lib.dd_stitch6(_p(views), _p(w32), None, None, B, H, W, -1, s()),
        "dd_stitch6[masked,target]": lambda: lib.dd_stitch6(_p(views), _p(w32), None, _p(tgt), B, H, W, 2, s()),
        "dd_stitch6_ptrs": lambda: lib.dd_stitch6_ptrs(tab_v, _p(w32), B, H, W, s()),
        "dd_stitch6_u8": lambda: lib.dd_stitch6_u8(_p(frames), _p(w32), B, H, W, s()),
        "dd_stitch6_u8_ptrs": lambda: lib.dd_stitch6_u8_ptrs(tab_f, _p(w32), None, B, H, W, -1, s()),
        "dd_stitch6_u8_ptrs[masked,target]": lambda: lib.dd_stitch6_u8_ptrs(tab_f, _p(w32), _p(tgt), B, H, W, 2, s()),
        "dd_stitch6_bf16": lambda: lib.dd_stitch6_bf16(_p(views), _p(wbf), B, H, W, s()),
        "dd_stitch6_bf16_ptrs": lambda: lib.dd_stitch6_bf16_ptrs(tab_v, _p(wbf), B, H, W, s()),
        "dd_stitch6_bf16_u8_ptrs": lambda: lib.dd_stitch6_bf16_u8_ptrs(tab_f, _p(wbf), B, H, W, s()),
        "dd_stitch6_bf16_masked": lambda: lib.dd_stitch6_bf16_masked(_p(views), _p(wbf), _p(tgt), B, H, W, 2, s()),
        "dd_stitch6_bf16_ptrs_masked": lambda: lib.dd_stitch6_bf16_ptrs_masked(tab_v, _p(wbf), _p(tgt), B, H, W, 2, s()),
        "dd_stitch6_bf16_u8_ptrs_masked": lambda: lib.dd_stitch6_bf16_u8_ptrs_masked(tab_f, _p(wbf), _p(tgt), B, H, W, 2, s()),
        "dd_view_to_nhwc4": lambda: lib.dd_view_to_nhwc4(_p(views), _p(one), B, H, W, 4, 1, s()),
        "dd_view_to_nhwc4_ptrs": lambda: lib.dd_view_to_nhwc4_ptrs(tab_v, _p(one), B, H, W, 4, 1, s()),
        "dd_view_to_nhwc4_u8_ptrs": lambda: lib.dd_view_to_nhwc4_u8_ptrs(tab_f, _p(one), B, H, W, 4, 1, s()),
    }
    out = {}
    for name, fn in cases.items():
        for _ in range(5):
            _lib.check(fn(), name)
        torch.cuda.synchronize()
        runs = []
        for _ in range(REPEATS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ITERS):
                fn()
            b.record()
            torch.cuda.synchronize()
            runs.append(a.elapsed_time(b) * 1e3 / ITERS)
        out[name] = round(statistics.median(runs), 3)
    return {"lib": os.environ.get("DD_HOTPATH_LIB", "tree"), "median_us_per_call": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternate", metavar="OTHER_LIB", help="another build of libdd_hotpath.so to run in turn with this tree's")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not a.alternate:
        print(json.dumps(measure()))
        return
    res = {"other": [], "tree": []}
    env = {k: v for k, v in os.environ.items() if k != "DD_HOTPATH_LIB"}
    for _ in range(a.rounds):
        for who, extra in (("other", {"DD_HOTPATH_LIB": os.path.abspath(a.alternate)}), ("tree", {})):
            out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(env, **extra), stdout=subprocess.PIPE, text=True, timeout=300,
                                 check=True).stdout      # a child that fails ends the whole run
            res[who].append(json.loads(out.strip().splitlines()[-1])["median_us_per_call"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
