"""Record what the box decode returns (ops.component_boxes, ops.labelled_boxes, the four dd_*_workspace_bytes of the fits) on small seeded
masks, as the fixture of tests/test_gpu_box_decode_fixture.py.

    python tools/record_box_decode.py [--out tests/golden/box_decode_parent.npz]

The kernels use integer atomics only, so what they return is the same from launch to launch and from build to build of the same
algorithm: run this ONCE, on a GPU, at the commit whose bytes a refactor has to keep.  The test rebuilds the inputs from the seeds and
keeps its own copy of the case list below; the two must agree.

Stored per case `<input>/<source>/<fit>/<min_pixels>_<max_boxes>[/<pad_px>]`: `counts` (uncapped), and the first min(count, max_boxes) rows of
every sample's `boxes` (and `moments`, oriented fit), sample after sample.  Per `<input>/workspace/<max_boxes>`: the workspace bytes of
dd_component_boxes, dd_component_obb, dd_labelled_boxes, dd_labelled_obb."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from driving_dirty_amd import _lib, ops  # noqa: E402

# (name, shape, density, seed): the smallest shapes that reach each loop and boundary of the fit kernels
INPUTS = (("wave", (1, 5, 7), 0.6, 11),             # one partial wave, one tile
          ("tiles", (2, 70, 100), 0.55, 12),        # tile borders, a 64-lane segment boundary, batch > 1
          ("wide", (1, 40, 300), 0.5, 13),          # a row longer than 256: two rounds of the in-row scan, five segments
          ("tall", (1, 260, 33), 0.5, 14))          # more than 256 rows: the second round of the row scan
LIMITS = ((1, 2048), (3, 8))                        # (min_pixels, max_boxes): the second one hits the cap
PADS = (0.5, 0.25)
SOURCES = ("components", "split_labels", "component_labels")


def stored_rows(t, counts, cap):
    return np.concatenate([t[i, :min(int(c), cap)].cpu().numpy() for i, c in enumerate(counts)])


def decode(source, maps, min_pixels, cap, **kw):
    if source == "components":
        return ops.component_boxes(maps, 0.5, min_pixels, cap, **kw)
    labels = ops.split_components(maps, 0.5, 2, 4) if source == "split_labels" else ops.label_components(maps)
    return ops.labelled_boxes(labels, min_pixels, cap, **kw)


def record():
    lib, out = _lib.lib(), {}
    for name, shape, density, seed in INPUTS:
        mask = np.random.default_rng(seed).random(shape) < density
        maps = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to("cuda:0")
        for min_pixels, cap in LIMITS:
            out[f"{name}/workspace/{cap}"] = np.array([lib.dd_component_boxes_workspace_bytes(*shape), lib.dd_component_obb_workspace_bytes(*shape, cap),
                                                       lib.dd_labelled_boxes_workspace_bytes(*shape), lib.dd_labelled_obb_workspace_bytes(*shape, cap)],
                                                      dtype=np.int64)
            for source in SOURCES:
                key = f"{name}/{source}/extent/{min_pixels}_{cap}"
                boxes, counts = decode(source, maps, min_pixels, cap)
                out[key + "/counts"], out[key + "/boxes"] = counts.cpu().numpy(), stored_rows(boxes, counts, cap)
                for pad in PADS:
                    key = f"{name}/{source}/oriented/{min_pixels}_{cap}/{pad}"
                    boxes, counts, moments = decode(source, maps, min_pixels, cap, fit="oriented", pad_px=pad, want_moments=True)
                    out[key + "/counts"] = counts.cpu().numpy()
                    out[key + "/boxes"], out[key + "/moments"] = stored_rows(boxes, counts, cap), stored_rows(moments, counts, cap)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "box_decode_parent.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_box_decode: needs a GPU")
    out = record()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    rows = sum(v.shape[0] for k, v in out.items() if k.endswith("/boxes"))
    print(f"{len(out)} arrays, {rows} box rows, {os.path.getsize(args.out)} bytes -> {args.out}")


if __name__ == "__main__":
    main()
