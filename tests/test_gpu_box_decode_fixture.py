"""The box decode (ops.component_boxes, ops.labelled_boxes, the workspace sizes of the four fit entry points of csrc/boxeval.hip) against
tests/golden/box_decode_parent.npz, which tools/record_box_decode.py wrote on the device before the four entry points were folded into one
pipeline.  The kernels use integer atomics only: their outputs do not depend on scheduling, so the recorded bytes are an oracle and
everything is compared with torch.equal.  The inputs are rebuilt from the seeds; the case list is a copy of the tool's."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (name, shape, density, seed): the smallest shapes that reach each loop and boundary of the fit kernels
INPUTS = (("wave", (1, 5, 7), 0.6, 11),             # one partial wave, one tile
          ("tiles", (2, 70, 100), 0.55, 12),        # tile borders, a 64-lane segment boundary, batch > 1
          ("wide", (1, 40, 300), 0.5, 13),          # a row longer than 256: two rounds of the in-row scan, five segments
          ("tall", (1, 260, 33), 0.5, 14))          # more than 256 rows: the second round of the row scan
LIMITS = ((1, 2048), (3, 8))                        # (min_pixels, max_boxes): the second one hits the cap
PADS = (0.5, 0.25)
SOURCES = ("components", "split_labels", "component_labels")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_decode_parent.npz")) as f:
        return {k: torch.from_numpy(f[k]) for k in f.files}


def decode(source, maps, min_pixels, cap, **kw):
    from driving_dirty_amd import ops
    if source == "components":
        return ops.component_boxes(maps, 0.5, min_pixels, cap, **kw)
    labels = ops.split_components(maps, 0.5, 2, 4) if source == "split_labels" else ops.label_components(maps)
    return ops.labelled_boxes(labels, min_pixels, cap, **kw)


def assert_stored(golden, key, got, counts, cap):
    """The first min(count, cap) rows of every sample are the recorded ones, sample after sample, and the rows after them are zero."""
    got, first = got.cpu(), 0
    for i, c in enumerate(counts.tolist()):
        n = min(c, cap)
        assert torch.equal(got[i, :n], golden[key][first:first + n]), (key, i)
        assert not got[i, n:].any(), (key, i)
        first += n
    assert first == golden[key].shape[0], key


@pytest.mark.parametrize("name,shape,density,seed", INPUTS, ids=[i[0] for i in INPUTS])
def test_decode_returns_the_recorded_bytes(dev, golden, name, shape, density, seed):
    from driving_dirty_amd import _lib
    lib = _lib.lib()
    mask = np.random.default_rng(seed).random(shape) < density
    maps = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(dev)
    checked = 0
    for min_pixels, cap in LIMITS:
        sizes = [lib.dd_component_boxes_workspace_bytes(*shape), lib.dd_component_obb_workspace_bytes(*shape, cap),
                 lib.dd_labelled_boxes_workspace_bytes(*shape), lib.dd_labelled_obb_workspace_bytes(*shape, cap)]
        assert sizes == golden[f"{name}/workspace/{cap}"].tolist()
        for source in SOURCES:
            key = f"{name}/{source}/extent/{min_pixels}_{cap}"
            boxes, counts = decode(source, maps, min_pixels, cap)
            assert counts.dtype == torch.int32 and torch.equal(counts.cpu(), golden[key + "/counts"]), key
            assert_stored(golden, key + "/boxes", boxes, counts, cap)
            for pad in PADS:
                key = f"{name}/{source}/oriented/{min_pixels}_{cap}/{pad}"
                boxes, counts, moments = decode(source, maps, min_pixels, cap, fit="oriented", pad_px=pad, want_moments=True)
                assert torch.equal(counts.cpu(), golden[key + "/counts"]), key
                assert_stored(golden, key + "/boxes", boxes, counts, cap)
                assert_stored(golden, key + "/moments", moments, counts, cap)
                checked += 3
            checked += 2
    assert checked == len([k for k in golden if k.startswith(name + "/") and "/workspace/" not in k])      # nothing recorded goes unchecked
    if name == "tiles":
        assert int(golden[f"{name}/components/extent/3_8/counts"].min()) > 8                               # the cap is hit
