"""The calls that cross the C ABI during a few tiny training steps, against the list recorded before the Python side of the boundary
was rewritten (tests/golden/abi_call_trace.json, written by tools/record_abi_call_trace.py: the steps, the recorder and the format
live there).  Same symbols, same order, same scalars and descriptors, pointers where pointers were, NULL where NULL was: the same
launches reach the library.  Seven steps: the roadmap, autoencoder (bf16 and fp32) and box-head steps on their default kernels, the box
head with split products, BoxesMergingCNN alone, and the box-head step with every A/B switch of gconv / heads off (recorded before
gconv.Layer's weight addressing moved into one derivation)."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_call_trace.json")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_abi_call_trace", os.path.join(ROOT, "tools", "record_abi_call_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_training_steps_make_the_recorded_calls():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    with open(GOLDEN) as f:
        golden = json.load(f)
    originals = {name: getattr(_lib.lib(), name) for name in _lib.SIGNATURES}
    trace = _recorder().record(torch.device("cuda:0"))
    assert all(getattr(_lib.lib(), name) is fn for name, fn in originals.items()), "the recorder left a wrapper on the library"
    assert list(trace) == list(golden)
    for step, calls in golden.items():
        got = trace[step]
        print(f"{step}: {len(got)} calls, {len(calls)} recorded")
        for i, (a, b) in enumerate(zip(got, calls)):
            assert a == b, f"{step}: call {i} is {a}, recorded {b}"
        n = min(len(got), len(calls))
        assert len(got) == len(calls), f"{step}: {len(got)} calls, {len(calls)} recorded; the first one without a partner: {(got + calls[n:])[n]}"
        assert len(calls) > 50
