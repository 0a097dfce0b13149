"""The order of the optimizer passes and the conv stack's kernels in one training step (``optim.HipAdam`` as an observer of the
encoder's backward, ``ops.BACKWARD_OBSERVERS``), and the step's bookkeeping (``HipAdam.reset_step``).

The order is pinned to tests/golden/backward_schedule_trace.json: the symbol names of the steady ``TrainStep`` call in four
arrangements, recorded by ``tools/record_abi_call_trace.py --schedule`` at the commit in which the order still lived in module
variables of ``ops`` that every optimizer wrote.  Model and batches: the tiny RoadMapBCE of tests/test_gpu_round5.py with
``big_numel=4096``, so that the head and the encoder's fc1 take rank-B passes."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_round5 import _tiny_batch  # noqa: E402

DGRAD, WGRAD = "dd_conv_wino2_dgrad_w1", "dd_conv_wino2_wgrad_partials"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("record_abi_call_trace", os.path.join(ROOT, "tools", "record_abi_call_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "backward_schedule_trace.json")) as f:
        return json.load(f)


def _seed():
    torch.manual_seed(0)
    np.random.seed(0)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _assert_same_training_state(ta, tb):
    """Parameters and Adam moments of two TrainSteps over twin models, bit for bit (buffers -- BatchNorm's running statistics -- are not
    compared)."""
    for (k, p), (_, q) in zip(ta.model.named_parameters(), tb.model.named_parameters()):
        assert _same(p.detach(), q.detach()), k
        sa, sb = ta.optimizer.state[p], tb.optimizer.state[q]
        assert sa["step"] == sb["step"], k
        assert _same(sa["exp_avg"], sb["exp_avg"]) and _same(sa["exp_avg_sq"], sb["exp_avg_sq"]), k


def test_every_arrangement_keeps_the_recorded_order(dev, tool, recorded):
    """Default (overlap, passes last), ``passes_last=False``, ``adam_overlap=False``, ``fuse_linear_wgrad=False``: the same Adam and
    conv entry points in the same order as recorded.  With the passes last c2's data gradient runs in front of its weight gradient,
    otherwise behind it."""
    from driving_dirty_amd import ops
    assert list(recorded) == list(tool.ARRANGEMENTS)
    got = tool.record_schedule(dev)
    assert not ops.BACKWARD_OBSERVERS and not ops.RANKB
    for name, calls in recorded.items():
        print(name, len(got[name]), "calls,", len(calls), "recorded")
        assert got[name] == calls, name
        assert len(calls) > 20 and any(c.startswith("dd_adam_") for c in calls)
    for name, dgrad_first in (("default", True), ("passes_first", False)):
        assert (recorded[name].index(DGRAD) < recorded[name].index(WGRAD)) == dgrad_first, name
    assert "dd_adam_step_rankb" in recorded["default"] and "dd_adam_step_rankb" not in recorded["materialised"]


def test_closing_one_optimizer_leaves_the_schedule_of_another_alone(dev, tool, recorded):
    """TrainStep A in the default arrangement; a second TrainStep B over another model is built and closed; A's next step makes the
    calls of the default arrangement in the recorded order (c2's data gradient still first), and leaves the parameters and moments of a
    twin of A that never had a neighbour."""
    from driving_dirty_amd import ops
    a, twin = tool.tiny_train_step(dev), None
    try:
        _seed()
        a(_tiny_batch(dev, 0, 0), 0)
        b = tool.tiny_train_step(dev)
        assert len(ops.BACKWARD_OBSERVERS) == 2
        b.close()
        assert ops.BACKWARD_OBSERVERS == [a.optimizer] and a.optimizer.c2_dgrad_first
        calls = tool.schedule_of(a, _tiny_batch(dev, 1, 0), 1)
        assert calls == recorded["default"]
        assert calls.index(DGRAD) < calls.index(WGRAD)
        twin = tool.tiny_train_step(dev)
        _seed()
        for step in range(2):
            twin(_tiny_batch(dev, step, 0), step)
        torch.cuda.synchronize()
        _assert_same_training_state(a, twin)
    finally:
        a.close()
        if twin is not None:
            twin.close()
    assert not ops.BACKWARD_OBSERVERS and not ops.RANKB


def test_reset_step_forgets_an_abandoned_backward(dev):
    """HipAdam alone, passes after the backward, one rank-B Linear(64, 4096): backward on one batch, ``reset_step()``, backward on
    another, ``step()`` -- parameters and moments of a twin that only saw the second batch, bit for bit.  (Without the reset the two
    backwards add up: test_rankb_two_backwards_before_the_step_add_up.)"""
    from driving_dirty_amd import ops
    from driving_dirty_amd.optim import HipAdam
    torch.manual_seed(5)
    lin_b, lin_c = torch.nn.Linear(64, 4096).to(dev), torch.nn.Linear(64, 4096).to(dev)
    lin_c.load_state_dict(lin_b.state_dict())
    ob, oc = HipAdam(lin_b.parameters(), lr=1e-2), HipAdam(lin_c.parameters(), lr=1e-2)
    assert len(ob.fuse_linear_wgrad(lin_b, min_numel=1024)) == 1 and len(oc.fuse_linear_wgrad(lin_c, min_numel=1024)) == 1
    xs = [torch.rand(8, 64, device=dev), torch.rand(5, 64, device=dev)]
    ops.linear(xs[0], lin_b.weight, lin_b.bias).square().sum().backward()
    ob.reset_step()
    ops.linear(xs[1], lin_b.weight, lin_b.bias).square().sum().backward()
    ob.step()
    ops.linear(xs[1], lin_c.weight, lin_c.bias).square().sum().backward()
    oc.step()
    assert lin_b.weight.grad is None and lin_c.weight.grad is None
    for p, q in zip(lin_b.parameters(), lin_c.parameters()):
        assert _same(p.detach(), q.detach())
        assert ob.state[p]["step"] == oc.state[q]["step"] == 1
        assert _same(ob.state[p]["exp_avg"], oc.state[q]["exp_avg"]) and _same(ob.state[p]["exp_avg_sq"], oc.state[q]["exp_avg_sq"])
    ob.close()
    oc.close()
    assert not ops.RANKB


def _abandon_a_step(ts, batch, batch_idx):
    """Forward and backward as ``TrainStep.__call__`` runs them, and no ``step()``: what an exception behind the backward leaves.  The
    device's random state is put back, so that the next step draws what it would have drawn."""
    dev = next(ts.model.parameters()).device
    state, np_state = torch.cuda.get_rng_state(dev), np.random.get_state()
    ts.model.zero_grad(set_to_none=True)
    ts.model.training_step(batch, batch_idx)["loss"].backward()
    torch.cuda.set_rng_state(state, dev)
    np.random.set_state(np_state)


def test_trainstep_after_an_abandoned_step_equals_one_that_was_not(dev, tool):
    """``TrainStep(adam_overlap=False)``: a forward and backward without ``step()``, then ``ts(batch, i)`` -- parameters and Adam moments
    of a twin that only ran ``ts(batch, i)``, bit for bit: the factors the abandoned backward left with the optimizer are not added to
    the step's own in the two rank-B layers."""
    from driving_dirty_amd import ops
    a, b = tool.tiny_train_step(dev, adam_overlap=False), tool.tiny_train_step(dev, adam_overlap=False)
    try:
        assert len(a.fused) == 2
        batch = _tiny_batch(dev, 0, 0)
        _abandon_a_step(a, _tiny_batch(dev, 1, 0), 0)
        _seed()
        la = a(batch, 0)["loss"]
        _seed()
        lb = b(batch, 0)["loss"]
        torch.cuda.synchronize()
        assert float(la.detach()) == float(lb.detach())
        _assert_same_training_state(a, b)
    finally:
        a.close()
        b.close()
    assert not ops.RANKB


def test_overlapped_trainstep_runs_after_an_abandoned_backward(dev, tool):
    """The default arrangement (passes beside the backward): the call after an abandoned backward does not take the layers' factors for
    a second backward of one step, and returns a finite loss."""
    from driving_dirty_amd import ops
    ts = tool.tiny_train_step(dev)
    try:
        assert ts.overlap and len(ts.fused) == 2
        _abandon_a_step(ts, _tiny_batch(dev, 0, 0), 0)
        loss = ts(_tiny_batch(dev, 1, 0), 1)["loss"]
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss.detach()))
        assert not any(vars(ts.optimizer._now).values())
    finally:
        ts.close()
    assert not ops.BACKWARD_OBSERVERS and not ops.RANKB
