"""GPU tests of ``optim.HipAdam(weight_decay=...)``: one tensor on the flat pass (70 001 elements, above ``SMALL_NUMEL``), three small
ones and an excluded one in the multi-tensor launch, and one small ``nn.Linear`` -- (136, 64 * 3 + 12), 7 and 32 batch rows -- registered
for the rank-B pass with ``min_numel`` lowered, as tests/test_gpu_round5.py does.

1. Every tensor after a step has the bits of the hand-made sequence ``p.mul_(keep)`` + the parent's entry point (``ops.adam_step_rankb``
   for the Linear, ``ops.adam_step_flat``, ``ops.adam_step_multi``) from the same state: the rank-B pre-scale and the fused kernels.
2. The same with clipping on, where the hand-made sequence hands the parent's ``_dev`` entry points the scale ``dd_clip_scale`` wrote.
3. Three steps of the flat and multi-tensor paths against ``torch.optim.AdamW`` in fp64 at the 1e-6 (of the tensor's peak) that
   tests/test_gpu_round5.py::test_adam_rankb_matches_fp64 uses for well-conditioned gradients; lr x weight_decay = 1e-4 per step, a
   hundred times that bound, so a step without the decay cannot pass."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, WD, EPS = 1e-3, 0.1, 1e-8
B1, B2 = 0.9, 0.999
KEEP = float(np.float32(1.0 - LR * WD))
IN, OUT = 64 * 3 + 12, 136


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import adamw
    adamw.lib()
    return torch.device("cuda:0")


class Net(torch.nn.Module):
    def __init__(self, seed=5):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *shape: torch.nn.Parameter(torch.rand(*shape, generator=g) - 0.5)
        self.big = rnd(70001)
        self.small_a, self.small_b, self.small_c = rnd(300), rnd(17, 5), rnd(1000)
        self.excluded = rnd(257)
        self.lin = torch.nn.Linear(IN, OUT)
        with torch.no_grad():
            self.lin.weight.copy_(torch.rand(OUT, IN, generator=g) - 0.5)
            self.lin.bias.copy_(torch.rand(OUT, generator=g) - 0.5)

    def plain(self):
        return {k: p for k, p in self.named_parameters() if not k.startswith("lin.")}


def make(dev, exclude_bias=False, clip=0.0):
    from driving_dirty_amd.optim import HipAdam
    net = Net().to(dev)
    opt = HipAdam(net.parameters(), lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    opt.exclude_from_decay([net.excluded] + ([net.lin.bias] if exclude_bias else []))
    assert [id(w) for w in opt.fuse_linear_wgrad(net.lin, min_numel=1024)] == [id(net.lin.weight)]
    if clip:
        opt.set_clip(clip)
    return net, opt


def inputs(net, step, rows, dev):
    """The step's gradients of the plain tensors and the Linear's factors (x, dy), seeded; positive factors: a well-conditioned dy^T x."""
    g = torch.Generator().manual_seed(1000 * step + rows)
    grads = {k: ((torch.rand(p.shape, generator=g) - 0.5) * 0.2).to(dev) for k, p in net.plain().items()}
    return grads, torch.rand(rows, IN, generator=g).to(dev), (torch.rand(rows, OUT, generator=g) * 0.1).to(dev)


def backward(net, grads, x, dy):
    from driving_dirty_amd import ops
    net.zero_grad(set_to_none=True)
    for k, p in net.plain().items():
        p.grad = grads[k].clone()
    (ops.linear(x, net.lin.weight, net.lin.bias) * dy).sum().backward()      # the output gradient is dy, bit for bit
    assert net.lin.weight.grad is None and net.lin.bias.grad is None, "the Linear took the rank-B pass"


def snapshot(net, opt):
    out = {}
    for k, p in net.named_parameters():
        st = opt.state.get(p)
        out[k] = (p.detach().clone(), st["exp_avg"].clone() if st else torch.zeros_like(p), st["exp_avg_sq"].clone() if st else torch.zeros_like(p))
    return out


def by_hand(net, opt, before, grads, x, dy, step, scale):
    """The hand-made sequence on copies of ``before``: a separate multiply by each tensor's keep, then the PARENT's entry points;
    ``scale`` a number or the device scalar of a clipped step (the ``_dev`` entry points) -> {name: (p, m, v)}."""
    from driving_dirty_amd import ops
    group = opt.param_groups[0]
    keeps = {k: opt._keep(p, group) for k, p in net.named_parameters()}
    out = {k: tuple(t.clone() for t in v) for k, v in before.items()}
    for k, (p, _, _) in out.items():
        p.mul_(keeps[k])
    (w, wm, wv), (b, bm, bv) = out["lin.weight"], out["lin.bias"]
    ops.adam_step_rankb(w, wm, wv, dy, x, b, bm, bv, LR, B1, B2, EPS, step, scale)
    p, m, v = out["big"]
    ops.adam_step_flat(p, grads["big"], m, v, LR, B1, B2, EPS, step, scale)
    small = [k for k in net.plain() if k != "big"]
    ops.adam_step_multi([(out[k][0].view(-1), grads[k].view(-1), out[k][1].view(-1), out[k][2].view(-1)) for k in small], LR, B1, B2, EPS,
                        step, scale)
    return out, keeps


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("clip", [0.0, 0.05], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("exclude_bias", [False, True])
@pytest.mark.parametrize("rows", [7, 32])
def test_a_step_is_the_multiply_followed_by_the_parents_entry_points(dev, rows, exclude_bias, clip):
    net, opt = make(dev, exclude_bias, clip)
    try:
        for step in (1, 2):      # zero moments, then moments that have seen a gradient
            grads, x, dy = inputs(net, step, rows, dev)
            before = snapshot(net, opt)
            backward(net, grads, x, dy)
            opt.step()
            torch.cuda.synchronize()
            if clip:
                assert 0.0 < float(opt.clip_coef) < 1.0, "the step is clipped"
                scale = opt._out3[0:1]      # grad_scale x coef on the device: what every update of the step read
            else:
                scale = 1.0
            want, keeps = by_hand(net, opt, before, grads, x, dy, step, scale)
            assert keeps["lin.weight"] == keeps["big"] == keeps["small_b"] == KEEP and keeps["excluded"] == 1.0
            assert keeps["lin.bias"] == (1.0 if exclude_bias else KEEP)
            for k, p in net.named_parameters():
                st = opt.state[p]
                assert st["step"] == step
                for name, got, ref in zip("pmv", (p.detach(), st["exp_avg"], st["exp_avg_sq"]), want[k]):
                    assert same_bits(got, ref), (step, k, name)
                assert not same_bits(p.detach(), before[k][0])
    finally:
        opt.close()


def test_three_steps_against_adamw_in_fp64(dev):
    net, opt = make(dev)
    names = list(net.plain())
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))      # the kernels take the betas as fp32 (tests/test_gpu_round5.py)
    twins = {k: torch.nn.Parameter(p.detach().double().cpu()) for k, p in net.plain().items()}
    ref = torch.optim.AdamW([{"params": [twins[k] for k in names if k != "excluded"], "weight_decay": WD},
                             {"params": [twins["excluded"]], "weight_decay": 0.0}], lr=float(np.float32(LR)), betas=(b1, b2),
                            eps=float(np.float32(EPS)))
    start = {k: p.detach().clone() for k, p in net.plain().items()}
    try:
        for step in (1, 2, 3):
            grads, x, dy = inputs(net, step, 7, dev)
            backward(net, grads, x, dy)
            opt.step()
            for k in names:
                twins[k].grad = grads[k].double().cpu()
            ref.step()
        torch.cuda.synchronize()
        rel = lambda a, r: float((a.double().cpu() - r).abs().max() / r.abs().max().clamp_min(1e-30))
        for k in names:
            st, rst = opt.state[net.plain()[k]], ref.state[twins[k]]
            errs = rel(net.plain()[k].detach(), twins[k].detach()), rel(st["exp_avg"], rst["exp_avg"]), rel(st["exp_avg_sq"], rst["exp_avg_sq"])
            print(f"{k}: p {errs[0]:.3g}, m {errs[1]:.3g}, v {errs[2]:.3g}")
            assert errs[0] < 1e-6 and errs[1] < 2e-6 and errs[2] < 2e-6, (k, errs)
        # the bound can tell: without the decay a decayed tensor ends 3 x 1e-4 of itself away
        moved = rel(start["big"] * (1.0 - LR * WD) ** 3, start["big"].double().cpu())
        assert moved > 100 * 1e-6
    finally:
        opt.close()
