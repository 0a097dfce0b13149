"""The reference of the augmentation tests: plain torch indexing on the CPU, written from the formulas of include/dd_augment.h
and not from the kernels.

    flags[b]  bit 0: mirror; bit 8 + v: blank OUTPUT view v
    mirror    out[b,v,c,y,x] = in[b,M[v],c,y,W-1-x], M = [2,1,0,5,4,3]; the road mask's rows reversed; a box's y negated and its
              left and right corners swapped
    colour    (gain, bias) per output view: (1, 0) moves the value bit for bit, else clamp(v * gain + bias, 0, 1) in fp32, two roundings
    uint8     the value is byte / 255 (a true division)
"""
import torch

M = [2, 1, 0, 5, 4, 3]
MIRROR, BLANK0 = 1, 1 << 8


def _stacked_cpu(x):
    return torch.stack([t.detach().cpu() for t in x], dim=0) if isinstance(x, (tuple, list)) else x.detach().cpu()


def views(sample, flags, color):
    """fp32 [B,6,3,H,W] / tuple of [6,3,H,W], or uint8 [B,6,H,W,3] / tuple of [6,H,W,3] (any device) -> fp32 [B,6,3,H,W] on the CPU."""
    x = _stacked_cpu(sample)
    if x.dtype == torch.uint8:
        x = x.permute(0, 1, 4, 2, 3).to(torch.float32).div(255)
    assert x.dtype == torch.float32 and x.dim() == 5 and tuple(x.shape[1:3]) == (6, 3), x.shape
    color = torch.as_tensor(color, dtype=torch.float32)
    out = torch.empty_like(x)
    for b in range(x.shape[0]):
        f = int(flags[b])
        src = x[b][M].flip(-1) if f & MIRROR else x[b]
        for v in range(6):
            gain, bias = color[b, v, 0], color[b, v, 1]
            if f & (BLANK0 << v):
                out[b, v] = 0.0
            elif float(gain) == 1.0 and float(bias) == 0.0:
                out[b, v] = src[v]
            else:
                out[b, v] = src[v].mul(gain).add(bias).clamp(0, 1)
    return out


def masks(road_image, flags):
    """bool / uint8 [B,h,w] or a tuple of [h,w] -> [B,h,w] on the CPU, dtype kept: row r <-> h-1-r where mirrored."""
    x = _stacked_cpu(road_image).clone()
    for b in range(x.shape[0]):
        if int(flags[b]) & MIRROR:
            x[b] = x[b].flip(0)
    return x


def boxes(bb):
    """[N,2,4] (rows x, y; columns front-left, front-right, back-left, back-right) -> the mirrored scene's boxes, dtype kept."""
    return torch.stack([bb[:, 0, :], -bb[:, 1, :]], dim=1).index_select(2, torch.tensor([1, 0, 3, 2], device=bb.device))


def targets(target, flags):
    """The tuple of target dicts with the boxes of the mirrored samples mirrored."""
    return tuple({**t, "bounding_box": boxes(t["bounding_box"])} if int(f) & MIRROR else t for t, f in zip(target, flags))
