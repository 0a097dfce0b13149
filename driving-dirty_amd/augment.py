"""Train-time augmentation on the device: the left/right mirror of the six-camera rig, exposure jitter, view drop.

Two parts.  The BINDER of ``csrc/libdd_augment.so`` (``include/dd_augment.h``): an extension library of its own, because the set of
functions of ``include/dd_hotpath.h`` is pinned.  It is a ``_lib.Extension``, whose parts are this module's ``lib`` / ``launch`` /
``last_error``: the ctypes table comes from the header through ``_lib.parse_header`` -- the one parser -- and
``launch(name, *operands)`` enters a function the way ``_lib.call`` does: looked up on the ``CDLL`` at every call, operands in header
order, the current torch stream appended, ``HotpathError`` with the library's message on a non-zero return.

The ``Augmenter``: what a model's ``training_step`` calls first.  Off by default: with every probability and width at 0 ``apply``
returns the batch object it was given and nothing is launched.

The mirror is the one label-preserving geometric transform of a six-camera rig with a top-down target: the ego car reflected about
its own axis.  Front-left swaps with front-right and back-left with back-right (views ``[2,1,0,5,4,3]``), every frame is reversed
left to right, the road map's rows are reversed (the bird's-eye frame has x forward along the columns and y to the left along the
rows) and a box has its y negated and its left and right corners swapped.
"""
import ctypes as C

import torch

from . import _lib, ops
from . import build as _build
from ._lib import HotpathError
from .lightning import hparam

# ---- the binder ------------------------------------------------------------------------------------------------------------------
_EXT = _lib.Extension(_build.EXTENSIONS["augment"])      # the one binder of an extension library (_lib.py)
LIB, SIGNATURES, STREAMED, OPERANDS = _EXT.library, _EXT.signatures, _EXT.streamed, _EXT.operands
lib, launch, last_error = _EXT.lib, _EXT.launch, _EXT.last_error      # module-level names: the functions below reach ``launch`` through the module's globals at call time
CHUNK = 32      # samples per kernel launch: kChunk of csrc/augment.hip (pointers, flags and colours travel in the kernel arguments)
FLAG_MIRROR = 1


def flag_blank(view):
    """The flag bit that blanks OUTPUT view ``view``."""
    return 1 << (8 + int(view))


MIRROR_VIEWS = (2, 1, 0, 5, 4, 3)      # output view v of a mirrored sample is input view MIRROR_VIEWS[v], reversed left to right


# ---- the three kernels as functions of tensors -------------------------------------------------------------------------------------
def _host_arrays(flags, color, b):
    flags = torch.as_tensor(flags).to("cpu", torch.int64).reshape(-1)
    if flags.numel() != b:
        raise ValueError(f"augment: {flags.numel()} flags for a batch of {b}")
    cflags = (C.c_uint32 * b)(*[int(f) for f in flags])
    if color is None:
        return cflags, None
    color = torch.as_tensor(color).to("cpu", torch.float32).contiguous()
    if tuple(color.shape) != (b, 6, 2):
        raise ValueError(f"augment: color must be [{b},6,2] (gain, bias per output view), got {tuple(color.shape)}")
    return cflags, (C.c_float * (b * 12)).from_buffer_copy(color.numpy().tobytes())


def _items(x):
    return [x[i] for i in range(x.shape[0])] if isinstance(x, torch.Tensor) else list(x)


def augment_views(sample, flags, color):
    """fp32 views ([B,6,3,H,W] or a tuple of [6,3,H,W]) or uint8 frames ([B,6,H,W,3] or a tuple of [6,H,W,3]) on the GPU -> ONE
    stacked fp32 [B,6,3,H,W]: mirrored, jittered and blanked per sample as ``flags`` [B] and ``color`` [B,6,2] say (dd_augment.h)."""
    table, b, h, w, dev, u8, _keep = ops.sample_table(sample, "augment_views")
    cflags, ccolor = _host_arrays(flags, color, b)
    out = torch.empty((b, 6, 3, h, w), device=dev, dtype=torch.float32)
    launch("dd_aug_views_u8_ptrs" if u8 else "dd_aug_views_ptrs", table, cflags, ccolor, out, b, h, w)
    return out


def augment_masks(road_image, flags):
    """Road masks (bool or uint8; [B,h,w] or a tuple of [h,w]) on the GPU -> a tuple of B contiguous views of ONE stacked [B,h,w]
    tensor of the same dtype, the masks of the mirrored samples with their rows reversed."""
    keep = [t if t.is_contiguous() else t.contiguous() for t in _items(road_image)]
    if not keep:
        raise HotpathError("augment_masks: empty batch")
    dtype, shape = keep[0].dtype, tuple(keep[0].shape)
    if dtype not in (torch.bool, torch.uint8) or len(shape) != 2:
        raise HotpathError(f"augment_masks: expected bool / uint8 road masks of [h,w] per sample, got {dtype} {shape}")
    for t in keep:
        if not (t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape):
            raise HotpathError(f"augment_masks: expected {dtype} {shape} masks on the GPU, got {t.dtype} {tuple(t.shape)} on {t.device}")
    b = len(keep)
    cflags, _ = _host_arrays(flags, None, b)
    out = torch.empty((b,) + shape, device=keep[0].device, dtype=torch.uint8)
    launch("dd_aug_masks_u8_ptrs", (C.c_void_p * b)(*[t.data_ptr() for t in keep]), cflags, out, b, shape[0], shape[1])
    return tuple(out.view(dtype).unbind(0))


def mirror_boxes(boxes):
    """[N,2,4] corners (rows x then y; columns front-left, front-right, back-left, back-right) of the mirrored scene: y negated,
    left and right corners swapped.  On the tensor where it lives, dtype kept; applied twice it is the identity bit for bit."""
    if boxes.dim() != 3 or tuple(boxes.shape[1:]) != (2, 4):
        raise ValueError(f"mirror_boxes: expected [N,2,4] boxes, got {tuple(boxes.shape)}")
    out = boxes.clone()
    out[:, 1, :] = -boxes[:, 1, :]
    return out[:, :, [1, 0, 3, 2]]


def current_rank():
    """This process's rank under torch.distributed, else 0: it goes into the augmenter's seed, so that the ranks draw differently."""
    dist = torch.distributed
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


# ---- the augmenter ----------------------------------------------------------------------------------------------------------------
def _is_triple(batch):
    """(sample, target, road_image) as the road-map and box models take it -- not the autoencoder's bare tuple of three views."""
    return (isinstance(batch, (tuple, list)) and len(batch) == 3
            and not all(isinstance(t, torch.Tensor) and t.dim() == 4 for t in batch))


class Augmenter:
    """``hparams``: ``aug_mirror`` (probability of the mirror, per sample), ``aug_brightness`` / ``aug_contrast`` (per sample) and
    ``aug_per_view`` (per sample and view): half-widths D of factors drawn from U[1-D, 1+D]; ``aug_view_drop``: probability that ONE
    uniformly chosen view of a sample is blanked; ``aug_seed``.  All default to 0.  With brightness f_b, contrast f_c and the
    per-view factor f_v a view's value becomes clamp(v * (f_b f_c f_v) + 0.5 (1 - f_c), 0, 1): contrast about mid-grey.

    The draws come from a generator of the augmenter's own, seeded from (aug_seed, rank): torch's and numpy's global states, which
    dropout, initialisation and BasicAE's masked slot draw from, are never touched."""

    def __init__(self, hparams=None, rank=0):
        self.mirror = float(hparam(hparams, "aug_mirror", 0.0) or 0.0)
        self.brightness = float(hparam(hparams, "aug_brightness", 0.0) or 0.0)
        self.contrast = float(hparam(hparams, "aug_contrast", 0.0) or 0.0)
        self.per_view = float(hparam(hparams, "aug_per_view", 0.0) or 0.0)
        self.view_drop = float(hparam(hparams, "aug_view_drop", 0.0) or 0.0)
        self.seed, self.rank = int(hparam(hparams, "aug_seed", 0) or 0), int(rank)
        for name in ("mirror", "view_drop"):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError(f"aug_{name} is a probability: {getattr(self, name)} is outside [0, 1]")
        for name in ("brightness", "contrast", "per_view"):
            if not 0.0 <= getattr(self, name) < 1.0:
                raise ValueError(f"aug_{name} is the half-width D of U[1-D, 1+D]: {getattr(self, name)} is outside [0, 1)")
        if self.seed < 0 or self.rank < 0:
            raise ValueError(f"aug_seed and the rank are non-negative: {self.seed}, {self.rank}")
        self.enabled = any(v > 0.0 for v in (self.mirror, self.brightness, self.contrast, self.per_view, self.view_drop))
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed((self.seed * 0x9E3779B1 + self.rank * 0x85EBCA6B + 1) % (1 << 63))

    def _factor(self, shape, half_width):
        u = torch.rand(shape, generator=self._gen, dtype=torch.float32)      # drawn whatever the width: one stream per (seed, rank)
        return 1.0 + half_width * (2.0 * u - 1.0)                            # exactly 1 at half_width 0

    def draw(self, batch_size):
        """-> (flags int64 [B], color fp32 [B,6,2]) on the CPU, as dd_augment.h reads them."""
        b = int(batch_size)
        mirror = torch.rand(b, generator=self._gen) < self.mirror
        f_b, f_c = self._factor((b,), self.brightness), self._factor((b,), self.contrast)
        f_v = self._factor((b, 6), self.per_view)
        drop = torch.rand(b, generator=self._gen) < self.view_drop
        view = torch.randint(0, 6, (b,), generator=self._gen)
        flags = mirror.to(torch.int64) * FLAG_MIRROR + drop.to(torch.int64) * torch.bitwise_left_shift(torch.ones_like(view), 8 + view)
        gain = (f_b * f_c).unsqueeze(1) * f_v
        bias = (0.5 * (1.0 - f_c)).unsqueeze(1).expand(b, 6)
        return flags, torch.stack([gain, bias], dim=2).contiguous()

    def apply(self, batch, draw=None):
        """A training batch -> the augmented batch.  ``(sample, target, road_image)``: ``sample`` (stacked or the collate's tuple, fp32
        views or uint8 frames) becomes one stacked fp32 [B,6,3,H,W]; ``road_image`` a tuple of per-sample views of the stacked,
        mirrored masks (dtype kept: the pointer-table kernels still serve them); each ``target['bounding_box']`` of a mirrored sample
        is mirrored where it lives, other keys pass through; a mirrored sample with a pre-rasterised ``'bb_map'`` raises ValueError
        (only coordinates mirror exactly).  A bare tensor or tuple of views (the autoencoder's batch) is augmented alone.
        ``draw``: (flags, color) instead of ``self.draw(B)``.  Not enabled: the batch object itself, nothing launched."""
        if not self.enabled:
            return batch
        triple = _is_triple(batch)
        sample = batch[0] if triple else batch
        b = sample.shape[0] if isinstance(sample, torch.Tensor) else len(sample)
        flags, color = self.draw(b) if draw is None else draw
        flags = torch.as_tensor(flags).to("cpu", torch.int64).reshape(-1)
        mirrored = [bool(f & FLAG_MIRROR) for f in flags.tolist()]
        if not triple:
            return augment_views(sample, flags, color)
        _, target, road_image = batch
        if target is not None:
            if len(target) != b:
                raise ValueError(f"augment: {len(target)} targets for a batch of {b}")
            for t, m in zip(target, mirrored):
                if m and "bb_map" in t:
                    raise ValueError("augment: a mirrored sample carries a pre-rasterised 'bb_map'; only box coordinates mirror exactly -- "
                                     "hand over 'bounding_box' and let the rasteriser draw the mirrored boxes")
            target = tuple({**t, "bounding_box": mirror_boxes(t["bounding_box"])} if m and "bounding_box" in t else t
                           for t, m in zip(target, mirrored))
        views = augment_views(sample, flags, color)
        if road_image is not None:
            road_image = augment_masks(road_image, flags)
        return views, target, road_image


def add_augment_args(p):
    """The augmentation's flags, for the ``add_model_specific_args`` of the models that train on the cameras."""
    p.add_argument("--aug_mirror", type=float, default=0.0, help="probability of the left/right mirror of the rig, per training sample")
    p.add_argument("--aug_brightness", type=float, default=0.0, help="brightness factor per sample from U[1-D, 1+D]: the half-width D")
    p.add_argument("--aug_contrast", type=float, default=0.0, help="contrast factor (about mid-grey) per sample from U[1-D, 1+D]: D")
    p.add_argument("--aug_per_view", type=float, default=0.0, help="exposure factor per sample and camera from U[1-D, 1+D]: D")
    p.add_argument("--aug_view_drop", type=float, default=0.0, help="probability that one uniformly chosen camera of a sample is blanked")
    p.add_argument("--aug_seed", type=int, default=0, help="seed of the augmentation's own generator (the rank is mixed in)")
    return p
