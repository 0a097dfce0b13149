"""torch.autograd.Function shims over the C ABI (``include/dd_hotpath.h``).

The shims own every tensor (the kernels never allocate), pass raw device pointers plus the
current PyTorch HIP stream, and raise on any non-zero return code.  Activations between conv
layers are NHWC fp32 tensors ``[B,H,W,C]``; the module layer (components.py) presents them to
callers as NCHW-shaped channels_last views, which is what the reference returns logically.
"""
import ctypes as C
import os

import torch

from . import _lib
from . import ddp as _ddp
from ._lib import ConvDesc, call, check, size  # noqa: F401  (check, C: tools/ and tests reach them as ops.check, ops.C)

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_RELU_MASK = 0, 1, 2, 3
PACK_FWD, PACK_DGRAD_S1, PACK_DGRAD_S2 = 0, 1, 2

_stream, _p, _dev = _lib.stream, _lib.ptr, _lib.dev      # the operand helpers live in _lib; these names stay for tools/ and tests


def conv_out(n, stride):
    return (n + 2 - 3) // stride + 1


def conv_desc(batch, h, w, cin_real, stride, rows_per_task=0):
    return ConvDesc(batch, h, w, cin_real, 4 if cin_real == 3 else cin_real, 32, 3, stride, 1, rows_per_task)


# ------------------------------------------------------------------------------------------------ layout
def is_u8_frames(sample):
    """uint8 camera frames as a decoder emits them: a [B,6,H,W,3] tensor or the collate's tuple / list of B [6,H,W,3] tensors."""
    if isinstance(sample, torch.Tensor):
        return sample.dtype == torch.uint8 and sample.dim() == 5
    return isinstance(sample, (tuple, list)) and len(sample) > 0 and all(
        isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 4 for t in sample)


def sample_table(sample, who):
    """-> (ctypes table of per-sample device pointers, B, H, W, device, u8 flag, keepalive) for every form the data pipeline hands over:
    fp32 [B,6,3,H,W], the collate's tuple / list of fp32 [6,3,H,W], uint8 [B,6,H,W,3] frames or a tuple / list of uint8 [6,H,W,3].  A
    stacked tensor is a table of its B slices: one code path for both forms.  Validated on the HOST, before anything is launched (a
    faulting kernel can reset the GPU): an empty batch, and per sample its device, its dtype -- the first sample's, so a tuple that
    mixes the forms is refused -- and its shape.  The keepalive holds the tensors the table points into (contiguous copies included)."""
    stacked = isinstance(sample, torch.Tensor)
    if not (stacked and sample.dim() == 5 or isinstance(sample, (tuple, list))):
        raise _lib.HotpathError(f"{who}: expected a stacked 5-d tensor or a tuple / list of per-sample tensors, got {type(sample).__name__}")
    items = [sample[i] for i in range(sample.shape[0])] if stacked else list(sample)
    if not items:
        raise _lib.HotpathError(f"{who}: empty batch")
    first = items[0]
    if not (isinstance(first, torch.Tensor) and first.dim() == 4):
        raise _lib.HotpathError(f"{who}: expected fp32 [6,3,H,W] views or uint8 [6,H,W,3] frames per sample, got {tuple(getattr(first, 'shape', ()))}")
    u8 = first.dtype == torch.uint8
    h, w = first.shape[1:3] if u8 else first.shape[2:4]
    dtype, shape = (torch.uint8, (6, h, w, 3)) if u8 else (torch.float32, (6, 3, h, w))
    keep = []
    for t in items:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == first.device and t.dtype == dtype and tuple(t.shape) == shape):
            raise _lib.HotpathError(f"{who}: expected {'uint8' if u8 else 'fp32'} {list(shape)} samples on one GPU, got "
                                    f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')}")
        keep.append(t if t.is_contiguous() else t.contiguous())
    table = (C.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
    return table, len(keep), h, w, first.device, int(u8), keep


def u8_table(sample, who):
    """``sample_table`` for a caller that takes uint8 frames only -> (table, B, H, W, device, keepalive)."""
    table, b, h, w, dev, u8, keep = sample_table(sample, who)
    if not u8:
        raise _lib.HotpathError(f"{who}: expected uint8 frames of [6,H,W,3] per sample, got fp32 views")
    return table, b, h, w, dev, keep


def stacked_views(views, who):
    """The operand of the entry points that read a stacked batch: contiguous fp32 [B,6,3,H,W] on the GPU -> (B, H, W)."""
    if not (isinstance(views, torch.Tensor) and views.dim() == 5 and views.shape[0] > 0 and tuple(views.shape[1:3]) == (6, 3)):
        raise _lib.HotpathError(f"{who}: expected [B,6,3,H,W], got {tuple(getattr(views, 'shape', ()))}")
    _dev(views, "views")
    return views.shape[0], views.shape[3], views.shape[4]


# The wide-image entry points by (output precision, input form) -> (without, with a masked view).  Forms: "views" a stacked fp32
# [B,6,3,H,W]; "samples" the collate's tuple of fp32 [6,3,H,W], read through a pointer table (no stack copy); "frames" uint8, stacked or
# a tuple, always through the table.  fp32 has no entry that reads fp32 samples WITH a masked view: wide_image stacks them for dd_stitch6.
WIDE_ENTRIES = {("fp32", "views"): ("dd_stitch6", "dd_stitch6"),
                ("fp32", "samples"): ("dd_stitch6_ptrs", None),
                ("fp32", "frames"): ("dd_stitch6_u8_ptrs", "dd_stitch6_u8_ptrs"),
                ("bf16", "views"): ("dd_stitch6_bf16", "dd_stitch6_bf16_masked"),
                ("bf16", "samples"): ("dd_stitch6_bf16_ptrs", "dd_stitch6_bf16_ptrs_masked"),
                ("bf16", "frames"): ("dd_stitch6_bf16_u8_ptrs", "dd_stitch6_bf16_u8_ptrs_masked")}
_TAKES_MASK = frozenset(masked for _, masked in WIDE_ENTRIES.values() if masked)      # their operands: ..., target, B, H, W, mask_slot


def camera_source(sample, who):
    """-> (form of WIDE_ENTRIES, the entry point's first operand, B, H, W, device, keepalive) for any of the four input forms.  A stacked
    tensor or a sample that is not contiguous is COPIED (``.contiguous()``; the keepalive holds the copy), as ``wide_image`` has always
    done; through this function that now also holds for ``stitch6_samples``, ``stitch6_bf16_samples`` and ``gconv.view_to_nhwc4``,
    which used to refuse such input."""
    if isinstance(sample, torch.Tensor) and sample.dtype != torch.uint8:
        views = sample.contiguous()
        return ("views", views, *stacked_views(views, who), views.device, views)
    table, b, h, w, dev, u8, keep = sample_table(sample, who)
    return "frames" if u8 else "samples", table, b, h, w, dev, keep


def mask_arg(mask_slot, who):
    """``mask_slot`` as the int the ABI takes: -1 (no masked view) or a wide slot 0 .. 5, checked on the host."""
    if not -1 <= int(mask_slot) <= 5:
        raise _lib.HotpathError(f"{who}: mask_slot {mask_slot} outside [-1, 5]")
    return int(mask_slot)


def wide_call(entry, src, b, h, w, dev, mask_slot=-1, want_target=False, want_nhwc4=True, want_nchw=False):
    """The one body behind every wide-image shim: allocates what ``entry`` (a dd_stitch6* function) writes for ``src`` (a stacked
    tensor or a pointer table, already validated) and calls it.  -> (wide NHWC4 [B,H,6W,4] fp32 or bf16, wide NCHW [B,3,H,6W], target
    [B,3,H,W] fp32), None for what was not asked for."""
    slot = mask_arg(mask_slot, entry)
    masked, both = entry in _TAKES_MASK, entry == "dd_stitch6"      # dd_stitch6 alone has the NCHW output
    if (slot >= 0 or want_target) and not masked or want_nchw and not both:
        raise _lib.HotpathError(f"{entry}: has no {'NCHW output' if want_nchw and not both else 'masked view'}")
    wide4 = torch.empty((b, h, 6 * w, 4), device=dev, dtype=torch.bfloat16 if "bf16" in entry else torch.float32) if want_nhwc4 else None
    wide = torch.empty((b, 3, h, 6 * w), device=dev, dtype=torch.float32) if want_nchw else None
    tgt = torch.empty((b, 3, h, w), device=dev, dtype=torch.float32) if want_target else None
    call(entry, src, wide4, *((wide,) if both else ()), *((tgt,) if masked else ()), b, h, w, *((slot,) if masked else ()))
    return wide4, wide, tgt


def stitch6(views, mask_slot=-1, want_nhwc4=True, want_nchw=False, want_target=False):
    """[B,6,3,H,W] -> wide image (view order [0,1,2,5,4,3]); see dd_stitch6 in dd_hotpath.h."""
    return wide_call("dd_stitch6", views, *stacked_views(views, "stitch6"), views.device, mask_slot, want_target, want_nhwc4, want_nchw)


def stitch6_samples(samples):
    """Tuple of B per-sample [6,3,H,W] tensors (the reference's collate, helper.py:22-23) -> wide NHWC4, no stack copy."""
    return wide_image(tuple(samples))


def stitch6_u8(frames):
    """frames [B,6,H,W,3] uint8 -> wide NHWC4 fp32 in [0,1] (ToTensor's /255 fused with the 6-view gather), read as ONE stacked batch."""
    if not (isinstance(frames, torch.Tensor) and frames.dim() == 5 and frames.shape[0] > 0 and frames.shape[1] == 6 and frames.shape[4] == 3
            and frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()):
        raise _lib.HotpathError(f"stitch6_u8: expected contiguous uint8 [B,6,H,W,3] on the GPU, got {tuple(frames.shape)} {frames.dtype}")
    return wide_call("dd_stitch6_u8", frames, frames.shape[0], frames.shape[2], frames.shape[3], frames.device)[0]


def stitch6_u8_samples(sample, mask_slot=-1, want_target=False):
    """uint8 frames ([B,6,H,W,3] or a tuple of [6,H,W,3]) -> wide NHWC4 fp32 in [0,1] (ToTensor's /255, data_helper.py:63-68, fused
    with the 6-view gather), optionally with BasicAE's masked-view task (-> (wide4, target [B,3,H,W]))."""
    table, b, h, w, dev, _keep = u8_table(sample, "stitch6_u8_samples")
    wide4, _, tgt = wide_call("dd_stitch6_u8_ptrs", table, b, h, w, dev, mask_slot, want_target)
    return (wide4, tgt) if want_target else wide4


def wide_image(sample, precision="fp32", mask_slot=-1, want_target=False):
    """Whatever the data pipeline hands over -> the wide NHWC4 image the conv stack reads (view order [0,1,2,5,4,3],
    roadmap_bce_v2.py:53-64), fp32 or bf16, in ONE pass:
      * fp32 [B,6,3,H,W] (autoencoder.py:53-57) or the collate's tuple of B fp32 [6,3,H,W] tensors (helper.py:22-23);
      * uint8 [B,6,H,W,3] or a tuple of B uint8 [6,H,W,3] decoded frames: ToTensor's /255 (data_helper.py:63-68) fused in.
    ``mask_slot`` / ``want_target``: the masked-view task of BasicAE.six_to_one_task -> (wide4, target); the target is the fp32 view
    [B,3,H,W] in both precisions (bit for bit the same), the wide image fp32 or bf16."""
    if precision not in ("fp32", "bf16"):
        raise _lib.HotpathError(f"wide_image: precision {precision!r} is neither 'fp32' nor 'bf16'")
    slot = mask_arg(mask_slot, "wide_image")
    form, src, b, h, w, dev, keep = camera_source(sample, "wide_image")
    entry = WIDE_ENTRIES[precision, form][slot >= 0 or want_target]
    if entry is None:
        entry, src = "dd_stitch6", torch.stack(keep, dim=0)
    wide4, _, tgt = wide_call(entry, src, b, h, w, dev, slot, want_target)
    return (wide4, tgt) if want_target else wide4


def boxes_to_binary_map(box_sets, device=None):
    """List of per-sample [n,2,4] corner tensors (f64 as the dataset holds them, or f32) -> [B,800,800] fp32 0/1 maps:
    boxes_to_binary_map (bb_to_img.py:5-20) for the whole batch in one launch, bit-identical to the Pillow fill."""
    import ctypes
    b = len(box_sets)
    if b == 0:
        raise _lib.HotpathError("boxes_to_binary_map: empty batch")
    dtype = box_sets[0].dtype
    if dtype not in (torch.float64, torch.float32) or any(t.dtype != dtype for t in box_sets):
        raise _lib.HotpathError("boxes_to_binary_map: boxes must all be float64 or all float32")
    for t in box_sets:
        if t.dim() != 3 or tuple(t.shape[1:]) != (2, 4):
            raise _lib.HotpathError(f"boxes_to_binary_map: expected [n,2,4] boxes, got {tuple(t.shape)}")
    if device is None:
        device = next((t.device for t in box_sets if t.is_cuda), None)
    if device is None or torch.device(device).type != "cuda":
        raise _lib.HotpathError("boxes_to_binary_map: no GPU device given (the rasteriser has no CPU fallback)")
    counts = [int(t.shape[0]) for t in box_sets]
    offsets = (ctypes.c_int32 * (b + 1))(0, *[sum(counts[:i + 1]) for i in range(b)])
    flat = torch.cat([t.reshape(-1, 8) for t in box_sets], dim=0).to(device).contiguous()
    maps = torch.empty((b, 800, 800), device=device, dtype=torch.float32)
    call("dd_boxes_to_binary_map", flat if flat.numel() else None, 0 if dtype == torch.float64 else 1, offsets, maps, b)
    return maps


def threat_score(a, b, round_b=False):
    """compute_ts_road_map (helper.py:74-77) in one pass on the device."""
    _dev(a, "a")
    _dev(b, "b", a.shape)
    out = torch.empty((), device=a.device, dtype=torch.float32)
    ws = torch.empty(size("dd_threat_score_workspace_bytes"), device=a.device, dtype=torch.uint8)
    call("dd_threat_score", a, b, out, a.numel(), int(round_b), ws)
    return out


TS_BINS = 256            # default resolution of the threshold calibration: thresholds k / 256


def ts_histogram(prob, target, bins=TS_BINS, out=None):
    """Histogram of the probabilities split by the target (dd_ts_hist): int64 [2, bins + 1], slot ``ceil(p * bins)`` (NaN: 0), row 1 for a
    non-zero target.  Holds the data set's exact threat score at every threshold ``k / bins`` (``ts_curve``).  The counts are ADDED to
    ``out`` when one is given: the batches of a validation epoch accumulate in one buffer.  ``target``: fp32, uint8 or bool."""
    _dev(prob, "prob")
    if not (isinstance(target, torch.Tensor) and target.is_cuda and target.is_contiguous() and target.numel() == prob.numel()
            and target.dtype in (torch.float32, torch.uint8, torch.bool)):
        raise _lib.HotpathError(f"ts_histogram: target must be a contiguous fp32 / uint8 / bool device tensor of {prob.numel()} elements, got "
                                f"{getattr(target, 'dtype', type(target))} {tuple(getattr(target, 'shape', ()))}")
    if out is None:
        out = torch.zeros((2, bins + 1), device=prob.device, dtype=torch.int64)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (2, bins + 1)):
        raise _lib.HotpathError(f"ts_histogram: out must be a contiguous int64 device tensor [2, {bins + 1}]")
    kind = 0 if target.dtype == torch.float32 else 1      # DD_TARGET_F32 / DD_TARGET_U8
    call("dd_ts_hist", prob, target, kind, prob.numel(), int(bins), out)
    return out


def ts_curve(hist):
    """``ts_histogram``'s counts -> (ts float64 [bins], best_k): ts[k] = TP_k / (P_k + T - TP_k) for the prediction ``p > k / bins``,
    with T every positive target; a threshold whose denominator is 0 scores 0.  best_k: the maximum; ties go to the k nearest
    bins / 2 (the reference's round()), then to the lower k.  Plain torch on 2 x (bins + 1) integers."""
    if hist.dim() != 2 or hist.size(0) != 2 or hist.size(1) < 3:
        raise ValueError(f"ts_curve: expected counts [2, bins + 1], got {tuple(hist.shape)}")
    h = hist.detach().to("cpu", torch.int64)
    bins = h.size(1) - 1
    above = torch.flip(torch.cumsum(torch.flip(h[:, 1:], [1]), 1), [1])      # [row, k]: elements with slot > k
    tp, p, t = above[1], above[0] + above[1], h[1].sum()
    den = p + t - tp
    ts = torch.where(den > 0, tp.double() / den.clamp(min=1).double(), torch.zeros(bins, dtype=torch.float64))
    k = torch.arange(bins)
    ties = k[ts == ts.max()]
    best = ties[torch.argmin((ties - bins // 2).abs() * (bins + 1) + ties)]
    return ts, int(best)


# ------------------------------------------------------------------------------------------------ box-level validation
def _maps(maps, who):
    if not isinstance(maps, torch.Tensor) or maps.dim() != 3:
        raise _lib.HotpathError(f"{who}: expected fp32 maps [B,H,W], got {tuple(getattr(maps, 'shape', ()))}")
    _dev(maps, "maps")
    b, h, w = maps.shape
    if b == 0 or _lib.lib().dd_label_components_workspace_bytes(b, h, w) < 0:
        raise _lib.HotpathError(f"{who}: unsupported shape {tuple(maps.shape)}: {_lib.lib().dd_last_error().decode()}")
    return b, h, w


def label_components(maps, threshold=0.5):
    """fp32 maps [B,H,W] -> int32 labels [B,H,W] of the 4-connected components of ``maps > threshold``: 0 for background, else
    1 + the raster-order index (inside its sample) of the component's first pixel.  Canonical and deterministic."""
    b, h, w = _maps(maps, "label_components")
    labels = torch.empty((b, h, w), device=maps.device, dtype=torch.int32)
    call("dd_label_components", maps, float(threshold), labels, b, h, w)
    return labels


def _split_args(split_px, grow_iters, who):
    """(split_px, grow_iters) as ints, ``grow_iters=None`` meaning ``2 * split_px``; anything that is no whole number is refused."""
    for name, v in (("split_px", split_px), ("grow_iters", grow_iters)):
        if not (v is None and name == "grow_iters") and (isinstance(v, bool) or int(v) != v):
            raise ValueError(f"{who}: {name} must be a whole number, got {v!r}")
    split_px = int(split_px)
    return split_px, 2 * split_px if grow_iters is None else int(grow_iters)


def split_components(maps, threshold=0.5, split_px=4, grow_iters=None):
    """fp32 maps [B,H,W] -> int32 labels [B,H,W]: ``maps > threshold`` partitioned into regions by marker-based splitting, which takes
    apart blobs that are joined through a neck narrower than ``2 * split_px + 1`` pixels (two cars in contact).  Erode by ``split_px``,
    label the cores, grow them back inside the mask for ``grow_iters`` synchronous rounds (default ``2 * split_px``; the smallest
    neighbouring label wins), label what is left as components of its own (include/dd_hotpath.h states the rule).  A label minus 1 is
    some pixel of its region, not necessarily the first.  ``split_px`` in [1,8], ``grow_iters`` in [0,16].  Integer only: deterministic."""
    b, h, w = _maps(maps, "split_components")
    split_px, grow_iters = _split_args(split_px, grow_iters, "split_components")
    nbytes = size("dd_split_components_workspace_bytes", b, h, w, split_px, grow_iters)
    labels = torch.empty((b, h, w), device=maps.device, dtype=torch.int32)
    ws = torch.empty(nbytes, device=maps.device, dtype=torch.uint8)
    call("dd_split_components", maps, float(threshold), split_px, grow_iters, labels, b, h, w, ws, nbytes)
    return labels


def _fit_args(who, fit, want_moments):
    if fit not in ("extent", "oriented"):
        raise ValueError(f"{who}: fit must be 'extent' or 'oriented', got {fit!r}")
    if want_moments and fit != "oriented":
        raise ValueError(f"{who}: want_moments needs fit='oriented' (the extent fit forms no moments)")


def _fit(who, entries, src, lead, min_pixels, max_boxes, fit, pad_px, want_moments):
    """What ``component_boxes`` and ``labelled_boxes`` share: ``src`` [B,H,W] (maps or labels, already checked) through
    ``entries`` = the (extent, oriented) pair of C entry points, whose arguments begin with ``lead`` (the source, and the threshold)."""
    min_pixels, max_boxes = int(min_pixels), int(max_boxes)
    if min_pixels < 1 or max_boxes < 1:
        raise _lib.HotpathError(f"{who}: min_pixels and max_boxes must be positive")
    b, h, w = src.shape
    oriented = fit == "oriented"
    entry = entries[oriented]
    # not size(): the refusal keeps this function's own message (who, and the shape that was refused)
    nbytes = getattr(_lib.lib(), entry + "_workspace_bytes")(b, h, w, *((max_boxes,) if oriented else ()))
    if b == 0 or nbytes < 0:
        raise _lib.HotpathError(f"{who}: unsupported shape {tuple(src.shape)}: {_lib.lib().dd_last_error().decode()}")
    boxes = torch.zeros((b, max_boxes, 2, 4), device=src.device, dtype=torch.float32)
    counts = torch.empty((b,), device=src.device, dtype=torch.int32)
    moments = torch.zeros((b, max_boxes, 6), device=src.device, dtype=torch.int64) if want_moments else None
    ws = torch.empty(nbytes, device=src.device, dtype=torch.uint8)
    out = (float(pad_px), boxes, counts, moments) if oriented else (boxes, counts)
    call(entry, *lead, min_pixels, max_boxes, *out, b, h, w, ws, nbytes)
    return (boxes, counts, moments) if want_moments else (boxes, counts)


def labelled_boxes(labels, min_pixels=1, max_boxes=256, fit="extent", pad_px=0.5, want_moments=False):
    """``component_boxes`` for regions given as an int32 label image [B,H,W] (``split_components``' or ``label_components``' output: the
    pixels of one label L form a region, and pixel L - 1 carries L).  Same survivors, order, counts, formats and roundings."""
    _fit_args("labelled_boxes", fit, want_moments)
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or labels.dtype != torch.int32:
        raise _lib.HotpathError(f"labelled_boxes: expected int32 labels [B,H,W], got {getattr(labels, 'dtype', None)} "
                                f"{tuple(getattr(labels, 'shape', ()))}")
    if not labels.is_cuda or not labels.is_contiguous():
        raise _lib.HotpathError("labelled_boxes: labels must be a contiguous GPU tensor (there is no CPU fallback)")
    return _fit("labelled_boxes", ("dd_labelled_boxes", "dd_labelled_obb"), labels, (labels,), min_pixels, max_boxes, fit, pad_px, want_moments)


def component_boxes(maps, threshold=0.5, min_pixels=1, max_boxes=256, fit="extent", pad_px=0.5, want_moments=False, split_px=0, grow_iters=None):
    """fp32 maps [B,H,W] -> (boxes fp32 [B,max_boxes,2,4], counts int32 [B]): one box for each component of ``maps > threshold`` with
    at least ``min_pixels`` pixels, in the data set's box format (metres, ego at the centre: the inverse of
    ``boxes_to_binary_map``'s pixel mapping), ordered by component label.  ``counts`` is the UNCAPPED number of such components:
    ``counts[i] > max_boxes`` means sample i overflowed and only its first ``max_boxes`` boxes are present.  Unused rows are zero.

    ``fit="extent"``: the axis-aligned pixel extent.  ``fit="oriented"``: the rectangle along the component's principal axis (exact
    integer second moments -> heading -> extents of the pixel centres along and across it, moved outwards by ``pad_px`` pixels:
    0.5 = the support of the pixel squares, 0 = the hull of the centres; include/dd_hotpath.h states the fit).  Same components, same
    order, same counts; sides up to 1024.  A principal-axis fit, not a minimum-area rectangle (for a filled rectangle the two agree);
    which end of the box is its front is arbitrary.  ``want_moments`` (oriented only) also returns int64 [B,max_boxes,6]:
    N, Sx, Sy, Sxx, Sxy, Syy of each stored box.

    ``split_px > 0``: the boxes are fitted to the regions of ``split_components(maps, threshold, split_px, grow_iters)`` instead of to the
    components (touching cars joined through a neck come apart; ``grow_iters=None`` = ``2 * split_px``).  ``split_px = 0``, the default,
    launches nothing new and changes no output."""
    _fit_args("component_boxes", fit, want_moments)
    split_px, grow_iters = _split_args(split_px, grow_iters, "component_boxes")
    if split_px != 0:
        return labelled_boxes(split_components(maps, threshold, split_px, grow_iters), min_pixels, max_boxes, fit, pad_px, want_moments)
    _maps(maps, "component_boxes")
    return _fit("component_boxes", ("dd_component_boxes", "dd_component_obb"), maps, (maps, float(threshold)), min_pixels, max_boxes, fit, pad_px,
                want_moments)


def _box_list(box_sets, who, device):
    """Per-sample [n,2,4] tensors (all f64 or all f32) -> (flat device tensor [sum n, 8], dtype code, ctypes offsets)."""
    dtypes = {t.dtype for t in box_sets}
    if len(dtypes) != 1 or next(iter(dtypes)) not in (torch.float64, torch.float32):
        raise _lib.HotpathError(f"{who}: boxes must all be float64 or all float32")
    for t in box_sets:
        if t.dim() != 3 or tuple(t.shape[1:]) != (2, 4):
            raise _lib.HotpathError(f"{who}: expected [n,2,4] boxes, got {tuple(t.shape)}")
    counts = [int(t.shape[0]) for t in box_sets]
    offsets = (C.c_int32 * (len(box_sets) + 1))(0, *[sum(counts[:i + 1]) for i in range(len(box_sets))])
    flat = torch.cat([t.reshape(-1, 8) for t in box_sets], dim=0).to(device).contiguous()
    return flat, 0 if flat.dtype == torch.float64 else 1, offsets


def _iou_ats(box_sets1, box_sets2, want_iou, who):
    b = len(box_sets1)
    if b == 0 or len(box_sets2) != b:
        raise _lib.HotpathError(f"{who}: needs two lists of the same non-zero length, got {b} and {len(box_sets2)}")
    device = next((t.device for t in list(box_sets1) + list(box_sets2) if t.is_cuda), None)
    if device is None:
        raise _lib.HotpathError(f"{who}: no box tensor is on a GPU (there is no CPU fallback)")
    flat1, dt1, off1 = _box_list(box_sets1, who, device)
    flat2, dt2, off2 = _box_list(box_sets2, who, device)
    nbytes = size("dd_box_iou_ats_workspace_bytes", off1, off2, b)
    ats = torch.empty((b,), device=device, dtype=torch.float32)
    pairs = sum(int(s.shape[0]) * int(t.shape[0]) for s, t in zip(box_sets1, box_sets2))
    iou = torch.empty((max(pairs, 1),), device=device, dtype=torch.float32) if want_iou else None
    ws = None if want_iou else torch.empty(nbytes, device=device, dtype=torch.uint8)
    call("dd_box_iou_ats", flat1 if flat1.numel() else None, dt1, off1, flat2 if flat2.numel() else None, dt2, off2, iou, ats, b, ws,
         0 if want_iou else nbytes)
    return iou, ats


def box_iou(boxes1, boxes2):
    """[n1,2,4], [n2,2,4] corner tensors of one sample -> fp32 IoU matrix [n1,n2] (compute_iou, helper.py:79-83, for every pair).
    Each box must be a convex quadrilateral of positive area with outline 0,1,3,2 (either orientation), as the data set's are."""
    iou, _ = _iou_ats([boxes1], [boxes2], True, "box_iou")
    n1, n2 = int(boxes1.shape[0]), int(boxes2.shape[0])
    return iou[:n1 * n2].reshape(n1, n2)


def ats_bounding_boxes(box_sets1, box_sets2):
    """Two lists of B per-sample [n,2,4] corner tensors (like ``boxes_to_binary_map``'s) -> fp32 [B]: compute_ats_bounding_boxes
    (helper.py:33-72) of each sample, ``iou_max`` taken over set 1 for each box of set 2.  DEPARTS from the reference in one point:
    a sample where either set is empty scores 0 (the reference raises on an empty set)."""
    return _iou_ats(box_sets1, box_sets2, False, "ats_bounding_boxes")[1]


def nchw_to_nhwc(x, c_store):
    b, c, h, w = x.shape
    _dev(x, "x")
    out = torch.empty((b, h, w, c_store), device=x.device, dtype=torch.float32)
    call("dd_nchw_to_nhwc", x, out, b, c, h, w, c_store)
    return out


def subsample_nhwc4(x, stride, offset, oh, ow):
    """x [B,1,H,W] or [B,H,W] -> [B,oh,ow,4] with channel 0 = x[stride*u + offset, stride*v + offset] (zero outside)."""
    _dev(x, "x")
    b, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    assert x.numel() == b * h * w, "subsample_nhwc4: one channel"
    out = torch.empty((b, oh, ow, 4), device=x.device, dtype=torch.float32)
    call("dd_subsample_nhwc4", x.contiguous(), out, b, h, w, oh, ow, stride, offset)
    return out


def subsample_masks_nhwc4(masks, stride, offset, oh, ow):
    """Tuple / list of B per-sample bool / uint8 [H,W] masks (the collate's ``road_image`` tuple) -> [B,oh,ow,4] fp32 with
    channel 0 = float(mask[stride*u + offset, stride*v + offset]) (zero outside): ``subsample_nhwc4`` of
    ``torch.stack(masks).float()`` without the stack and the cast."""
    import ctypes
    b = len(masks)
    h, w = masks[0].shape[-2], masks[0].shape[-1]
    for t in masks:
        if not (t.is_cuda and t.is_contiguous() and t.dtype in (torch.bool, torch.uint8) and t.numel() == h * w):
            raise _lib.HotpathError("subsample_masks_nhwc4: expected contiguous bool / uint8 device masks of one size")
    out = torch.empty((b, oh, ow, 4), device=masks[0].device, dtype=torch.float32)
    table = (ctypes.c_void_p * b)(*[t.data_ptr() for t in masks])
    call("dd_subsample_nhwc4_u8_ptrs", table, out, b, h, w, oh, ow, stride, offset)
    return out


def deconv2x2_c32_fwd(x, wt, bias, relu=True):
    """x [B,h,w,32] NHWC, wt [32,32,2,2] -> (relu)(ConvTranspose2d k2 s2) [B,2h,2w,32] NHWC, one launch."""
    b, h, w, c = x.shape
    assert c == 32 and tuple(wt.shape) == (32, 32, 2, 2) and x.is_contiguous() and wt.is_contiguous()
    out = torch.empty((b, 2 * h, 2 * w, 32), device=x.device, dtype=torch.float32)
    call("dd_deconv2x2_c32_fwd", x, wt, bias, out, b, h, w, int(relu))
    return out


def deconv2x2_c32_fwd_into(x, wt, bias, out, coff, relu=True):
    """The same into channels [coff, coff+32) of ``out`` [B,2h,2w,C] NHWC (a concat buffer's slice)."""
    b, h, w, c = x.shape
    assert c == 32 and tuple(wt.shape) == (32, 32, 2, 2) and x.is_contiguous() and wt.is_contiguous()
    assert out.is_contiguous() and tuple(out.shape[:3]) == (b, 2 * h, 2 * w) and 0 <= coff and coff + 32 <= out.shape[3]
    call("dd_deconv2x2_c32_fwd_slice", x, wt, bias, out, b, h, w, int(relu), out.shape[3], coff)


def ssconv_dgrad_ok(g, dx):
    """ss_conv's data gradient in one launch serves these tensors: dense 32-channel NHWC, gw = (xw - 24) / 7 + 1 <= 128."""
    return (g.dim() == 4 and dx.dim() == 4 and g.shape[3] == 32 and dx.shape[3] == 32 and g.is_contiguous() and dx.is_contiguous()
            and g.shape[:2] == dx.shape[:2] and bool(_lib.lib().dd_ssconv_dgrad_supported(g.shape[1], g.shape[2], dx.shape[2])))


def ssconv_dgrad(g, wt, dx):
    """g [B,h,gw,32], wt [32,32,1,24] (Conv2d weight) -> dx [B,h,xw,32] = dL/d(input) of Conv2d(32,32,(1,24),stride (1,7))."""
    assert tuple(wt.shape) == (32, 32, 1, 24) and wt.is_contiguous() and ssconv_dgrad_ok(g, dx)
    b, h, gw, _ = g.shape
    call("dd_ssconv_dgrad", g, wt, dx, b, h, gw, dx.shape[2])


def ssconv_fwd(x, wt, bias, y, relu=True):
    """x [B,h,xw,32], wt [32,32,1,24], bias [32] or None -> y [B,h,gw,32] = (relu)(Conv2d(32,32,(1,24),stride (1,7))(x)), one launch."""
    assert tuple(wt.shape) == (32, 32, 1, 24) and wt.is_contiguous() and ssconv_dgrad_ok(y, x)
    b, h, xw, _ = x.shape
    call("dd_ssconv_fwd", x, wt, bias, y, b, h, xw, y.shape[2], int(relu))


def conv1x1_c32_c3_nchw(x, wt, bias):
    """x [B,h,w,32] NHWC, wt [32,3,1,1] -> ConvTranspose2d k1 [B,3,h,w] NCHW."""
    b, h, w, c = x.shape
    assert c == 32 and tuple(wt.shape) == (32, 3, 1, 1) and x.is_contiguous() and wt.is_contiguous()
    out = torch.empty((b, 3, h, w), device=x.device, dtype=torch.float32)
    call("dd_conv1x1_c32_c3_nchw", x, wt, bias, out, b, h, w)
    return out


def conv1ch_fwd(taps4, w, bias, relu=True):
    """taps4 [B,sh,sw,4] (channel 0), w [32,1,7,7] -> relu(conv + bias) [B,sh-6,sw-6,32] (NHWC)."""
    b, sh, sw, _ = taps4.shape
    assert tuple(w.shape) == (32, 1, 7, 7) and w.is_contiguous()
    y = torch.empty((b, sh - 6, sw - 6, 32), device=taps4.device, dtype=torch.float32)
    call("dd_conv1ch_fwd", taps4, w, bias, y, b, sh, sw, int(relu))
    return y


def conv1ch_wgrad(taps4, g):
    """-> (dw [32,1,7,7], db [32]) of conv1ch_fwd from g = dL/dy [B,sh-6,sw-6,32] (ReLU mask already applied)."""
    b, sh, sw, _ = taps4.shape
    assert tuple(g.shape) == (b, sh - 6, sw - 6, 32) and g.is_contiguous()
    dw = torch.empty((32, 1, 7, 7), device=g.device, dtype=torch.float32)
    db = torch.empty(32, device=g.device, dtype=torch.float32)
    ws = torch.empty(size("dd_conv1ch_wgrad_workspace_bytes"), device=g.device, dtype=torch.uint8)
    call("dd_conv1ch_wgrad", taps4, g, dw, db, b, sh, sw, ws)
    return dw, db


def conv1ch_fwd_phase3(taps4, w, bias, relu=True):
    """conv1ch_fwd with the output in the phase-major layout of a dilation-3 consumer: -> (y [9B, ph, pw, 32], its sign words int32
    [9B, ph, pw]), ph = ceil((sh-6) / 3), pw likewise; image b * 9 + (i % 3) * 3 + j % 3 holds the pixels (i, j) of that residue class."""
    b, sh, sw, _ = taps4.shape
    assert tuple(w.shape) == (32, 1, 7, 7) and w.is_contiguous()
    ph, pw = (sh - 6 + 2) // 3, (sw - 6 + 2) // 3
    y = torch.empty((9 * b, ph, pw, 32), device=taps4.device, dtype=torch.float32)
    bits = torch.empty((9 * b, ph, pw), device=taps4.device, dtype=torch.int32)
    call("dd_conv1ch_fwd_phase3", taps4, w, bias, y, bits, b, sh, sw, int(relu))
    return y, bits


def conv1ch_wgrad_phase3(taps4, g_phase):
    """conv1ch_wgrad from dL/dy in the phase-major layout [9B, ph, pw, 32]."""
    b, sh, sw, _ = taps4.shape
    ph, pw = (sh - 6 + 2) // 3, (sw - 6 + 2) // 3
    assert tuple(g_phase.shape) == (9 * b, ph, pw, 32) and g_phase.is_contiguous()
    dw = torch.empty((32, 1, 7, 7), device=g_phase.device, dtype=torch.float32)
    db = torch.empty(32, device=g_phase.device, dtype=torch.float32)
    ws = torch.empty(size("dd_conv1ch_wgrad_workspace_bytes"), device=g_phase.device, dtype=torch.uint8)
    call("dd_conv1ch_wgrad_phase3", taps4, g_phase, dw, db, b, sh, sw, ws)
    return dw, db


def phase3_scatter(src_phase, dst, coff, off):
    """dst [B,oh,ow,cs] channels [coff, +32) <- the phase images src_phase [9B, ph, pw, 32], read ``off`` cells in from their corner."""
    _dev(src_phase, "src_phase")
    _dev(dst, "dst")
    b, oh, ow, cs = dst.shape
    assert src_phase.shape[0] == 9 * b and src_phase.shape[3] == 32
    call("dd_phase3_scatter", src_phase, dst, b, oh, ow, src_phase.shape[1], src_phase.shape[2], off, cs, coff)


def phase3_gather(src, coff, ph, pw, off):
    """-> [9B, ph, pw, 32]: the 32-channel slice [coff, +32) of the dense NHWC buffer src in phase images, ``off`` cells in; zero elsewhere."""
    _dev(src, "src")
    b, oh, ow, cs = src.shape
    out = torch.empty((9 * b, ph, pw, 32), device=src.device, dtype=torch.float32)
    call("dd_phase3_gather", src, out, b, oh, ow, ph, pw, off, cs, coff)
    return out


def nhwc_to_nchw(x, c):
    b, h, w, cs = x.shape
    _dev(x, "x")
    out = torch.empty((b, c, h, w), device=x.device, dtype=torch.float32)
    call("dd_nhwc_to_nchw", x, out, b, c, h, w, cs)
    return out


class ToNHWC(torch.autograd.Function):
    """Differentiable NCHW -> NHWC(c_store) re-layout (API edges: callers may hand in ordinary NCHW tensors)."""

    @staticmethod
    def forward(ctx, x, c_store):
        ctx.c = x.shape[1]
        return nchw_to_nhwc(x.contiguous(), c_store)

    @staticmethod
    def backward(ctx, g):
        return nhwc_to_nchw(g.contiguous(), ctx.c), None


# ------------------------------------------------------------------------------------------------ conv primitives
def conv_pack(weight, desc, kind):
    _dev(weight, "weight", (32, desc.cin_real, 3, 3))
    n = size("dd_conv_packed_floats", desc, kind)
    packed = torch.empty(n, device=weight.device, dtype=torch.float32)
    call("dd_conv_pack", weight, packed, desc, kind)
    return packed


def conv_fwd(x, packed, bias, desc, epilogue=EPI_BIAS_RELU, mask=None):
    ho, wo = conv_out(desc.height, desc.stride), conv_out(desc.width, desc.stride)
    _dev(x, "x", (desc.batch, desc.height, desc.width, desc.cin_store))
    if bias is not None:
        _dev(bias, "bias", (32,))
    if mask is not None:
        _dev(mask, "mask", (desc.batch, ho, wo, 32))
    y = torch.empty((desc.batch, ho, wo, 32), device=x.device, dtype=torch.float32)
    call("dd_conv_fwd", x, packed, bias, mask, y, desc, epilogue)
    return y


def conv_fwd_bits(x, packed, bias, desc):
    """relu(conv(x) + bias) plus the ReLU signs as one uint32 per pixel (bit c = channel c is positive)."""
    ho, wo = conv_out(desc.height, desc.stride), conv_out(desc.width, desc.stride)
    _dev(x, "x", (desc.batch, desc.height, desc.width, desc.cin_store))
    _dev(bias, "bias", (32,))
    y = torch.empty((desc.batch, ho, wo, 32), device=x.device, dtype=torch.float32)
    bits = torch.empty((desc.batch, ho, wo), device=x.device, dtype=torch.int32)
    call("dd_conv_fwd_relu_bits", x, packed, bias, y, bits, desc)
    return y, bits


# Winograd F(2,3) along x for the 32 -> 32 stride-1 layer: 2/3 of the matrix-core work of the direct form, exact fp32
# arithmetic.  On by default for c2's forward and data gradient inside EncoderConvStack; the direct kernels stay
# available (set ops.WINOGRAD = False) and are what the kernel-level entry points above call.
WINOGRAD = True
WINOGRAD_2D = True      # forward / data gradient of c2 by F(2x2,3x3) instead of F(2,3) along x (16 instead of 24 multiplies per tile)


def _relu_bits(bits, desc, who):
    """The ReLU sign words a data gradient masks with: one int32 per pixel of the layer's input."""
    if not (bits.is_cuda and bits.dtype == torch.int32 and bits.is_contiguous() and tuple(bits.shape) == (desc.batch, desc.height, desc.width)):
        raise _lib.HotpathError(f"{who}: relu_bits must be a contiguous int32 [B,H,W] device tensor")
    return bits


# The two Winograd families of c2 -- "dd_conv_wino" (F(2,3) along x) and "dd_conv_wino2" (F(2x2,3x3)) -- have the same entry points
# with the same contracts: one body each, the public names below pick the family.
def _wino_pack(family, weight, desc, kind):
    _dev(weight, "weight", (32, 32, 3, 3))
    packed = torch.empty(size(family + "_packed_floats", desc), device=weight.device, dtype=torch.float32)
    call(family + "_pack", weight, packed, desc, kind)
    return packed


def _wino_fwd_bits(family, x, packed, bias, desc):
    _dev(x, "x", (desc.batch, desc.height, desc.width, 32))
    _dev(bias, "bias", (32,))
    y = torch.empty((desc.batch, desc.height, desc.width, 32), device=x.device, dtype=torch.float32)
    bits = torch.empty((desc.batch, desc.height, desc.width), device=x.device, dtype=torch.int32)
    call(family + "_fwd_relu_bits", x, packed, bias, y, bits, desc)
    return y, bits


def _wino_dgrad_bits(family, dy, packed, bits, desc):
    _dev(dy, "dy", (desc.batch, desc.height, desc.width, 32))
    _relu_bits(bits, desc, family[3:] + "_dgrad_bits")
    dx = torch.empty((desc.batch, desc.height, desc.width, 32), device=dy.device, dtype=torch.float32)
    call(family + "_dgrad_relu_bits", dy, packed, bits, dx, desc)
    return dx


def _wino_wgrad_buffers(family, x, dy, desc):
    _dev(x, "x", (desc.batch, desc.height, desc.width, 32))
    _dev(dy, "dy", (desc.batch, desc.height, desc.width, 32))
    nbytes = size(family + "_wgrad_workspace_bytes", desc)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    dw = torch.empty((32, 32, 3, 3), device=x.device, dtype=torch.float32)
    db = torch.empty(32, device=x.device, dtype=torch.float32)
    return ws, nbytes, dw, db


def _wino_wgrad(family, x, dy, desc):
    ws, nbytes, dw, db = _wino_wgrad_buffers(family, x, dy, desc)
    call(family + "_wgrad", x, dy, dw, db, ws, nbytes, desc)
    return dw, db


def conv_wino_pack(weight, desc, kind):
    return _wino_pack("dd_conv_wino", weight, desc, kind)


def conv_wino_fwd_bits(x, packed, bias, desc):
    return _wino_fwd_bits("dd_conv_wino", x, packed, bias, desc)


def conv_wino_dgrad_bits(dy, packed, bits, desc):
    return _wino_dgrad_bits("dd_conv_wino", dy, packed, bits, desc)


def conv_wino_wgrad(x, dy, desc):
    return _wino_wgrad("dd_conv_wino", x, dy, desc)


def wino2_desc(batch, h, w):
    """The c2-layer descriptor under which the F(2x2,3x3) Winograd kernels (dd_conv_wino2_*) take a 32 -> 32, k3, padding-1 convolution of
    ``batch`` NHWC images of h x w, or None where they do not (h, w >= 4 and dd_conv_wino2_packed_floats answers a size)."""
    if h < 4 or w < 4:
        return None
    d = conv_desc(batch, h, w, 32, 1)
    return d if _lib.lib().dd_conv_wino2_packed_floats(C.byref(d)) > 0 else None


def conv_wino2_pack(weight, desc, kind):
    return _wino_pack("dd_conv_wino2", weight, desc, kind)


def conv_wino2_fwd_bits(x, packed, bias, desc):
    return _wino_fwd_bits("dd_conv_wino2", x, packed, bias, desc)


def conv_wino2_dgrad_bits(dy, packed, bits, desc):
    return _wino_dgrad_bits("dd_conv_wino2", dy, packed, bits, desc)


def conv_wino2_dgrad_w1(dy, packed, bits, x4, desc):
    """c2's data gradient consumed in place: returns the 3 -> 32 layer's (dW1 [32,3,3,3], db1 [32]) instead of g1
    (dd_conv_wino2_dgrad_w1: g1 is never written to or re-read from HBM)."""
    _dev(dy, "dy", (desc.batch, desc.height, desc.width, 32))
    _dev(x4, "x4", (desc.batch, desc.height, desc.width, 4))
    _relu_bits(bits, desc, "conv_wino2_dgrad_w1")
    n = size("dd_conv_wino2_dgrad_w1_workspace_bytes", desc)
    ws = torch.empty(n, device=dy.device, dtype=torch.uint8)
    dw = torch.empty((32, 3, 3, 3), device=dy.device, dtype=torch.float32)
    db = torch.empty((32,), device=dy.device, dtype=torch.float32)
    call("dd_conv_wino2_dgrad_w1", dy, packed, bits, x4, dw, db, ws, n, desc)
    return dw, db


def conv_wino2_wgrad(x, dy, desc, finish_stream=None):
    if finish_stream is None:
        return _wino_wgrad("dd_conv_wino2", x, dy, desc)
    # the two reduce kernels go to `finish_stream` (beside whatever the caller launches next); the caller's stream has to
    # wait for the returned event before it reads dw / db
    ws, nbytes, dw, db = _wino_wgrad_buffers("dd_conv_wino2", x, dy, desc)
    main = torch.cuda.current_stream()
    call("dd_conv_wino2_wgrad_partials", x, dy, ws, nbytes, desc)
    finish_stream.wait_event(main.record_event())
    with torch.cuda.stream(finish_stream):
        for t in (ws, dw, db):
            t.record_stream(finish_stream)
        call("dd_conv_wino2_wgrad_finish", ws, nbytes, dw, db, desc)
        done = finish_stream.record_event()
    return dw, db, done


def conv_dgrad_bits(dy, packed_dgrad, bits, desc):
    ho, wo = conv_out(desc.height, desc.stride), conv_out(desc.width, desc.stride)
    _dev(dy, "dy", (desc.batch, ho, wo, 32))
    _relu_bits(bits, desc, "conv_dgrad_bits")
    dx = torch.empty((desc.batch, desc.height, desc.width, 32), device=dy.device, dtype=torch.float32)
    call("dd_conv_dgrad_relu_bits", dy, packed_dgrad, bits, dx, desc)
    return dx


def conv_dgrad(dy, packed_dgrad, relu_src, desc):
    ho, wo = conv_out(desc.height, desc.stride), conv_out(desc.width, desc.stride)
    _dev(dy, "dy", (desc.batch, ho, wo, 32))
    if relu_src is not None:
        _dev(relu_src, "relu_src", (desc.batch, desc.height, desc.width, 32))
    dx = torch.empty((desc.batch, desc.height, desc.width, 32), device=dy.device, dtype=torch.float32)
    call("dd_conv_dgrad", dy, packed_dgrad, relu_src, dx, desc)
    return dx


def conv_wgrad(x, dy, desc):
    ho, wo = conv_out(desc.height, desc.stride), conv_out(desc.width, desc.stride)
    _dev(x, "x", (desc.batch, desc.height, desc.width, desc.cin_store))
    _dev(dy, "dy", (desc.batch, ho, wo, 32))
    nbytes = size("dd_conv_wgrad_workspace_bytes", desc)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    dw = torch.empty((32, desc.cin_real, 3, 3), device=x.device, dtype=torch.float32)
    db = torch.empty(32, device=x.device, dtype=torch.float32)
    call("dd_conv_wgrad", x, dy, dw, db, ws, nbytes, desc)
    return dw, db


def add(a, b):
    _dev(a, "a")
    _dev(b, "b", a.shape)
    out = torch.empty_like(a)
    call("dd_add", a, b, out, a.numel())
    return out


def relu_bwd(dy, y):
    _dev(dy, "dy", y.shape)
    _dev(y, "y")
    out = torch.empty_like(y)
    call("dd_relu_bwd", dy, y, out, y.numel())
    return out


def relu_sign_bits(x):
    """int32 [B,H,W]: bit c = x[b,y,x,c] > 0 of an NHWC activation with 32 channels (dd_relu_sign_bits)."""
    _dev(x, "x")
    if x.dim() != 4 or x.shape[3] != 32:
        raise _lib.HotpathError(f"relu_sign_bits: expected [B,H,W,32], got {tuple(x.shape)}")
    bits = torch.empty(x.shape[:3], device=x.device, dtype=torch.int32)
    call("dd_relu_sign_bits", x, bits, bits.numel())
    return bits


def channel_slice(v):
    """``v`` [B,H,W,C]: (dense NHWC buffer [B,H,W,cs] it is a channel slice of, channel offset), or None (dense tensors: (v, 0))."""
    if v.dim() != 4:
        return None
    if v.is_contiguous():
        return v, 0
    b, h, w, c = v.shape
    sb, sh, sw, sc = v.stride()
    if sc != 1 or sw < c or sh != w * sw or (b > 1 and sb != h * sh):
        return None
    coff = v.storage_offset() % sw
    if coff + c > sw or v.storage_offset() != coff or v.untyped_storage().nbytes() // v.element_size() < b * h * w * sw:
        return None
    return v.as_strided((b, h, w, sw), (h * w * sw, w * sw, sw, 1), 0), coff


def relu_bwd_pad_bits(dy, bits_pad):
    """dy [B,H,W,32] (dense, or a channel slice of a dense NHWC buffer: read where it lies), sign words [B,H+2,W+2] ->
    [B,H+2,W+2,32]: dy behind the ReLU in the interior, zero on the border ring."""
    src = channel_slice(dy)
    if src is None:
        src = (dy.contiguous(), 0)
    buf, coff = src
    _dev(buf, "dy")
    b, h, w, c = dy.shape
    if c != 32 or coff % 4 or buf.shape[3] % 4 or not (bits_pad.is_cuda and bits_pad.dtype == torch.int32 and bits_pad.is_contiguous() and
                                                        tuple(bits_pad.shape) == (b, h + 2, w + 2)):
        raise _lib.HotpathError(f"relu_bwd_pad_bits: dy {tuple(dy.shape)} needs 32 channels (a 4-aligned slice) and contiguous int32 sign words [B,H+2,W+2], got {tuple(bits_pad.shape)}")
    out = torch.empty((b, h + 2, w + 2, 32), device=dy.device, dtype=torch.float32)
    call("dd_relu_bwd_pad_bits", buf, bits_pad, out, b, h, w, buf.shape[3], coff)
    return out


# The pool shims of both precisions share their bodies: the feature and its gradient are fp32 here and bf16 in ops_bf16 (pooled and
# dpooled are fp32 in both).  A body takes the dtype TOGETHER with that dtype's entry points; the public names fix the pair.
_POOL4_F32 = (torch.float32, {"fwd": "dd_pool4_fwd", "relu_bwd": "dd_pool4_relu_bwd", "idx_elems": "dd_pool4_idx_elems",
                              "fwd_idx": "dd_pool4_fwd_idx", "idx_relu_bwd": "dd_pool4_idx_relu_bwd"})


def _pool4_fwd(kind, feat):
    dtype, entry = kind
    b, h, w, c = feat.shape
    _dev(feat, "feat", dtype=dtype)
    out = torch.empty((b, (c * h * w) // 4), device=feat.device, dtype=torch.float32)
    call(entry["fwd"], feat, out, b, h, w, c)
    return out


def _pool4_fwd_idx(kind, feat):
    dtype, entry = kind
    b, h, w, c = feat.shape
    _dev(feat, "feat", dtype=dtype)
    n = size(entry["idx_elems"], b, h, w, c)
    out = torch.empty((b, (c * h * w) // 4), device=feat.device, dtype=torch.float32)
    idx = torch.empty((n,), device=feat.device, dtype=torch.int16)
    call(entry["fwd_idx"], feat, out, idx, b, h, w, c)
    return out, idx


def _pool4_idx_relu_bwd(kind, dpooled, idx, shape):
    dtype, entry = kind
    b, h, w, c = shape
    _dev(dpooled, "dpooled", (b, (c * h * w) // 4))
    if idx.dtype != torch.int16 or not idx.is_cuda or idx.numel() != b * (h * w // 4) * (c // 4):
        raise _lib.HotpathError(f"{entry['idx_relu_bwd']}: bad routing codes {tuple(idx.shape)} {idx.dtype}")
    out = torch.empty(shape, device=dpooled.device, dtype=dtype)
    call(entry["idx_relu_bwd"], dpooled, idx, out, b, h, w, c)
    return out


def _pool4_relu_bwd(kind, dpooled, feat):
    dtype, entry = kind
    b, h, w, c = feat.shape
    _dev(dpooled, "dpooled", (b, (c * h * w) // 4))
    _dev(feat, "feat", dtype=dtype)
    out = torch.empty_like(feat)
    call(entry["relu_bwd"], dpooled, feat, out, b, h, w, c)
    return out


def pool4_fwd(feat):
    return _pool4_fwd(_POOL4_F32, feat)


def pool4_has_idx(h, w, c):
    """The routing-code form needs windows that stay inside one channel plane."""
    return (h * w) % 4 == 0 and c % 4 == 0


def pool4_fwd_idx(feat):
    """pooled, codes: max_pool1d(4) + the backward's routing (dd_pool4_fwd_idx)."""
    return _pool4_fwd_idx(_POOL4_F32, feat)


def pool4_idx_relu_bwd(dpooled, idx, shape):
    return _pool4_idx_relu_bwd(_POOL4_F32, dpooled, idx, shape)


def pool4_relu_bwd(dpooled, feat):
    return _pool4_relu_bwd(_POOL4_F32, dpooled, feat)


def pool4_relu_bwd_add(dpooled, feat, gfeat):
    """(feat > 0) * (gfeat + routed dpooled): the c3 feature's gradient when both the pool and the box heads consume it, one pass."""
    b, h, w, c = feat.shape
    _dev(dpooled, "dpooled", (b, (c * h * w) // 4))
    _dev(feat, "feat")
    _dev(gfeat, "gfeat", feat.shape)
    out = torch.empty_like(feat)
    call("dd_pool4_relu_bwd_add", dpooled, feat, gfeat, out, b, h, w, c)
    return out


# Observers of the encoder's backward (optim.HipAdam registers itself in overlap_with_backward and leaves in close).  Each has
#   backward_phase1()  called when backward enters its long MFMA-bound stretch (the c2 weight / data gradient kernels, ~4.4 ms at
#                      bs = 32 that use a third of the HBM bandwidth): the place to start bandwidth-bound side work such as the
#                      optimizer pass of already-finished gradients;
#   backward_phase2()  called between c2's two gradient kernels, ~1.2 ms later: the place for work that has to WAIT for something
#                      started at the top of the backward (factor mode of ddp.GradSync: the gathered factors of the big Linear layers);
#   c2_dgrad_first     whether it needs c2's data gradient in front of its weight gradient (same results either way; asked when the
#                      backward runs, true if any observer says so: see EncoderConvStack.backward).
# The list is the whole mechanism: which order an observer wants, and what it launches where, is the observer's business.
BACKWARD_OBSERVERS = []

# c1's weight gradient taken from c2's data gradient inside conv_wino2_fwd<EPI_RELU_BITS_W1> (2-D Winograd path only)
FUSE_C1_WGRAD = True      # c1's weight gradient inside c2's data gradient (the 2-D Winograd form); tests may switch it off in process

# c2's three kernel families by path: (pack, forward, data gradient, weight gradient).  NAMES, looked up in this module when they are
# called: bench.py, tools/ and tests replace these functions by assignment on the module (_lib.py's docstring).
_C2_PATHS = {"wino2": ("conv_wino2_pack", "conv_wino2_fwd_bits", "conv_wino2_dgrad_bits", "conv_wino2_wgrad"),
             "wino": ("conv_wino_pack", "conv_wino_fwd_bits", "conv_wino_dgrad_bits", "conv_wino_wgrad"),
             "direct": ("conv_pack", "conv_fwd_bits", "conv_dgrad_bits", "conv_wgrad")}


def _c2(path):
    return [globals()[name] for name in _C2_PATHS[path]]


# Test hook: when set to a dict, EncoderConvStack.forward leaves its three ReLU outputs (NHWC) in it, so that a checker can
# replay the product's ReLU / max-pool decisions (oracle.branch); None in production.
TRACE = None

_PACK_STREAMS = {}


def _pack_stream(device):
    """Side stream for the weight-image packs of EncoderConvStack (one per device)."""
    key = torch.device(device).index
    if key not in _PACK_STREAMS:
        _PACK_STREAMS[key] = torch.cuda.Stream(device=device)
    return _PACK_STREAMS[key]


# ------------------------------------------------------------------------------------------------ encoder conv stack
class EncoderConvStack(torch.autograd.Function):
    """c1 -> ReLU -> c2 -> ReLU -> c3 (stride 2) -> ReLU [-> NCHW-order max_pool1d(4)] as one autograd node.

    Reference: Encoder.forward, src/autoencoder/components.py:41-47.  Running the three layers as
    one node lets the backward fuse each ReLU's gradient into the neighbouring kernel (the pool
    backward masks with c3's output, each data-gradient kernel masks with its layer's input) and
    keeps every intermediate in NHWC.

    forward(x4 [B,H,W,4], w1,b1,w2,b2,w3,b3, pool) -> feat [B,Ho,Wo,32] (NHWC)   or  pooled [B, 32*Ho*Wo/4]
    """

    @staticmethod
    def forward(ctx, x4, w1, b1, w2, b2, w3, b3, pool, rows_per_task):
        b, h, w, _ = x4.shape
        d1 = conv_desc(b, h, w, 3, 1, rows_per_task)
        d2 = conv_desc(b, h, w, 32, 1, rows_per_task)
        d3 = conv_desc(b, h, w, 32, 2, rows_per_task)
        # Operand images.  Only c1's is needed at once; the other four (c2 / c3 forward, and the backward's two: the weights do
        # not change before the backward, where these tiny kernels would sit on the critical path behind the optimizer pass
        # that overlaps it -- 4 us alone, up to 390 us squeezed between Adam's workgroups) are packed on a side stream
        # while c1's forward runs: five 5-us launches less on the critical path.
        need = ctx.needs_input_grad               # (x4, w1, b1, w2, b2, w3, b3, ...)
        path = "wino2" if WINOGRAD and WINOGRAD_2D else "wino" if WINOGRAD else "direct"      # c2: F(2x2,3x3), F(2,3) along x, direct
        c2_pack, c2_fwd_bits, _, _ = _c2(path)
        p1 = conv_pack(w1, d1, PACK_FWD)
        main = torch.cuda.current_stream()
        side = _pack_stream(x4.device)
        side.wait_event(main.record_event())
        with torch.cuda.stream(side):
            p2 = c2_pack(w2, d2, PACK_FWD)
            p3 = conv_pack(w3, d3, PACK_FWD)
            p2d = p3d = torch.empty(0, device=x4.device)
            if need[1] or need[2] or need[3] or need[4]:
                p3d = conv_pack(w3, d3, PACK_DGRAD_S2)
            if need[1] or need[2]:
                p2d = c2_pack(w2, d2, PACK_DGRAD_S1)
            for t in (p2, p3, p2d, p3d):
                t.record_stream(main)             # allocated under the side stream, consumed on the main one
            packed_ready = side.record_event()
        # c1 / c2 also emit their ReLU signs as bit planes (60 MB instead of 1.9 GB to re-read in the backward)
        a1, s1 = conv_fwd_bits(x4, p1, b1, d1)
        main.wait_event(packed_ready)
        a2, s2 = c2_fwd_bits(a1, p2, b2, d2)
        a3 = conv_fwd(a2, p3, b3, d3)
        if TRACE is not None:
            TRACE.update(a1=a1, a2=a2, a3=a3)
        ctx.c2_path = path
        ctx.pool = int(pool)                  # 0: conv feature, 1: pooled vector, 2: both (joint roadmap + box model)
        ctx.rows_per_task = rows_per_task
        ctx.a3_shape = tuple(a3.shape)
        if ctx.pool == 1 and pool4_has_idx(*a3.shape[1:]):
            # the pool decides the backward's routing now (4 bits per window): the feature itself is not kept
            pooled, codes = pool4_fwd_idx(a3)
            ctx.save_for_backward(x4, a1, a2, codes, p2d, p3d, s1, s2)
            ctx.codes = True
            return pooled
        ctx.codes = False
        ctx.save_for_backward(x4, a1, a2, a3, p2d, p3d, s1, s2)
        if ctx.pool == 2:
            return a3, pool4_fwd(a3)
        if ctx.pool:
            return pool4_fwd(a3)
        return a3

    @staticmethod
    def backward(ctx, grad, grad_pooled=None):
        x4, a1, a2, a3, p2d, p3d, s1, s2 = ctx.saved_tensors
        _, _, c2_dgrad_bits, c2_wgrad = _c2(ctx.c2_path)
        wino2 = ctx.c2_path == "wino2"
        b, h, w, _ = x4.shape
        rpt = ctx.rows_per_task
        d1, d2, d3 = conv_desc(b, h, w, 3, 1, rpt), conv_desc(b, h, w, 32, 1, rpt), conv_desc(b, h, w, 32, 2, rpt)
        if ctx.pool == 2:                     # two consumers of the c3 feature: their gradients add
            if grad is not None and grad_pooled is not None and a3.shape[3] == 32 and (a3.shape[1] * a3.shape[2]) % 4 == 0:
                g3 = pool4_relu_bwd_add(grad_pooled.contiguous(), a3, grad.contiguous())      # one pass instead of three over the 481 MB feature
            else:
                parts = []
                if grad is not None:
                    parts.append(relu_bwd(grad.contiguous(), a3))
                if grad_pooled is not None:
                    parts.append(pool4_relu_bwd(grad_pooled.contiguous(), a3))
                g3 = parts[0] if len(parts) == 1 else add(parts[0], parts[1])
        else:
            grad = grad.contiguous()
            if ctx.codes:
                g3 = pool4_idx_relu_bwd(grad, a3, ctx.a3_shape)      # a3 holds the routing codes here
            else:
                g3 = pool4_relu_bwd(grad, a3) if ctx.pool else relu_bwd(grad, a3)
        need = ctx.needs_input_grad
        dw3, db3 = conv_wgrad(a2, g3, d3) if (need[5] or need[6]) else (None, None)
        dw2 = db2 = dw1 = db1 = None
        if need[1] or need[2] or need[3] or need[4]:
            g2 = conv_dgrad_bits(g3, p3d, s2, d3)
            del g3
            for obs in BACKWARD_OBSERVERS:
                obs.backward_phase1()
            reduced = None

            def c2_weight_gradient():
                nonlocal dw2, db2, reduced
                if need[3] or need[4]:
                    if wino2:      # the reduce of the partials runs on the side stream, beside c2's data gradient
                        dw2, db2, reduced = c2_wgrad(a1, g2, d2, finish_stream=_pack_stream(g2.device))
                    else:
                        dw2, db2 = c2_wgrad(a1, g2, d2)

            def c2_data_gradient():
                nonlocal dw1, db1
                if (need[1] or need[2]) and wino2 and FUSE_C1_WGRAD:
                    dw1, db1 = conv_wino2_dgrad_w1(g2, p2d, s1, x4, d2)      # g1 never leaves the registers
                elif need[1] or need[2]:
                    dw1, db1 = conv_wgrad(x4, c2_dgrad_bits(g2, p2d, s1, d2), d1)

            # Data gradient first when an observer asks for it (optim.HipAdam: rank-B passes, factor mode of ddp.GradSync): the optimizer
            # passes of the two big Linear layers can only start once their gathered factors have arrived, ~3 ms into the backward, and
            # they can only run BESIDE c2's weight gradient (440 registers per SIMD: one 48-register Adam wave fits; the data-gradient
            # kernel's 475 leave no room) -- so that kernel goes last and phase 2 sits in front of it
            first, second = c2_weight_gradient, c2_data_gradient
            if any(obs.c2_dgrad_first for obs in BACKWARD_OBSERVERS):
                first, second = second, first
            first()
            for obs in BACKWARD_OBSERVERS:
                obs.backward_phase2()
            second()
            del g2
            if reduced is not None:
                torch.cuda.current_stream().wait_event(reduced)
        return None, dw1, db1, dw2, db2, dw3, db3, None, None


def encoder_conv_stack(x4, c1, c2, c3, pool, rows_per_task=0):
    return EncoderConvStack.apply(x4, c1.weight, c1.bias, c2.weight, c2.bias, c3.weight, c3.bias, pool, rows_per_task)


# ------------------------------------------------------------------------------------------------ skinny GEMMs
def _linear_ws(m, n, k, device):
    nbytes = size("dd_linear_workspace_bytes", m, n, k)
    return torch.empty(nbytes, device=device, dtype=torch.uint8), nbytes


# data_ptr of an nn.Linear weight -> optim.HipAdam in rank-B mode: Linear.backward hands (x, dy) over instead of forming dW
RANKB = {}


class Linear(torch.autograd.Function):
    """y = x W^T + b with nn.Linear's [out, in] weight, all three passes on the fp32 matrix cores
    (dd_linear_fwd / dgrad / wgrad).  Reference call sites: components.py:105 (DenseBlock.fc1),
    components.py:51 (fc_z_out), roadmap_bce_v2.py:75 (head)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        m, k = x.shape
        n = weight.shape[0]
        _dev(x, "x")
        _dev(weight, "weight", (n, k))
        if bias is not None:
            _dev(bias, "bias", (n,))
        y = torch.empty((m, n), device=x.device, dtype=torch.float32)
        ws, nbytes = _linear_ws(m, n, k, x.device)
        call("dd_linear_fwd", x, weight, bias, y, m, n, k, ws, nbytes)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        m, k = x.shape
        n = weight.shape[0]
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ws, nbytes = _linear_ws(m, n, k, x.device)
            call("dd_linear_dgrad", dy, weight, dx, m, n, k, ws, nbytes)
        sync = _ddp.FACTOR_SYNC.get(weight.data_ptr()) if _ddp.FACTOR_SYNC else None
        fused = RANKB.get(weight.data_ptr()) if RANKB else None
        taken = 0
        if sync is not None and ctx.needs_input_grad[1] and sync.linear_factors(weight, x, dy):
            # data parallel, factor mode (ddp.GradSync): x and dy travel instead of dW; the optimizer forms the global-batch gradient
            # (rank-B mode of the optimizer: inside its Adam pass, the bias from the gathered dy as well)
            if ctx.has_bias and ctx.needs_input_grad[2] and not (fused is not None and fused.factor_bias(weight, sync.world * m)):
                db = column_sum(dy)
        elif fused is not None and ctx.needs_input_grad[1] and (taken := fused.linear_factors(weight, x, dy)):
            # rank-B mode (optim.HipAdam): no dW at all, dd_adam_step_rankb forms it from (x, dy) inside the optimizer pass
            if taken == 1 and ctx.has_bias and ctx.needs_input_grad[2]:
                db = column_sum(dy)
        elif ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw = torch.empty_like(weight)
            db = torch.empty(n, device=x.device, dtype=torch.float32) if ctx.has_bias else None
            call("dd_linear_wgrad", dy, x, dw, db, m, n, k)
        return dx, dw, db


def linear(x, weight, bias):
    x = x.contiguous()
    # factor mode of ddp.GradSync: a big input (fc1's 120 MB of pooled activations) starts its all-gather now, not in the backward.
    # Decided HERE: inside Function.forward grad mode is always off and ctx.needs_input_grad ignores torch.no_grad()
    if _ddp.FACTOR_SYNC and torch.is_grad_enabled() and weight.requires_grad:
        sync = _ddp.FACTOR_SYNC.get(weight.data_ptr())
        if sync is not None:
            sync.linear_input(weight, x)
    return Linear.apply(x, weight, bias)


def linear_sigmoid_gt(x, weight, bias, tau):
    """``sigmoid(x W^T + b) > tau`` as torch.bool [M, N] from one kernel (dd_linear_sigmoid_gt): element for element what
    ``sigmoid(linear(x, W, b)) > tau`` gives, without the logits or the probabilities ever reaching memory.  The road-map head at
    prediction time; outside autograd."""
    x = x.detach().contiguous()
    m, k = x.shape
    n = weight.shape[0]
    _dev(x, "x")
    _dev(weight.detach(), "weight", (n, k))
    if bias is not None:
        _dev(bias.detach(), "bias", (n,))
    out = torch.empty((m, n), device=x.device, dtype=torch.uint8)
    call("dd_linear_sigmoid_gt", x, weight, bias, float(tau), out, m, n, k)
    return out.view(torch.bool)


def column_sum(dy):
    """db [n] = sum over the rows of dy [m, n] on the hot path's own kernel (dd_column_sum): the bias gradient of a Linear layer whose
    weight gradient is not formed by dd_linear_wgrad."""
    m, n = dy.shape
    _dev(dy, "dy")
    db = torch.empty(n, device=dy.device, dtype=torch.float32)
    call("dd_column_sum", dy, db, m, n)
    return db


def linear_wgrad(dy, x, dw):
    """dw [n, k] = dy^T x for dy [m, n], x [m, k] (dd_linear_wgrad without the bias sum): the optimizer's global-batch weight gradient
    from gathered factors (ddp.GradSync, factor mode)."""
    m, n = dy.shape
    k = x.shape[1]
    _dev(dy, "dy")
    _dev(x, "x", (m, k))
    _dev(dw, "dw", (n, k))
    call("dd_linear_wgrad", dy, x, dw, None, m, n, k)


# ------------------------------------------------------------------------------------------------ dense block tail
class BnReluDrop(torch.autograd.Function):
    """BatchNorm1d -> ReLU -> dropout(keep mask) in one kernel each way (components.py:105-108)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, keep, training, eps, momentum, scale, num_batches_tracked=None):
        rows, feat = x.shape
        if num_batches_tracked is not None and not (num_batches_tracked.is_cuda and num_batches_tracked.dtype == torch.int64):
            raise _lib.HotpathError("bn_relu_drop: num_batches_tracked must be an int64 device tensor")
        _dev(x, "x")
        y = torch.empty_like(x)
        save_mean = torch.empty(feat, device=x.device, dtype=torch.float32)
        save_inv = torch.empty(feat, device=x.device, dtype=torch.float32)
        call("dd_bn_relu_drop_fwd", x, gamma, beta, running_mean, running_var, keep, y, save_mean, save_inv, rows, feat, eps, momentum, scale,
             int(training), num_batches_tracked)
        if TRACE is not None:
            TRACE.setdefault("dense", []).append(y)
        ctx.save_for_backward(x, y, gamma, keep, save_mean, save_inv, running_mean, running_var)
        ctx.cfg = (bool(training), eps, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, keep, save_mean, save_inv, running_mean, running_var = ctx.saved_tensors
        training, eps, scale = ctx.cfg
        rows, feat = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dgamma = torch.empty_like(gamma)
        dbeta = torch.empty_like(gamma)
        call("dd_bn_relu_drop_bwd", dy, x, y, gamma, keep, save_mean, save_inv, running_mean, running_var, dx, dgamma, dbeta, rows, feat, eps, scale,
             int(training))
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------ encoder tail
FUSE_MLP_TAIL = True      # the encoder tail as one launch each way where its sizes allow (dd_mlp_tail_supported)


def mlp_tail_supported(m, h1, h2, l):
    return FUSE_MLP_TAIL and bool(_lib.lib().dd_mlp_tail_supported(m, h1, h2, l))


class EncoderTail(torch.autograd.Function):
    """BatchNorm1d -> ReLU -> dropout -> Linear -> BatchNorm1d -> ReLU -> dropout -> Linear as one launch each way
    (dd_mlp_tail_fwd / dd_mlp_tail_bwd; reference components.py:48-51 + DenseBlock.forward :104-109).

    forward(lin1, gamma1, beta1, w2, bias2, gamma2, beta2, wz, bz, keep1, keep2, bn1, bn2, scale1, scale2) -> z
    ``bn1`` / ``bn2`` are the BatchNorm1d modules (running statistics, eps, momentum, mode)."""

    @staticmethod
    def forward(ctx, lin1, gamma1, beta1, w2, bias2, gamma2, beta2, wz, bz, keep1, keep2, bn1, bn2, scale1, scale2):
        m, h1 = lin1.shape
        h2, l = w2.shape[0], wz.shape[0]
        for name, t, shape in (("lin1", lin1, None), ("w2", w2, (h2, h1)), ("wz", wz, (l, h2)), ("bias2", bias2, (h2,)), ("bz", bz, (l,)),
                               ("gamma1", gamma1, (h1,)), ("beta1", beta1, (h1,)), ("gamma2", gamma2, (h2,)), ("beta2", beta2, (h2,))):
            _dev(t, name, shape)
        if keep1 is not None:
            _dev(keep1, "keep1", (m, h1))
        if keep2 is not None:
            _dev(keep2, "keep2", (m, h2))
        training = bool(bn1.training)
        dev = lin1.device
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        y1, lin2, y2, z = new(m, h1), new(m, h2), new(m, h2), new(m, l)
        mean1, inv1, mean2, inv2 = new(h1), new(h1), new(h2), new(h2)
        mom = lambda bn: 0.1 if bn.momentum is None else bn.momentum
        nbt = lambda bn: bn.num_batches_tracked if (training and bn.num_batches_tracked is not None) else None
        call("dd_mlp_tail_fwd", lin1, gamma1, beta1, bn1.running_mean, bn1.running_var, nbt(bn1), keep1, w2, bias2, gamma2, beta2, bn2.running_mean,
             bn2.running_var, nbt(bn2), keep2, wz, bz, y1, lin2, y2, z, mean1, inv1, mean2, inv2, m, h1, h2, l, bn1.eps, bn2.eps, mom(bn1), mom(bn2),
             scale1, scale2, int(training))
        if TRACE is not None:
            TRACE.setdefault("dense", []).extend([y1, y2])
        ctx.save_for_backward(lin1, y1, lin2, y2, gamma1, gamma2, keep1, keep2, w2, wz, mean1, inv1, mean2, inv2,
                              bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var)
        ctx.cfg = (training, bn1.eps, bn2.eps, scale1, scale2)
        return z

    @staticmethod
    def backward(ctx, dz):
        (lin1, y1, lin2, y2, gamma1, gamma2, keep1, keep2, w2, wz, mean1, inv1, mean2, inv2, rm1, rv1, rm2, rv2) = ctx.saved_tensors
        training, eps1, eps2, scale1, scale2 = ctx.cfg
        m, h1 = lin1.shape
        h2, l = w2.shape[0], wz.shape[0]
        dz = dz.contiguous()
        dlin1 = torch.empty_like(lin1)
        dg1, db1, dg2, db2 = torch.empty_like(gamma1), torch.empty_like(gamma1), torch.empty_like(gamma2), torch.empty_like(gamma2)
        dw2, dwz = torch.empty_like(w2), torch.empty_like(wz)
        dbias2 = torch.empty(h2, device=dz.device, dtype=torch.float32)
        dbz = torch.empty(l, device=dz.device, dtype=torch.float32)
        call("dd_mlp_tail_bwd", dz, lin1, y1, lin2, y2, gamma1, gamma2, keep1, keep2, w2, wz, mean1, inv1, mean2, inv2, rm1, rv1, rm2, rv2, dlin1,
             dg1, db1, dw2, dbias2, dg2, db2, dwz, dbz, m, h1, h2, l, eps1, eps2, scale1, scale2, int(training))
        return dlin1, dg1, db1, dw2, dbias2, dg2, db2, dwz, dbz, None, None, None, None, None, None



# ------------------------------------------------------------------------------------------------ losses
PTR_TABLE_MAX = 64        # samples per pointer table of dd_bce_logits_u8_ptrs (the table travels in the kernel arguments)


def _check_masks(target, n):
    """The collate's tuple of per-sample masks for ``n`` logits -> elements per sample; raises on anything the byte kernels cannot read."""
    b = len(target)
    per = n // max(b, 1)
    for t in target:
        if not (t.is_cuda and t.is_contiguous() and t.dtype in (torch.bool, torch.uint8) and t.numel() == per):
            raise _lib.HotpathError("bce: per-sample masks must be contiguous bool / uint8 GPU tensors of logits.numel() / batch elements")
    if b * per != n:
        raise _lib.HotpathError(f"bce: {b} masks of {per} elements for {n} logits")
    return per


def _stack_masks(target, shape):
    """One byte copy of the per-sample masks into a tensor of the logits' shape, for dd_bce_logits_u8."""
    return torch.stack(tuple(t.reshape(-1) for t in target), dim=0).reshape(shape)


def _loss_ws(n, device):
    return torch.empty(size("dd_loss_workspace_bytes", n), device=device, dtype=torch.uint8)


def _scaled_loss_grad(ctx, dz, g):
    """dz * g for the 0-dim upstream gradient ``g`` of a scalar loss.  The forward already wrote d(loss)/d(input), so for a
    plain ``loss.backward()`` (g == 1, known only on the device) nothing needs to move: ``dd_scale_by_device_scalar`` scales
    the saved buffer in place and is skipped on the device when g == 1.  The in-place pass is remembered on ``ctx``: a
    repeated backward through a retained graph (``retain_graph=True``) finds the buffer already carrying the previous factor
    and takes the generic out-of-place route with the ratio of the two factors."""
    prev = getattr(ctx, "applied_scale", None)
    if prev is not None:
        if float(prev) == 0.0:
            raise RuntimeError("loss backward: the retained graph was first back-propagated with a zero upstream gradient; "
                               "its saved loss gradient cannot be rescaled (run the forward again)")
        return dz * (g / prev)
    if (g.numel() == 1 and g.is_cuda and g.dtype == torch.float32 and dz.is_contiguous() and dz.dtype == torch.float32
            and dz.data_ptr() % 16 == 0 and not torch.is_grad_enabled()):
        call("dd_scale_by_device_scalar", dz, g, dz.numel())
        ctx.applied_scale = g.detach()
        return dz
    return dz * g


class BceWithLogits(torch.autograd.Function):
    """mean BCE-with-logits; the gradient is produced by the forward's single pass (roadmap_bce_v2.py:106)."""

    @staticmethod
    def forward(ctx, logits, target):
        _dev(logits, "logits")
        n = logits.numel()
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        dz = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        if isinstance(target, (tuple, list)):               # the collate's tuple of per-sample masks: stacked (any batch size)
            _check_masks(target, n)
            target = _stack_masks(target, logits.shape)
        if target.dtype in (torch.bool, torch.uint8):      # the dataset's bool road masks, read as bytes
            if not target.is_cuda or not target.is_contiguous() or target.shape != logits.shape:
                raise _lib.HotpathError(f"bce: target must be a contiguous GPU tensor of shape {tuple(logits.shape)}")
            call("dd_bce_logits_u8", logits, target, loss, dz, None, n, 1.0, _loss_ws(n, logits.device))
        else:
            _dev(target, "target", logits.shape)
            call("dd_bce_logits", logits, target, loss, dz, None, n, 1.0, _loss_ws(n, logits.device))
        ctx.save_for_backward(dz)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return _scaled_loss_grad(ctx, dz, g), None


class BceWithLogitsProbs(torch.autograd.Function):
    """(mean BCE-with-logits, sigmoid(logits)) from ONE pass over the logits: the roadmap step needs both
    (roadmap_bce_v2.py:81 and :106) and the separate sigmoid kernel would read the 82 MB of logits a second time.
    The probabilities carry no gradient (the reference takes the loss from the logits)."""

    @staticmethod
    def forward(ctx, logits, target):
        """``target``: a tensor of the logits' shape, or the collate's TUPLE of per-sample bool / uint8 masks (read through
        a pointer table: no torch.stack copy)."""
        _dev(logits, "logits")
        n = logits.numel()
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        probs = torch.empty_like(logits)
        dz = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        if isinstance(target, (tuple, list)):
            b, per = len(target), _check_masks(target, n)
            if b > PTR_TABLE_MAX:
                # past the pointer table's size the masks are stacked after all and take dd_bce_logits_u8: the same arithmetic in
                # the same order over the same grid, so the same bits as the table kernel would give
                target = _stack_masks(target, logits.shape)
        if isinstance(target, (tuple, list)):
            table = (C.c_void_p * b)(*[t.data_ptr() for t in target])
            call("dd_bce_logits_u8_ptrs", logits, table, b, per, loss, dz, probs, 1.0, _loss_ws(n, logits.device))
            ctx.save_for_backward(dz)
            ctx.mark_non_differentiable(probs)
            ctx.set_materialize_grads(False)
            return loss, probs
        if not target.is_cuda or not target.is_contiguous() or target.shape != logits.shape:
            raise _lib.HotpathError(f"bce: target must be a contiguous GPU tensor of shape {tuple(logits.shape)}")
        if target.dtype in (torch.bool, torch.uint8):
            call("dd_bce_logits_u8", logits, target, loss, dz, probs, n, 1.0, _loss_ws(n, logits.device))
        else:
            _dev(target, "target", logits.shape)
            call("dd_bce_logits", logits, target, loss, dz, probs, n, 1.0, _loss_ws(n, logits.device))
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(probs)
        ctx.set_materialize_grads(False)      # no 82 MB of zeros for the probabilities' (unused) gradient slot
        return loss, probs

    @staticmethod
    def backward(ctx, g, _gp):
        (dz,) = ctx.saved_tensors
        if g is None:
            return None, None
        return _scaled_loss_grad(ctx, dz, g), None


class MseLoss(torch.autograd.Function):
    """mean((pred - target)^2) (autoencoder.py:91; symmetric in its arguments)."""

    @staticmethod
    def forward(ctx, pred, target):
        _dev(pred, "pred")
        _dev(target, "target", pred.shape)
        n = pred.numel()
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        da = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        call("dd_mse", pred, target, loss, da, n, 1.0, _loss_ws(n, pred.device))
        ctx.save_for_backward(da)
        return loss

    @staticmethod
    def backward(ctx, g):
        (da,) = ctx.saved_tensors
        return _scaled_loss_grad(ctx, da, g), None


class BceProbs(torch.autograd.Function):
    """mean F.binary_cross_entropy on probabilities (spatial_w_rm.py:131), gradient from the same pass."""

    @staticmethod
    def forward(ctx, probs, target):
        _dev(probs, "probs")
        _dev(target, "target", probs.shape)
        n = probs.numel()
        loss = torch.empty((), device=probs.device, dtype=torch.float32)
        dp = torch.empty_like(probs) if ctx.needs_input_grad[0] else None
        call("dd_bce_probs", probs, target, loss, dp, n, 1.0, _loss_ws(n, probs.device))
        ctx.save_for_backward(dp)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return _scaled_loss_grad(ctx, dp, g), None


POS_WEIGHT_AUTO = -1.0      # DD_POS_WEIGHT_AUTO


def _box_loss_operands(probs, target, pos_weight):
    """Host-side check of ``box_loss``'s operands -> (target as the kernels read it, DD_TARGET_*, pos_weight as the ABI takes it)."""
    if not isinstance(probs, torch.Tensor) or probs.dim() != 2:
        raise _lib.HotpathError(f"box_loss: probs must be [B, P], got {tuple(getattr(probs, 'shape', ()))}")
    _dev(probs, "probs")
    if not (isinstance(target, torch.Tensor) and target.is_cuda and target.is_contiguous() and target.shape == probs.shape
            and target.dtype in (torch.float32, torch.uint8, torch.bool)):
        raise _lib.HotpathError(f"box_loss: target must be a contiguous fp32 / uint8 / bool device tensor of shape {tuple(probs.shape)}, got "
                                f"{getattr(target, 'dtype', type(target))} {tuple(getattr(target, 'shape', ()))}")
    if pos_weight is None:
        pos_weight = 1.0
    elif isinstance(pos_weight, str):
        if pos_weight != "auto":
            raise _lib.HotpathError(f"box_loss: pos_weight must be None, a positive number or 'auto', got {pos_weight!r}")
        pos_weight = POS_WEIGHT_AUTO
    elif float(pos_weight) == POS_WEIGHT_AUTO:
        raise _lib.HotpathError("box_loss: pos_weight must be positive (the per-sample weight is asked for as 'auto')")
    return target, 0 if target.dtype == torch.float32 else 1, float(pos_weight)      # DD_TARGET_F32 / DD_TARGET_U8


def box_loss_fwd(probs, target, pos_weight=None, bce_weight=1.0, ts_weight=0.0, ts_eps=1.0):
    """dd_box_loss_fwd outside autograd -> (losses fp32 [3] = {L, L_bce, L_ts}, stats fp64 [B,5] = {T, S, I, A, C} per sample, coef fp32
    [B,4]: the gradient coefficients ``box_loss_bwd`` takes).  One pass over the data for any weight; validation stops here."""
    target, kind, pw = _box_loss_operands(probs, target, pos_weight)
    b, per = probs.shape
    losses = torch.empty(3, device=probs.device, dtype=torch.float32)
    stats = torch.empty((b, 5), device=probs.device, dtype=torch.float64)
    coef = torch.empty((b, 4), device=probs.device, dtype=torch.float32)
    ws = torch.empty(size("dd_box_loss_workspace_bytes", b), device=probs.device, dtype=torch.uint8)
    call("dd_box_loss_fwd", probs, target, kind, b, per, pw, float(bce_weight), float(ts_weight), float(ts_eps), losses, stats, coef, ws)
    return losses, stats, coef


def box_loss_bwd(probs, target, coef, grad_scale=1.0):
    """dd_box_loss_bwd: d(loss)/d(probs) * grad_scale from the coefficients of ``box_loss_fwd`` on the same operands."""
    target, kind, _ = _box_loss_operands(probs, target, None)
    b, per = probs.shape
    _dev(coef, "coef", (b, 4))
    dprobs = torch.empty_like(probs)
    call("dd_box_loss_bwd", probs, target, kind, b, per, coef, float(grad_scale), dprobs)
    return dprobs


class BoxLoss(torch.autograd.Function):
    """Weighted BCE + soft threat score on probabilities (dd_box_loss_fwd / dd_box_loss_bwd; formulas in include/dd_hotpath.h) ->
    (loss, L_bce, L_ts), the two components without a gradient.  The gradient is written with the forward, as the other losses do."""

    @staticmethod
    def forward(ctx, probs, target, pos_weight, bce_weight, ts_weight, ts_eps):
        losses, _, coef = box_loss_fwd(probs, target, pos_weight, bce_weight, ts_weight, ts_eps)
        ctx.save_for_backward(box_loss_bwd(probs, target, coef) if ctx.needs_input_grad[0] else None)
        loss, bce, ts = losses.unbind(0)
        ctx.mark_non_differentiable(bce, ts)
        ctx.set_materialize_grads(False)
        return loss, bce, ts

    @staticmethod
    def backward(ctx, g, _gb, _gt):
        (dp,) = ctx.saved_tensors
        if g is None or dp is None:
            return (None,) * 6
        return (_scaled_loss_grad(ctx, dp, g),) + (None,) * 5


def box_loss(probs, target, pos_weight=None, bce_weight=1.0, ts_weight=0.0, ts_eps=1.0, return_parts=False):
    """The class-balanced box-map loss ``bce_weight * L_bce + ts_weight * L_ts`` of probabilities ``probs`` [B, P] against ``target``
    [B, P] (fp32 in [0,1], uint8 or bool): the 0-dim loss, differentiable in ``probs``.
      * L_bce: mean binary cross-entropy with the positive elements weighted by ``pos_weight``: None (1), a positive number, or "auto" =
        each sample's own (P - T_b) / max(T_b, 1), a constant of the step;
      * L_ts: mean over the samples of 1 - (I_b + ts_eps) / (U_b + ts_eps), the soft threat score.
    ``return_parts=True``: (loss, L_bce, L_ts), the components detached 0-dim tensors for logging."""
    loss, bce, ts = BoxLoss.apply(probs, target, pos_weight, bce_weight, ts_weight, ts_eps)
    return (loss, bce, ts) if return_parts else loss


def sigmoid(z):
    """sigmoid(logits) outside autograd (the reference's second forward output, roadmap_bce_v2.py:81)."""
    _dev(z, "z")
    if z.numel() % 4:
        raise _lib.HotpathError("sigmoid: element count must be a multiple of 4")
    p = torch.empty_like(z)
    call("dd_sigmoid", z, p, z.numel())
    return p


class Sigmoid(torch.autograd.Function):
    """p = sigmoid(z) with its autograd on the device (dd_sigmoid / dd_sigmoid_bwd): the sigmoid INSIDE ``RoadMap.forward``
    of the MSE twin (roadmap_pretrain_ae.py:76), whose loss is taken from the probabilities."""

    @staticmethod
    def forward(ctx, z):
        p = sigmoid(z.contiguous())
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, dp):
        (p,) = ctx.saved_tensors
        dp = dp.contiguous()
        _dev(dp, "dp", p.shape)
        dz = torch.empty_like(p)
        call("dd_sigmoid_bwd", dp, p, dz, p.numel())
        return dz


def sigmoid_and_loss(logits, target):
    """One pass: (loss, probs) without autograd -- used by validation."""
    n = logits.numel()
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    probs = torch.empty_like(logits)
    call("dd_bce_logits", logits, target, loss, None, probs, n, 1.0, _loss_ws(n, logits.device))
    return loss, probs


# ------------------------------------------------------------------------------------------------ optimizer
def _scale_arg(grad_scale):
    """(by value, device pointer) of an optimizer shim's ``grad_scale``: a Python number goes to the host-scalar entry point, a one-element
    fp32 device tensor (what ``clip_scale`` wrote) to the ``_dev`` one, which reads it when the kernel starts."""
    if isinstance(grad_scale, torch.Tensor):
        if not (grad_scale.is_cuda and grad_scale.dtype == torch.float32 and grad_scale.numel() == 1):
            raise _lib.HotpathError("grad_scale: a tensor must be one fp32 element on the device")
        return None, grad_scale
    return float(grad_scale), None


def _adam_table(tensors):
    table = (_lib.AdamTensor * len(tensors))()
    for i, quad in enumerate(tensors):
        for name, t in zip("pgmv", quad):
            _dev(t, name, quad[0].shape)
        table[i] = _lib.AdamTensor(_p(quad[0]), _p(quad[1]), _p(quad[2]), _p(quad[3]), quad[0].numel())
    return table


def adam_step_multi(tensors, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """One launch for a list of small (p, g, m, v) quadruples that share ``step`` (dd_adam_step_multi; ``grad_scale`` a device tensor:
    dd_adam_step_multi_dev)."""
    if not tensors:
        return
    table = _adam_table(tensors)
    scale, scale_dev = _scale_arg(grad_scale)
    if scale_dev is not None:
        call("dd_adam_step_multi_dev", table, len(tensors), lr, beta1, beta2, eps, int(step), scale_dev)
        return
    call("dd_adam_step_multi", table, len(tensors), lr, beta1, beta2, eps, int(step), scale)


def adam_step_rankb(p, m, v, dy, x, bias, bias_m, bias_v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """Adam on the Linear weight ``p`` [n, k] (moments ``m``, ``v``) with its gradient dy^T x formed inside the pass from the layer's
    output gradient ``dy`` [rows, n] and input ``x`` [rows, k]; ``bias`` (optional, with its moments) is updated from dy's column sums
    in the same launch (dd_adam_step_rankb; ``grad_scale`` a device tensor: dd_adam_step_rankb_dev)."""
    rows, n = dy.shape
    k = x.shape[1]
    _dev(dy, "dy")
    _dev(x, "x", (rows, k))
    for name, t in (("p", p), ("m", m), ("v", v)):
        _dev(t, name, (n, k))
    if bias is not None:
        for name, t in (("bias", bias), ("bias_m", bias_m), ("bias_v", bias_v)):
            _dev(t, name, (n,))
    scale, scale_dev = _scale_arg(grad_scale)
    if scale_dev is not None:
        call("dd_adam_step_rankb_dev", p, m, v, dy, x, rows, n, k, bias, bias_m, bias_v, lr, beta1, beta2, eps, int(step), scale_dev)
        return
    call("dd_adam_step_rankb", p, m, v, dy, x, rows, n, k, bias, bias_m, bias_v, lr, beta1, beta2, eps, int(step), scale)


def adam_step_flat(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _dev(t, name, p.shape)
    scale, scale_dev = _scale_arg(grad_scale)
    if scale_dev is not None:
        call("dd_adam_step_dev", p, g, m, v, p.numel(), lr, beta1, beta2, eps, int(step), scale_dev)
        return
    call("dd_adam_step", p, g, m, v, p.numel(), lr, beta1, beta2, eps, int(step), scale)


# ------------------------------------------------------------------------------------------------ gradient norm (clipping)
_NORM_WS = {}      # device -> persistent workspace of the norm kernels (grown, never shrunk: no allocation in a steady step)


def _norm_ws(nbytes, device):
    """The norm kernels run one after the other on the optimizer's stream, each done with its partials when its own last stage has
    run: one workspace per device serves them all."""
    ws = _NORM_WS.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _NORM_WS[device] = torch.empty(max(int(nbytes), 1 << 16), device=device, dtype=torch.uint8)
    return ws


def _slot(out):
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.numel() == 1):
        raise _lib.HotpathError("out: expected one fp64 element on the device")
    return out


def sqnorm(g, out):
    """``out`` (one fp64 device element) = sum of squares of the flat fp32 device tensor ``g``, accumulated in fp64 (dd_sqnorm)."""
    _dev(g, "g")
    nbytes = size("dd_sqnorm_workspace_bytes", g.numel())
    ws = _norm_ws(nbytes, g.device)
    call("dd_sqnorm", g, g.numel(), _slot(out), ws, ws.numel())
    return out


def sqnorm_multi(grads, out):
    """The same over a list of (small) fp32 device tensors: one launch per 48 of them (dd_sqnorm_multi)."""
    if not grads:
        raise _lib.HotpathError("sqnorm_multi: no tensors")
    table = (_lib.AdamTensor * len(grads))()
    for i, g in enumerate(grads):
        _dev(g, "g")
        table[i] = _lib.AdamTensor(None, _p(g), None, None, g.numel())
    nbytes = size("dd_sqnorm_multi_workspace_bytes", table, len(grads))
    ws = _norm_ws(nbytes, grads[0].device)
    call("dd_sqnorm_multi", table, len(grads), _slot(out), ws, ws.numel())
    return out


def rankb_sqnorm(dy, x, with_bias, out):
    """``out`` = ||dy^T x||_F^2 (+ ||dy.sum(0)||^2 with ``with_bias``) from the factors of a Linear layer, in fp64, without forming the
    weight gradient (dd_rankb_sqnorm)."""
    rows, n = dy.shape
    k = x.shape[1]
    _dev(dy, "dy")
    _dev(x, "x", (rows, k))
    nbytes = size("dd_rankb_sqnorm_workspace_bytes", rows, n, k)
    ws = _norm_ws(nbytes, dy.device)
    call("dd_rankb_sqnorm", dy, x, rows, n, k, 1 if with_bias else 0, _slot(out), ws, ws.numel())
    return out


def clip_scale(sq, max_norm, grad_scale, out3):
    """``out3`` (3 fp32 device elements) = {grad_scale * coef, norm, coef} from the fp64 squared norms ``sq`` (dd_clip_scale)."""
    if not (isinstance(sq, torch.Tensor) and sq.is_cuda and sq.dtype == torch.float64 and sq.is_contiguous() and sq.numel() > 0):
        raise _lib.HotpathError("sq: expected a contiguous fp64 device tensor")
    _dev(out3, "out3", (3,))
    call("dd_clip_scale", sq, sq.numel(), float(max_norm), float(grad_scale), out3)
    return out3
