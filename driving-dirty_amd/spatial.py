"""Spatial bounding-box heads on the HIP hot path: ``SpatialMappingCNN``, ``RoadMapBoxesMergingCNN``,
``BoxesMergingCNN`` (reference src/bounding_box_model/spatial_bb/components.py) and the ``BBSpatialRoadMap``
LightningModule (reference spatial_bb/spatial_w_rm.py, registry name ``spatial_rm``).  Same constructors,
parameter names, construction order (default init parity) and ``forward`` signatures; the modules only hold
parameters, the arithmetic is ``heads.SpatialMapFn`` / ``heads.MergeFn``.
"""
import warnings
from argparse import ArgumentParser

import torch
from torch import nn

from . import gconv, ops
from . import tta as _tta
from .augment import Augmenter, add_augment_args, current_rank
from .adamw import add_weight_decay_args
from .ema import add_ema_args
from .autoencoder import BasicAE
from .heads import MergeFn, SpatialMapFn, _ORDER, as_nhwc, road_map_taps
from .lightning import LightningModule, hparam, pretrained_ae
from .roadmap import eval_no_grad


def _gpu(t, who):
    if not t.is_cuda:
        raise RuntimeError(f"{who}: the hot path runs on MI355X only (got a {t.device} tensor)")


class SpatialMappingCNN(nn.Module):
    def __init__(self):
        super().__init__()
        self.f_conv = nn.Conv2d(3, 32, kernel_size=(52, 1), stride=(3, 2), padding=(1))
        self.fl_conv = nn.Conv2d(3, 32, kernel_size=(1, 50), stride=(3, 2))
        self.fr_conv = nn.Conv2d(3, 32, kernel_size=(1, 50), stride=(3, 2))
        self.b_conv = nn.Conv2d(3, 32, kernel_size=(52, 1), stride=(3, 2), padding=(1))
        self.bl_conv = nn.Conv2d(3, 32, kernel_size=(1, 50), stride=(3, 2))
        self.br_conv = nn.Conv2d(3, 32, kernel_size=(1, 50), stride=(3, 2))
        self.out_conv = nn.Conv2d(32, 32, kernel_size=(3, 3))

    def forward(self, x):
        """(b, 6, 3, 256, 306) -- or the collate's tuple of b [6,3,256,306] tensors, read through a pointer table instead of being
        stacked first (spatial_w_rm.py:100-103) -- -> (b, 32, 256, 256), returned as an NCHW-shaped view of the NHWC result."""
        per_sample = isinstance(x, (tuple, list))
        _gpu(x[0] if per_sample else x, "SpatialMappingCNN")
        params = []
        for n in _ORDER:
            m = getattr(self, n)
            params += [m.weight, m.bias]
        # uint8 frames ([b,6,256,306,3] or a tuple of [6,256,306,3]) are read as they are: ToTensor's /255 happens in the re-layout
        views = tuple(t.contiguous() for t in x) if per_sample else x.contiguous()
        return SpatialMapFn.apply(views, *params).permute(0, 3, 1, 2)


class _Merging(nn.Module):
    with_rm = False
    # "fp32": the reference's arithmetic on the exact-fp32 matrix kernels.  "fp32x3": the dilated up-convs take every fp32 product as six
    # bf16 x bf16 products of three-way split operands (csrc/dconv_split.hip; same 2e-5-of-peak bound against fp64 as the exact kernels in
    # the tests, error model in DESIGN.md 3.3d; 59 -> 43 ms per config-3 step).  None: the process-wide default (gconv.SPLIT_BF16).
    precision = None

    def _params(self, names):
        out = []
        for n in names:
            m = getattr(self, n)
            out += [m.weight, m.bias]
        return out

    def _run(self, ssr, spatial_map, rm):
        _gpu(ssr, type(self).__name__)
        names = ["ss_conv", "ss_deconv"] + (["rm_conv_1", "rm_conv_2"] if self.with_rm else []) + self.up_names
        rm4 = road_map_taps(rm) if self.with_rm else None
        if self.precision not in (None, "fp32", "fp32x3"):
            raise ValueError(f"{type(self).__name__}.precision must be 'fp32' or 'fp32x3', got {self.precision!r}")
        with gconv.split_products(None if self.precision is None else self.precision == "fp32x3"):
            probs = MergeFn.apply(as_nhwc(ssr, 32), as_nhwc(spatial_map, 32), rm4, self.with_rm, *self._params(names))
        return probs.unsqueeze(1)                        # [B,1,800,800] like the reference


class BoxesMergingCNN(_Merging):
    up_names = ["up_conv_1", "up_conv_2", "up_conv_3", "up_conv_4"]

    def __init__(self):
        super().__init__()
        self.ss_conv = nn.Conv2d(32, 32, kernel_size=(1, 24), stride=(1, 7))
        self.ss_deconv = nn.ConvTranspose2d(32, 32, kernel_size=2, stride=2)
        self.up_conv_1 = nn.ConvTranspose2d(64, 32, kernel_size=8, stride=1, dilation=8)
        self.up_conv_2 = nn.ConvTranspose2d(32, 16, kernel_size=8, stride=1, dilation=8)
        self.up_conv_3 = nn.ConvTranspose2d(16, 8, kernel_size=6, stride=1, dilation=6, output_padding=2)
        self.up_conv_4 = nn.ConvTranspose2d(8, 1, kernel_size=2, stride=2)

    def forward(self, ssr, spatial_map):
        return self._run(ssr, spatial_map, None)


class RoadMapBoxesMergingCNN(_Merging):
    with_rm = True
    up_names = ["up_conv_1", "up_conv_2", "up_conv_3", "up_conv_4", "up_conv_5"]

    def __init__(self):
        super().__init__()
        self.ss_conv = nn.Conv2d(32, 32, kernel_size=(1, 24), stride=(1, 7))
        self.ss_deconv = nn.ConvTranspose2d(32, 32, kernel_size=2, stride=2)
        self.rm_conv_1 = nn.Conv2d(1, 32, kernel_size=7, stride=3, dilation=3, padding=1)
        self.rm_conv_2 = nn.Conv2d(32, 32, kernel_size=3, stride=1, dilation=3)
        self.up_conv_1 = nn.ConvTranspose2d(96, 64, kernel_size=7, stride=1, dilation=7)
        self.up_conv_2 = nn.ConvTranspose2d(64, 32, kernel_size=7, stride=1, dilation=7)
        self.up_conv_3 = nn.ConvTranspose2d(32, 16, kernel_size=7, stride=1, dilation=7)
        self.up_conv_4 = nn.ConvTranspose2d(16, 8, kernel_size=7, stride=1, dilation=3)
        self.up_conv_5 = nn.ConvTranspose2d(8, 1, kernel_size=2, stride=2)

    def forward(self, ssr, spatial_map, rm):
        return self._run(ssr, spatial_map, rm)


def per_sample_inputs(sample, road_image):
    """True when the collate's tuples (helper.py:22-23) can be read where they lie: fp32 [6,3,H,W] views and bool / uint8 road
    masks, contiguous, on the GPU, at most 64 x k samples of one size."""
    if not (isinstance(sample, (tuple, list)) and isinstance(road_image, (tuple, list)) and 0 < len(sample) == len(road_image)):
        return False
    shape = tuple(sample[0].shape)
    dtype = sample[0].dtype                                   # fp32 [6,3,H,W] views or uint8 [6,H,W,3] decoded frames
    return (dtype in (torch.float32, torch.uint8) and
            all(t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.dim() == 4 for t in sample)
            and all(t.is_cuda and t.is_contiguous() and t.dtype in (torch.bool, torch.uint8) and t.dim() == 2 for t in road_image))


def bb_coord_to_map(target, device=None, rasterizer=None):
    """Targets -> [b,800,800] maps: pre-rasterised ``'bb_map'`` entries are taken as they are, a caller-supplied
    ``rasterizer`` is honoured, everything else goes through the HIP rasteriser in one launch."""
    if all("bb_map" in t for t in target):
        return torch.stack([t["bb_map"] for t in target], dim=0)
    if rasterizer is not None:
        return torch.stack([torch.as_tensor(rasterizer(t["bounding_box"])) for t in target], dim=0)
    return ops.boxes_to_binary_map([t["bounding_box"] for t in target], device)


def box_loss_config(hparams):
    """The class-balanced box-map loss as the hparams ask for it: None when it is off (``box_pos_weight`` None, ``box_ts_weight`` 0,
    ``box_bce_weight`` 1: the reference's loss, spatial_w_rm.py:128-131), else the keyword arguments of ``ops.box_loss``.
    ``box_pos_weight``: None, a positive number (or a string that parses as one), or "auto" = each sample's own negatives / positives.
    A value the kernels would refuse, or the loss together with ``mse_loss``, raises ValueError here, when the module is built."""
    pos_weight = hparam(hparams, "box_pos_weight", None)
    if isinstance(pos_weight, str) and pos_weight != "auto":
        try:
            pos_weight = float(pos_weight)
        except ValueError:
            raise ValueError(f"box_pos_weight must be a positive number or 'auto', got {pos_weight!r}") from None
    if pos_weight is not None and pos_weight != "auto":
        if isinstance(pos_weight, bool) or not isinstance(pos_weight, (int, float)) or not 0 < pos_weight < float("inf"):
            raise ValueError(f"box_pos_weight must be a positive number or 'auto', got {pos_weight!r}")
        pos_weight = float(pos_weight)
    weights = {}
    for name, default in (("box_bce_weight", 1.0), ("box_ts_weight", 0.0), ("box_ts_eps", 1.0)):
        try:
            weights[name] = float(hparam(hparams, name, default))
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number, got {hparam(hparams, name, default)!r}") from None
        if not 0 <= weights[name] < float("inf"):
            raise ValueError(f"{name} must be a finite number >= 0, got {weights[name]!r}")
    if pos_weight is None and weights["box_ts_weight"] == 0 and weights["box_bce_weight"] == 1:
        return None
    if hparam(hparams, "mse_loss", False):
        raise ValueError("box_pos_weight / box_bce_weight / box_ts_weight select a loss on probabilities and cannot be combined with mse_loss")
    if weights["box_bce_weight"] == 0 and weights["box_ts_weight"] == 0:
        raise ValueError("box_bce_weight and box_ts_weight are both 0: the loss would be constant")
    return {"pos_weight": pos_weight, "bce_weight": weights["box_bce_weight"], "ts_weight": weights["box_ts_weight"], "ts_eps": weights["box_ts_eps"]}


def compute_ats_bounding_boxes(boxes1, boxes2):
    """helper.py:33-72 for one sample, on the device: [n1,2,4] and [n2,2,4] corner tensors -> 0-dim average threat score
    (``iou_max`` over ``boxes1`` for each box of ``boxes2``).  An empty set scores 0 where the reference raises."""
    return ops.ats_bounding_boxes([boxes1], [boxes2])[0]


def boxes_from_map(maps, threshold=0.5, min_pixels=1, max_boxes=256, fit="extent", pad_px=0.5, split_px=0, grow_iters=None, warn_overflow=True):
    """[b,H,W] occupancy maps -> tuple of b [n_i,2,4] box tensors (``ops.component_boxes`` cut to each sample's count).
    ``fit="oriented"`` fits each component along its principal axis instead of taking its axis-aligned extent.  ``split_px > 0`` first
    splits blobs joined through a neck narrower than ``2 * split_px + 1`` pixels (``ops.split_components``; ``grow_iters=None`` =
    ``2 * split_px``).  ``warn_overflow=False``: a sample with more than ``max_boxes`` components is cut there without a warning (the
    threshold sweep: at a low threshold on a noisy map that is the normal case)."""
    boxes, counts = ops.component_boxes(maps.detach().float().contiguous(), threshold, min_pixels, max_boxes, fit=fit, pad_px=pad_px,
                                        split_px=split_px, grow_iters=grow_iters)
    counts = counts.tolist()
    over = [i for i, c in enumerate(counts) if c > max_boxes]
    if over and warn_overflow:
        warnings.warn(f"boxes_from_map: samples {over} have more than max_boxes={max_boxes} components "
                      f"({[counts[i] for i in over]}); only the first {max_boxes} are returned")
    return tuple(boxes[i, :min(c, max_boxes)] for i, c in enumerate(counts))


def require_bounding_boxes(targets):
    """``box_metrics`` scores boxes against boxes: every target must hold its ``'bounding_box'`` tensor."""
    missing = [i for i, t in enumerate(targets) if "bounding_box" not in t]
    if missing:
        raise KeyError(f"box_metrics needs a 'bounding_box' tensor in every target (missing in samples {missing})")


BOX_THRESHOLD_GRID = tuple(k / 16 for k in range(1, 16))      # the default candidates of the box threshold: exact in fp32, 0.5 among them


def box_threshold_grid(hparams):
    """``hparams.box_threshold_grid`` as a tuple of floats (default ``BOX_THRESHOLD_GRID``): the thresholds ``box_ats_sweep`` decodes at.
    Strictly increasing numbers inside (0, 1), at least one; anything else raises ValueError (when the module is built)."""
    grid = hparam(hparams, "box_threshold_grid", None)
    if grid is None:
        return BOX_THRESHOLD_GRID
    if not isinstance(grid, (list, tuple)) or len(grid) == 0:
        raise ValueError(f"box_threshold_grid must be a non-empty list of thresholds, got {grid!r}")
    if any(isinstance(t, bool) or not isinstance(t, (int, float)) or not 0.0 < t < 1.0 for t in grid):
        raise ValueError(f"box_threshold_grid: every threshold must be a number inside (0, 1), got {grid!r}")
    grid = tuple(float(t) for t in grid)
    if any(a >= b for a, b in zip(grid, grid[1:])):
        raise ValueError(f"box_threshold_grid must be strictly increasing, got {grid!r}")
    return grid


def box_min_pixels(hparams):
    """``hparams.box_min_pixels``: the smallest component the decode keeps (speckle removal), a whole number >= 1, default 1."""
    n = hparam(hparams, "box_min_pixels", None)
    if n is None:
        return 1
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"box_min_pixels must be a whole number >= 1, got {n!r}")
    return n


class _ShownDefault:
    """A default that a signature shows as the value it falls back to (``box_threshold=0.5``: what a call without the argument gets while
    nothing is calibrated) and that is told from the same number GIVEN by a caller by its type: an explicit 0.5 is a plain float and
    stays 0.5.  ``JointRoadMapBBox.predict``'s signature is pinned with these values; everywhere else "not given" is None."""
    __slots__ = ()


class _ShownFloat(_ShownDefault, float):
    __slots__ = ()


class _ShownInt(_ShownDefault, int):
    __slots__ = ()


HALF_UNLESS_CALIBRATED = _ShownFloat(0.5)      # JointRoadMapBBox.predict's box_threshold default
ONE_UNLESS_CONFIGURED = _ShownInt(1)           # ... and its min_pixels default


def box_decode_point(hparams, threshold=None, min_pixels=None):
    """The operating point of a box decode -> (threshold, min_pixels).  THE ORDER, stated once: an explicit argument wins; an argument left
    out (None, or one of the two shown defaults above) means the calibrated ``hparams.box_threshold`` where there is one, else 0.5, and
    ``hparams.box_min_pixels``, else 1."""
    if threshold is None or isinstance(threshold, _ShownDefault):
        threshold = hparam(hparams, "box_threshold", None)
    if min_pixels is None or isinstance(min_pixels, _ShownDefault):
        min_pixels = hparam(hparams, "box_min_pixels", None)
    return 0.5 if threshold is None else float(threshold), 1 if min_pixels is None else int(min_pixels)


def _decode_args(hparams):
    return dict(fit=hparam(hparams, "box_fit", "extent"), pad_px=hparam(hparams, "box_pad_px", 0.5),
                split_px=hparam(hparams, "box_split_px", 0), grow_iters=hparam(hparams, "box_grow_iters", None))


def decoded_box_ats(hparams, pred_maps, targets):
    """The task's own unit for one batch: boxes extracted from the predicted maps [b,800,800] as ``hparams`` ask (``box_fit``,
    ``box_pad_px``, ``box_split_px``, ``box_grow_iters``, ``box_min_pixels``; cut at the calibrated ``box_threshold`` when one is set,
    else at 0.5) against the targets' boxes -> the batch's mean average threat score, 0-dim."""
    threshold, min_pixels = box_decode_point(hparams)
    fitted = boxes_from_map(pred_maps, threshold, min_pixels, **_decode_args(hparams))
    return ops.ats_bounding_boxes(fitted, [t["bounding_box"] for t in targets]).mean()


def box_ats_sweep(hparams, pred_maps, targets, thresholds):
    """``decoded_box_ats`` at every threshold of ``thresholds`` -> (sums fp64 [K] on the maps' device, the sample count b): sums[k] is the
    SUM over the batch's samples of the per-sample average threat score of the map decoded at thresholds[k], so sums[k] / b is
    ``decoded_box_ats`` with ``hparams.box_threshold = thresholds[k]``.  The same kernels with the same arguments and the same rule (a
    pixel is in where ``map > t``, strictly, t rounded to fp32), one decode per threshold: the box score is no function of per-pixel
    counts, so no histogram holds it (the road map's does, ``ops.ts_histogram``).  Sums, not means: batches of different sizes add up
    to the data set's mean.  A threshold at which a sample has more than 256 components scores what its first 256 boxes score, quietly."""
    _, min_pixels = box_decode_point(hparams)
    maps = pred_maps.detach().float().contiguous()
    boxes = [t["bounding_box"] for t in targets]
    sums = [ops.ats_bounding_boxes(boxes_from_map(maps, t, min_pixels, warn_overflow=False, **_decode_args(hparams)), boxes).double().sum()
            for t in thresholds]
    return torch.stack(sums), len(boxes)


def best_box_threshold(sums, count, thresholds):
    """Summed sweeps -> (k, curve): curve[k] = sums[k] / count in fp64 (the data set's mean score at thresholds[k]; on the CPU), k its
    maximum.  Ties go to the threshold nearest 0.5, then to the lower one, as ``ops.ts_curve`` breaks them.  Plain torch on K numbers."""
    count = int(count)
    if count <= 0:
        raise ValueError(f"best_box_threshold: no samples were swept (count = {count})")
    sums = torch.as_tensor(sums).detach().to("cpu", torch.float64).reshape(-1)
    if sums.numel() != len(thresholds) or sums.numel() == 0:
        raise ValueError(f"best_box_threshold: {sums.numel()} sums for {len(thresholds)} thresholds")
    curve = sums / count
    ties = [k for k in range(curve.numel()) if curve[k] == curve.max()]
    if not ties:
        raise ValueError(f"best_box_threshold: the curve has no maximum ({curve.tolist()})")
    return min(ties, key=lambda k: (abs(float(thresholds[k]) - 0.5), k)), curve


class CalibratedBoxThreshold:
    """What a module with a box head needs to calibrate the threshold its map is decoded at on validation data
    (hparams.calibrate_box_threshold) and to carry it: the ``box_threshold`` property, the per-batch sweep and the epoch's argmax.  Shared
    by ``BBSpatialRoadMap`` and the joint model; the sibling of ``roadmap.CalibratedThreshold``.  Per process, like ``rm_threshold``:
    nothing is reduced across data-parallel ranks."""

    BOX_SWEEP = "box_ats_sweep"      # validation_step's key: fp64 [K + 1], the sweep's K sums and then the sample count

    @property
    def box_threshold(self):
        """The threshold ``validation_epoch_end`` / ``calibrate_boxes`` calibrated, a plain float, or None.  Kept in ``hparams`` -- not a
        buffer, not in the state_dict -- so ``save_checkpoint`` / ``load_from_checkpoint`` carry it, as they do ``rm_threshold``."""
        return hparam(self.hparams, "box_threshold", None)

    @box_threshold.setter
    def box_threshold(self, value):
        self.hparams.box_threshold = None if value is None else float(value)

    def _check_box_decode(self):
        """A bad ``box_threshold_grid`` or ``box_min_pixels`` fails when the module is built, not in the first validation step."""
        box_threshold_grid(self.hparams)
        box_min_pixels(self.hparams)

    def _wants_box_sweep(self):
        return bool(hparam(getattr(self, "hparams", None), "calibrate_box_threshold", False))      # off for a module without hparams

    def _with_box_sweep(self, out, pred_maps, targets):
        """``out[BOX_SWEEP]`` <- this batch's sweep of ``pred_maps`` [b,800,800], whether or not the hparams ask for one."""
        sums, count = box_ats_sweep(self.hparams, pred_maps, targets, box_threshold_grid(self.hparams))
        out[self.BOX_SWEEP] = torch.cat([sums, sums.new_tensor([count])])
        return out

    def _calibrate_boxes(self, outputs, logs):
        """``box_threshold`` <- the grid's threshold with the best mean score of the DATA SET (the batches' summed sweeps over the number
        of samples: a ragged last batch counts as what it is; the ``avg_*`` values are means of batch means), and its figures into
        ``logs``.  -> the curve."""
        grid = box_threshold_grid(self.hparams)
        total = torch.stack([x[self.BOX_SWEEP] for x in outputs]).sum(0).cpu()
        best, curve = best_box_threshold(total[:-1], round(float(total[-1])), grid)
        self.box_threshold = grid[best]
        logs.update(best_box_threshold=self.box_threshold, best_val_ats=float(curve[best]))
        if 0.5 in grid:
            logs["val_ats_at_half"] = float(curve[grid.index(0.5)])
        return curve

    def _box_sweep_of(self, batch):
        """One validation batch -> its sweep as ``{BOX_SWEEP: ...}``: the forward pass and the sweep, nothing else (each module's own)."""
        raise NotImplementedError

    def calibrate_boxes(self, batches):
        """Calibrate a module that was trained without ``--calibrate_box_threshold``: the forward pass and the sweep over an iterable of
        validation batches, in ``eval()`` mode under ``no_grad`` (every submodule's mode is put back), then what
        ``validation_epoch_end`` does with an epoch's sweeps.  Sets ``box_threshold``; -> (threshold, curve fp64 [K])."""
        with eval_no_grad(self):
            outputs = [self._box_sweep_of(batch) for batch in batches]
        curve = self._calibrate_boxes(outputs, {})
        return self.box_threshold, curve


def mean_logs(outputs, keys):
    """{'avg_' + k: mean over the epoch's outputs} for every k of ``keys`` that all outputs hold."""
    return {"avg_" + k: torch.stack([x[k] for x in outputs]).mean() for k in keys if outputs and all(k in x for x in outputs)}


def add_box_args(p):
    """The command-line flags of box validation and of the box-map loss, shared by every module with a box head."""
    p.add_argument("--box_metrics", action="store_true",
                   help="validation also extracts boxes from the predicted map and reports val_ats (average threat score against the "
                        "targets' boxes) and val_ts (map-level threat score)")
    p.add_argument("--box_fit", type=str, default="extent", choices=("extent", "oriented"),
                   help="how box_metrics fits a box to a component of the predicted map: its axis-aligned extent, or the rectangle "
                        "along its principal axis (the data set's boxes are rotated)")
    p.add_argument("--box_pad_px", type=float, default=0.5,
                   help="oriented fit: pixels added on each side of the pixel centres' extents (0.5 = the pixel squares, 0 = the centres)")
    p.add_argument("--box_split_px", type=int, default=0,
                   help="box_metrics: split blobs joined through a neck narrower than 2 * box_split_px + 1 pixels before fitting "
                        "(touching cars); 0 = off, at most 8")
    p.add_argument("--box_grow_iters", type=int, default=None,
                   help="box_metrics with --box_split_px: rounds the eroded cores grow back inside the map (default 2 * box_split_px, at most 16)")
    p.add_argument("--box_pos_weight", type=str, default=None,
                   help="box-map loss: weight of the positive (car) elements in the BCE: a positive number, or 'auto' = each sample's own "
                        "negatives / positives; default: unweighted (the reference's loss)")
    p.add_argument("--box_bce_weight", type=float, default=1.0, help="box-map loss: factor of the (weighted) BCE term")
    p.add_argument("--box_ts_weight", type=float, default=0.0,
                   help="box-map loss: factor of the soft threat-score term 1 - (I + eps) / (U + eps), per sample; 0 = off")
    p.add_argument("--box_ts_eps", type=float, default=1.0, help="box-map loss: eps of the soft threat score (>= 0)")
    p.add_argument("--calibrate_box_threshold", action="store_true",
                   help="validation also decodes the predicted box map at every threshold of a grid (1/16 .. 15/16) and keeps the one with "
                        "the best data-set average threat score (box_threshold): val_ats and the predictions then decode there")
    p.add_argument("--box_min_pixels", type=int, default=1,
                   help="box decoding (validation, the threshold sweep, predictions): components of fewer pixels are dropped; >= 1")


class BBSpatialRoadMap(CalibratedBoxThreshold, LightningModule):
    """spatial_w_rm.py:25-167.  ``bb_coord_to_map`` (the per-sample PIL polygon loop of src/utils/bb_to_img.py) runs
    as one launch of the HIP rasteriser over the batch's ``'bounding_box'`` tensors; batches may instead carry a
    pre-rasterised ``'bb_map'`` [800,800] tensor in each target dict, or name their own ``hparams.rasterizer``."""

    box_loss = None      # box_loss_config(hparams): None = the reference's loss

    def __init__(self, hparams):
        super().__init__()
        self.hparams = hparams
        self.output_dim = 800 * 800
        self.ae = pretrained_ae(hparams)
        self.frozen = True
        self.ae.freeze()
        self.ae.encoder.c3_only = True
        self.ae.decoder = None
        # hparams.precision = "bf16": the (frozen or fine-tuned) encoder conv stack on the bf16 matrix cores, its feature handed to
        # the fp32 heads (no reference counterpart: oracle/bf16_parts.py states the contract).  "fp32x3": everything fp32, the box
        # head's dilated up-convs by split products on the bf16 pipe (_Merging.precision).  Default "fp32": the reference's arithmetic.
        precision = str(hparam(hparams, "precision", self.ae.encoder.precision))
        if precision not in ("fp32", "bf16", "fp32x3"):
            raise ValueError(f"precision must be 'fp32', 'bf16' or 'fp32x3', got {precision!r}")
        self.ae.encoder.precision = "bf16" if precision == "bf16" else "fp32"
        self.space_map_cnn = SpatialMappingCNN()
        self.box_merge = RoadMapBoxesMergingCNN()
        if hparam(hparams, "precision", None) is not None:
            self.box_merge.precision = "fp32x3" if precision == "fp32x3" else "fp32"
        self.box_loss = box_loss_config(hparams)      # None: the reference's loss; a bad value fails here, not in the first step
        self._check_box_decode()
        self.augment = Augmenter(hparams, rank=current_rank())      # train-time only; off unless an aug_* hparam is set

    def wide_stitch_six_images(self, x):
        return ops.stitch6(x.contiguous(), want_nhwc4=False, want_nchw=True)[1]

    def forward(self, x, rm):
        """x [b,6,3,256,306], rm [b,1,800,800] -> [b,800,800].  spatial_w_rm.py:67-83.  Both may also be the collate's tuples
        (b x [6,3,256,306] views, b x bool [800,800] masks): the kernels then gather from the per-sample tensors."""
        space_rep = self.space_map_cnn(x)
        wide4 = ops.wide_image(x, self.ae.encoder.precision)      # fp32 views or uint8 frames, tensor or the collate's tuple
        ssr = self.ae.encoder.forward_nhwc4(wide4)
        yhat = self.box_merge(ssr, space_rep, rm)
        return yhat.squeeze(1)

    def bb_coord_to_map(self, target, device=None):
        """tuple of b target dicts -> [b,800,800].  spatial_w_rm.py:85-95."""
        return bb_coord_to_map(target, device, hparam(self.hparams, "rasterizer", None))

    def _run_step(self, batch, batch_idx, step_name):
        return self._run_step_parts(batch, batch_idx, step_name)[:3]

    @staticmethod
    def _batch_inputs(sample, road_image):
        """A batch's views and road maps -> (x, rm) as ``forward`` takes them.  The collate's tuples are read where they lie (pointer
        tables) when they can be: no torch.stack of the 180 MB of views, no stack + float() of the road masks (spatial_w_rm.py:100-105);
        else a stacked tensor of views and rm [b,1,800,800] fp32."""
        if per_sample_inputs(sample, road_image):
            return tuple(sample), tuple(road_image)
        sample = torch.stack(tuple(sample), dim=0) if isinstance(sample, (tuple, list)) else sample
        return sample, torch.stack(tuple(road_image), dim=0).float().unsqueeze(1)

    def _tta_box_map(self, x, rm, scene=None):
        """The averaged box map [b,800,800] of mirror test-time averaging (tta.py): ``self(x, rm)`` (or ``scene``, where the caller
        has it) and the same code on the mirrored scene, ``self(tta.mirror_views(x), tta.mirror_masks(rm))``, through
        ``tta.mean_prob``.  Two passes at B, not one at 2 B.  Outside autograd."""
        with torch.no_grad():
            scene = self(x, rm) if scene is None else scene
            mirrored = self(_tta.mirror_views(x), _tta.mirror_masks(rm))
            return _tta.mean_prob(scene.detach().reshape(-1, 800, 800).contiguous(), mirrored.detach().contiguous(), False)

    def _box_sweep_of(self, batch):
        sample, target, road_image = batch
        require_bounding_boxes(target)
        x, rm = self._batch_inputs(sample, road_image)
        return self._with_box_sweep({}, self(x, rm) if _tta.resolve(self, None) is None else self._tta_box_map(x, rm), target)

    def _run_step_parts(self, batch, batch_idx, step_name):
        """-> (loss, target, prediction, parts): parts is None with the reference's loss, (L_bce, L_ts) with ``box_loss_config``'s."""
        sample, target, road_image = batch
        sample, rm = self._batch_inputs(sample, road_image)
        if isinstance(sample, tuple):
            dev = sample[0].device
            target_bb_img = self.bb_coord_to_map(target, dev).to(dev).float()
        else:
            target_bb_img = self.bb_coord_to_map(target, sample.device).to(sample.device)
            target_bb_img = target_bb_img.float() if sample.dtype == torch.uint8 else target_bb_img.type_as(sample)
        pred_bb_img = self(sample, rm)
        batch_size = target_bb_img.size(0)
        target_bb_img = target_bb_img.reshape(batch_size, -1)
        pred_bb_img = pred_bb_img.reshape(batch_size, -1)
        if self.box_loss is not None:
            loss, bce, soft_ts = ops.box_loss(pred_bb_img, target_bb_img.contiguous(), return_parts=True, **self.box_loss)
            return loss, target_bb_img, pred_bb_img, (bce, soft_ts)
        if hparam(self.hparams, "mse_loss", False):
            loss = ops.MseLoss.apply(pred_bb_img, target_bb_img)
        else:
            loss = ops.BceProbs.apply(pred_bb_img, target_bb_img)
        return loss, target_bb_img, pred_bb_img, None

    def training_step(self, batch, batch_idx):
        if self.current_epoch >= self.hparams.unfreeze_epoch_no and self.frozen:
            self.frozen = False
            self.ae.unfreeze()
        batch = self.augment.apply(batch)      # a mirrored sample's target map is rasterised from its mirrored boxes
        train_loss, _, _, parts = self._run_step_parts(batch, batch_idx, step_name="train")
        log = {"train_loss": train_loss}
        if parts is not None:
            log["bbox_bce"], log["bbox_soft_ts"] = parts
        return {"loss": train_loss, "log": log}

    def predict_boxes(self, x, rm, threshold=None, min_pixels=None, max_boxes=256, fit="extent", pad_px=0.5, split_px=0, grow_iters=None,
                      tta=None):
        """Forward pass, then the predicted map's connected components as boxes (``ops.component_boxes``): a tuple of b tensors
        [n_i,2,4] in the data set's format.  ``threshold=None``: the calibrated ``box_threshold`` where there is one, else 0.5;
        ``min_pixels=None``: ``hparams.box_min_pixels``, else 1; an explicit argument wins (``box_decode_point``).  A sample with more
        than ``max_boxes`` components is cut there, with a warning.
        ``fit="oriented"``: rotated rectangles along each component's principal axis (which end is the front is arbitrary).
        ``split_px > 0``: touching cars joined through a neck are split first (``ops.split_components``).

        ``tta``: None = ``hparams.tta_mirror`` (default off), False = off, True / "mirror" = mirror test-time averaging: the map decoded
        is ``_tta_box_map(x, rm)``, the mean of the scene's map and the mirrored scene's, reflected back; that path runs in ``eval()``
        mode (every submodule's mode is put back).  The encoder's dense blocks are not part of this model's forward, so the two passes
        draw no dropout masks here; in the models that run them (the road-map head) dropout is on in eval mode too and each pass draws
        its own.  ``threshold=None`` is the one ``box_threshold`` in either mode: under ``hparams.tta_mirror`` it is calibrated on the
        averaged map, and ``tta=False`` on such a checkpoint reuses it as it is."""
        threshold, min_pixels = box_decode_point(self.hparams, threshold, min_pixels)
        if _tta.resolve(self, tta) is not None:
            with eval_no_grad(self):
                return boxes_from_map(self._tta_box_map(x, rm), threshold, min_pixels, max_boxes, fit, pad_px, split_px, grow_iters)
        with torch.no_grad():
            return boxes_from_map(self(x, rm), threshold, min_pixels, max_boxes, fit, pad_px, split_px, grow_iters)

    def validation_step(self, batch, batch_idx):
        """Under ``hparams.calibrate_box_threshold`` also ``box_ats_sweep``: the predicted map (computed with the batch's road map, as
        everything this module validates) decoded and scored at every threshold of the grid.  Under ``hparams.tta_mirror`` the sweep
        reads the averaged map (``_tta_box_map``: one more forward pass, on the mirrored batch), and ``hparams.box_metrics`` adds
        ``val_ats_tta`` / ``val_ts_tta`` from it; the other keys keep their meaning."""
        val_loss, target_bb_img, pred_bb_img, parts = self._run_step_parts(batch, batch_idx, step_name="valid")
        out = {"val_loss": val_loss}
        if parts is not None:
            out["val_bce"], out["val_soft_ts"] = parts
        sweep_map = pred_bb_img.detach().reshape(-1, 800, 800)
        if _tta.resolve(self, None) is not None and (hparam(self.hparams, "box_metrics", False) or self._wants_box_sweep()):
            sweep_map = self._tta_box_map(*self._batch_inputs(batch[0], batch[2]), scene=pred_bb_img)
            if hparam(self.hparams, "box_metrics", False):
                require_bounding_boxes(batch[1])
                out["val_ats_tta"] = decoded_box_ats(self.hparams, sweep_map, batch[1])
                out["val_ts_tta"] = ops.threat_score(target_bb_img.contiguous(), sweep_map.reshape(target_bb_img.shape), round_b=True)
        if hparam(self.hparams, "box_metrics", False):
            # the task's own unit: boxes extracted from the predicted map against the targets' boxes, and the map-level threat score
            with torch.no_grad():
                require_bounding_boxes(batch[1])
                out["val_ats"] = decoded_box_ats(self.hparams, pred_bb_img.detach().reshape(-1, 800, 800).contiguous(), batch[1])
                out["val_ts"] = ops.threat_score(target_bb_img.contiguous(), pred_bb_img.detach().contiguous(), round_b=True)
        if self._wants_box_sweep():
            with torch.no_grad():
                require_bounding_boxes(batch[1])
                self._with_box_sweep(out, sweep_map, batch[1])
        return out

    def validation_epoch_end(self, outputs):
        avg_val_loss = torch.stack([x["val_loss"] for x in outputs]).mean()
        logs = {"avg_val_loss": avg_val_loss}
        logs.update(mean_logs(outputs, ("val_ats", "val_ts", "val_bce", "val_soft_ts", "val_ats_tta", "val_ts_tta")))      # present only under hparams.box_metrics / the box-map loss
        if self._wants_box_sweep():
            self._calibrate_boxes(outputs, logs)      # sets box_threshold: the next epoch's val_ats and the predictions decode there
        return {"val_loss": avg_val_loss, "log": logs}

    def configure_optimizers(self):
        return torch.optim.Adam(self.parameters(), lr=self.hparams.learning_rate)

    @staticmethod
    def add_model_specific_args(parent_parser):
        p = ArgumentParser(parents=[parent_parser], add_help=False)
        p.add_argument("--learning_rate", type=float, default=1e-3)
        p.add_argument("--unfreeze_epoch_no", type=int, default=0)
        p.add_argument("--batch_size", type=int, default=16)
        p.add_argument("--mse_loss", action="store_true")
        add_box_args(p)
        p.add_argument("--link", type=str, default="/scratch/ab8690/DLSP20Dataset/data")
        p.add_argument("--pretrained_path", type=str, default="")
        p.add_argument("--output_img_freq", type=int, default=500)
        p.add_argument("--precision", type=str, default="fp32", choices=("fp32", "bf16", "fp32x3"),
                       help="fp32: the reference's arithmetic; bf16: encoder conv stack on the bf16 matrix cores; fp32x3: the box head's "
                            "dilated up-convs as six bf16 products per fp32 product (MI355X build only)")
        add_augment_args(p)
        _tta.add_tta_args(p)
        add_ema_args(p)
        add_weight_decay_args(p)
        return p
