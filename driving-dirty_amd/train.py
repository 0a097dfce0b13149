"""``TrainStep``: the step ``bench.py`` measures, as one callable over any of the drop-in modules.

The reference hands its modules to ``pytorch_lightning.Trainer.fit`` (autoencoder.py:192-193, submit.py:40-46), which per batch does
``optimizer.zero_grad(); out = model.training_step(batch, i); out['loss'].backward(); optimizer.step()`` with the optimizer (and
scheduler) ``configure_optimizers()`` returned -- ``Adam(lr)`` for every module, plus ``ReduceLROnPlateau(patience=10)`` on the
validation loss for the road-map modules (roadmap_bce_v2.py:154-157) -- and, under
``--distributed_backend ddp``, averages gradients across processes.  ``configure_optimizers()`` of the drop-in modules still returns
exactly that (torch.optim.Adam): a caller with its own loop keeps working.  This helper is the SAME step arranged for the MI355X:

  * ``optim.HipAdam`` (one fused pass per tensor, torch.optim.Adam's arithmetic) with the pass of the big tensors on a side stream
    beside the MFMA-bound stretch of the backward (``overlap_with_backward``); the big ``nn.Linear`` weights (encoder fc1, head,
    decoder fc2) take a rank-B update: their gradient is formed inside the Adam pass from the layer's input and output gradient and
    never written (``fuse_linear_wgrad``; ``weight.grad`` of those layers stays None -- pass ``fuse_linear_wgrad=False`` to keep it);
  * ``gradient_clip_val`` / ``track_grad_norm`` (Lightning's Trainer arguments): the global gradient norm measured and applied on the
    device, the rank-B layers' from their factors (``HipAdam.set_clip``); a clipped step runs its optimizer passes after the backward;
  * ``ddp.GradSync`` when ``torch.distributed`` is initialised: per-tensor asynchronous all-reduce from autograd hooks, or -- with
    ``shard_optimizer=True`` -- reduce-scatter, Adam on the owned 1/N, in-place all-gather under the next forward; or -- with
    ``factor_linear=True``, for 2-4 ranks -- the big Linear layers send their factors (input, output gradient) instead of their
    weight gradients and every rank forms the global-batch gradient itself (ddp.py);
  * ``ema_decay`` / ``ema_every`` / ``ema_warmup`` (``--ema_*``): an exponential moving average of the parameters kept on the device
    (``ema.WeightEMA``), updated after the optimizer step; ``averaged()`` evaluates it in place; one GPU only;
  * ``weight_decay`` / ``weight_decay_all`` (``--weight_decay*``): torch.optim.AdamW's decoupled decay inside the same optimizer passes
    (``adamw.py``); biases and BatchNorm vectors are left out unless ``weight_decay_all``; off by default, and off is the same calls;
  * frozen feature extractors (``self.ae.freeze()`` in the fine-tuning modules) are handled: both objects are built over the model
    as constructed and re-arm when ``training_step`` unfreezes it (lightning.on_unfreeze);
  * ``validation_epoch_end(val_loss)`` steps ``ReduceLROnPlateau`` the way Lightning does for a scheduler returned beside the
    optimizer (monitor = ``val_loss``), for the modules whose ``configure_optimizers`` has one.

It is a helper, not a Trainer: no data loading, logging, checkpoint policy or CLI (out of scope).
"""
import torch
import torch.distributed as dist

from .adamw import check_weight_decay
from .ddp import GradSync
from .optim import HipAdam


class TrainStep:
    def __init__(self, model, lr=None, adam_overlap="auto", shard_optimizer=False, reserve_cus=None, process_group=None,
                 force_collectives=False, simulate_world=0, scheduler="auto", big_numel=1 << 20, chunk_numel=1 << 25, factor_linear=False,
                 fuse_linear_wgrad=True, passes_last="auto", gradient_clip_val=None, track_grad_norm=False, ema_decay=None, ema_every=None,
                 ema_warmup=None, weight_decay=None, weight_decay_all=None):
        """``weight_decay`` (None: ``hparams.weight_decay``, absent: 0): decoupled weight decay, torch.optim.AdamW's, with ``keep = 1 - lr
        * weight_decay`` derived from the group's CURRENT lr at every step (ReduceLROnPlateau moves both).  Parameters of at most one
        dimension -- biases, BatchNorm scale and shift -- are excluded unless ``weight_decay_all`` (None: ``hparams.weight_decay_all``,
        absent: False), which decays everything as a bare ``torch.optim.AdamW(model.parameters())`` does.  It composes with
        ``adam_overlap``, ``passes_last``, clipping (the norm is the gradients' alone), the EMA and the scheduler.  Under a live
        ``GradSync`` the elementwise passes work by construction (every rank uses the same ``keep``); like every multi-GPU path here
        that has not been run on more than one GPU."""
        self.model = model
        hp = getattr(model, "hparams", None)
        if lr is None:
            lr = getattr(hp, "learning_rate", None)
            if lr is None:
                raise ValueError("TrainStep: no lr given and model.hparams has no learning_rate")
        # Lightning 0.7.5's --gradient_clip_val / --track_grad_norm (Trainer.from_argparse_args, submit.py:40; its parser leaves 0 in
        # hparams): clip the step to a global 2-norm, log the norm.  On the device, rank-B layers included (HipAdam.set_clip).
        if gradient_clip_val is None:
            gradient_clip_val = getattr(hp, "gradient_clip_val", 0)
        self.clip = float(gradient_clip_val or 0.0)
        self.track = bool(track_grad_norm)
        if self.clip < 0:
            raise ValueError(f"TrainStep: gradient_clip_val = {gradient_clip_val}")
        if self.clip > 0 and adam_overlap is not False and adam_overlap != "auto" and adam_overlap:
            raise ValueError("TrainStep: gradient_clip_val needs the optimizer passes after the backward; adam_overlap=True starts them "
                             "beside it")
        distributed = dist.is_available() and dist.is_initialized()
        world = dist.get_world_size(process_group) if distributed else 1
        comm = distributed and (world > 1 or force_collectives)
        if reserve_cus is None:      # RCCL's workgroups need LDS the resident conv grids do not leave free
            reserve_cus = 16 if comm and next(model.parameters()).is_cuda and dist.get_backend(process_group) == "nccl" else 0
        # over the model AS CONSTRUCTED (extractor possibly frozen): every parameter is in the optimizer from the start, as with
        # the reference's Adam(self.parameters()); a parameter without a gradient is skipped until it has one
        self.optimizer = self._make_optimizer(model.parameters(), lr)
        self.sync = GradSync(model, process_group=process_group, big_numel=big_numel, chunk_numel=chunk_numel, reserve_cus=reserve_cus,
                             force_collectives=force_collectives, shard_optimizer=shard_optimizer, simulate_world=simulate_world,
                             factor_linear=factor_linear)
        self.optimizer.attach(self.sync)
        if (self.clip > 0 or self.track) and (self.sync.active or self.sync.shard or self.sync.factor):
            self.sync.remove()
            raise NotImplementedError("TrainStep: gradient_clip_val / track_grad_norm under a live GradSync (all-reduce, sharded, factor "
                                      "gather) is not implemented: one GPU only")
        # --ema_decay / --ema_every / --ema_warmup (ema.add_ema_args): an exponential moving average of the parameters, updated on the
        # device after every optimizer step (ema.WeightEMA).  Off (decay 0 or absent): self.ema is None and the step is unchanged.
        if ema_decay is None:
            ema_decay = getattr(hp, "ema_decay", 0.0)
        if ema_every is None:
            ema_every = getattr(hp, "ema_every", 1)
        if ema_warmup is None:
            ema_warmup = getattr(hp, "ema_warmup", False)
        ema_decay = float(ema_decay or 0.0)
        if not 0.0 <= ema_decay < 1.0:
            self.sync.remove()
            raise ValueError(f"TrainStep: ema_decay = {ema_decay} is outside [0, 1)")
        if ema_decay > 0 and (self.sync.active or self.sync.shard or self.sync.factor):
            self.sync.remove()
            raise NotImplementedError("TrainStep: ema_decay under a live GradSync (all-reduce, sharded, factor gather) is not implemented: "
                                      "one GPU only (a sharded all-gather still writes parameters under the next forward)")
        # --weight_decay / --weight_decay_all (adamw.add_weight_decay_args).  Off (0 or absent): the optimizer is built and steps as before.
        if weight_decay is None:
            weight_decay = getattr(hp, "weight_decay", 0.0)
        if weight_decay_all is None:
            weight_decay_all = getattr(hp, "weight_decay_all", False)
        try:
            self.weight_decay = check_weight_decay(weight_decay, "TrainStep")
        except ValueError:
            self.sync.remove()
            raise
        self.weight_decay_all = bool(weight_decay_all)
        if self.weight_decay > 0:
            for group in self.optimizer.param_groups:
                group["weight_decay"] = self.weight_decay
            if not self.weight_decay_all:
                self.optimizer.exclude_from_decay(p for p in model.parameters() if p.ndim <= 1)
        self.ema = None
        if ema_decay > 0:
            from .ema import WeightEMA
            try:
                self.ema = WeightEMA(model, ema_decay, every=int(ema_every or 1), warmup=bool(ema_warmup))
            except Exception:
                self.sync.remove()
                raise
        if self.clip > 0 and adam_overlap == "auto":
            adam_overlap = False      # no optimizer pass may start before every gradient exists: the after-backward arrangement
        if adam_overlap == "auto":
            # fp32 models: the passes of the big tensors ride beside the MFMA-bound c2 weight gradient.  A bf16 encoder has no MFMA-bound
            # stretch -- its conv kernels are HBM-bound, and an 11.6 GB optimizer stream beside them only time-shares the same HBM
            # (config 5: the c2 weight gradient at 0.19-0.28 of the HBM peak beside it, 0.62 alone; same step either way,
            # profiles/r05_config5_adam_overlap_ab.txt): there the optimizer runs after the backward, four workgroups per CU
            adam_overlap = not any(getattr(m, "precision", None) == "bf16" for m in model.modules())
        self.overlap = bool(adam_overlap)
        if not self.overlap and next(model.parameters()).is_cuda:
            from . import _lib
            _lib.call("dd_set_adam_blocks_per_cu", 4)
        if self.overlap:
            self.optimizer.overlap_with_backward(big_numel=big_numel, grad_scale=self.sync.grad_scale,
                                                 grad_sync=self.sync if (self.sync.active or self.sync.shard) else None)
        # rank-B mode: the weight gradient of the big Linear layers is formed inside their Adam pass, never written (optim.py); the
        # optimizer declines by itself where the gradient has to travel as a tensor (all-reduce / sharded GradSync)
        self.fused = self.optimizer.fuse_linear_wgrad(model, min_numel=big_numel) if fuse_linear_wgrad else []
        # rank-B passes only fit beside c2's weight gradient: that kernel goes last, the data gradient runs by itself in front of it
        # (HipAdam.passes_last).  Under an all-reduce / sharded GradSync the passes are the plain 48-register kernel, ready at the top of
        # the backward, and keep the old order (they run beside both conv kernels).
        if passes_last == "auto":
            passes_last = bool(self.fused) and not ((self.sync.active or self.sync.shard) and not self.sync.factor)
        if self.overlap and passes_last:
            self.optimizer.passes_last(True)
        if self.clip > 0 or self.track:
            self.optimizer.set_clip(self.clip, track=self.track)
        if scheduler == "auto":      # the modules that return ([optimizer], [scheduler]) from configure_optimizers
            scheduler = self._reference_has_scheduler(model)
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, patience=10) if scheduler else None
        self.last = None
        self._one = None

    @staticmethod
    def _make_optimizer(params, lr):
        return HipAdam(params, lr=lr)

    @staticmethod
    def _reference_has_scheduler(model):
        """Whether the module's own ``configure_optimizers()`` returns ``([optimizer], [scheduler])`` (the road-map modules,
        roadmap_bce_v2.py:154-157) rather than a bare optimizer (autoencoder.py:119-120, spatial_w_rm.py:166-167)."""
        make = getattr(model, "configure_optimizers", None)
        if make is None:
            return False
        out = make()                                        # a torch.optim.Adam over the parameters: no state until it steps
        return isinstance(out, (tuple, list)) and len(out) == 2 and bool(out[1])

    def __call__(self, batch, batch_idx):
        """One training step; returns ``training_step``'s dict (``out['loss']`` is the step's loss, still on the device)."""
        self.optimizer.reset_step()              # a step that never reached step() (an exception on the way) leaves nothing for this one
        self.model.zero_grad(set_to_none=True)
        out = self.model.training_step(batch, batch_idx)
        loss = out["loss"]
        if self._one is None or self._one.device != loss.device or self._one.dtype != loss.dtype:
            self._one = torch.ones((), device=loss.device, dtype=loss.dtype)
        loss.backward(self._one)                 # the root gradient is a kept tensor: no ones_like fill launch per step
        self.sync.finish()
        self.optimizer.step(grad_scale=self.sync.grad_scale)
        if self.ema is not None:                 # step() ended in reset_step(), which joined the side stream: every pass of this step has landed
            self.ema.update()
        if self.track:                           # Lightning's key for --track_grad_norm 2; the value stays on the device
            out.setdefault("log", {})["grad_2.0_norm_total"] = self.optimizer.grad_norm
        self.last = out
        return out

    def sync_params(self):
        """Sharded optimizer: wait for the all-gathers still writing into parameters.  Call before validation, ``state_dict()`` or
        a checkpoint -- anything that reads parameters other than through the next ``training_step``."""
        self.sync.wait_gathers()

    def validation_epoch_end(self, val_loss):
        """``scheduler.step(val_loss)`` once per validation epoch (Lightning 0.7.5's handling of ReduceLROnPlateau)."""
        self.sync_params()
        if self.scheduler is not None:
            self.scheduler.step(float(val_loss))

    def averaged(self):
        """``with step.averaged():`` the model holds the averaged weights (``ema.WeightEMA.applied``): wrap a validation epoch, a
        threshold calibration or a prediction in it.  Buffers (BatchNorm statistics) stay the live model's."""
        if self.ema is None:
            raise RuntimeError("TrainStep.averaged(): weight averaging is off (ema_decay is 0 or absent)")
        return self.ema.applied()

    @property
    def lr(self):
        return self.optimizer.param_groups[0]["lr"]

    def close(self):
        self.sync_params()
        self.optimizer.close()
        self.sync.remove()
        if self.ema is not None:
            self.ema.close()
