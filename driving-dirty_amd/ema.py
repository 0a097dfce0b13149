"""Weight averaging on the device: an exponential moving average (EMA) of the parameters, evaluated and shipped in place of the last
iterate.

The next tool against over-fitting after the class-balanced losses, the calibrated thresholds, the augmentation and the mirror
averaging: it costs no forward pass and composes with all of them.  Two parts.  The BINDER of ``csrc/libdd_ema.so``
(``include/dd_ema.h``), a ``_lib.Extension`` of its entry in ``build.EXTENSIONS``.  And ``WeightEMA``, which ``train.TrainStep`` holds when ``--ema_decay`` is set.

THE SEMANTICS are the header's: per element ``e' = fmaf(alpha, w - e, e)``, one rounded subtract and one fused multiply-add;
``e == w`` keeps ``e``'s bits.  The exchange moves 32-bit words.  The cost is 4 bytes per parameter for the shadows and, per update,
12 bytes of HBM traffic per trainable parameter.

One GPU, fp32 parameters, buffers stay live.
"""
import contextlib
import ctypes as C

import torch

from . import _lib, lightning
from . import build as _build
from ._lib import HotpathError

# ---- the binder ------------------------------------------------------------------------------------------------------------------
_EXT = _lib.Extension(_build.EXTENSIONS["ema"])
LIB, SIGNATURES, STREAMED, OPERANDS = _EXT.library, _EXT.signatures, _EXT.streamed, _EXT.operands
lib, launch, last_error = _EXT.lib, _EXT.launch, _EXT.last_error      # module-level names: the methods below reach ``launch`` through the module's globals at call time
CHUNK = _EXT.constant("DD_EMA_CHUNK")              # elements per piece of the kernels' flat work list
TABLE_MAX = _EXT.constant("DD_EMA_TABLE_MAX")      # tensors per launch; a longer table is split


def pointer_tables(a, b):
    """Two equally long lists of tensors -> the operands of a ``*_ptrs`` call: (HOST array of ``a``'s device pointers, the same of
    ``b``'s, HOST array of int64 element counts, the number of tensors)."""
    n = len(a)
    return ((C.c_void_p * n)(*[t.data_ptr() for t in a]), (C.c_void_p * n)(*[t.data_ptr() for t in b]),
            (C.c_int64 * n)(*[t.numel() for t in a]), n)


# ---- the schedule, in Python floats ------------------------------------------------------------------------------------------------
def decay_at(decay, t, warmup=False):
    """The decay of update number ``t`` (counted from 0).  Warmup: ``min(decay, (1 + t) / (10 + t))``, so that the first updates do
    not average in the initial weights at full weight."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def alpha_at(decay, every, t, warmup=False):
    """The weight of the parameters in update number ``t`` when one update stands for ``every`` steps: ``1 - decay_t ** every``."""
    return 1.0 - decay_at(decay, t, warmup) ** every


class WeightEMA:
    """fp32 device copies (the shadows) of every parameter of ``model``, taken now and bit-equal to the weights; ``update()`` after
    each optimizer step moves them towards the weights, ``applied()`` / ``swap()`` exchange them with the weights in place.

    ``decay``: the average's memory per step, in [0, 1).  ``every``: one update per ``every`` steps, with ``alpha = 1 -
    decay ** every``.  ``warmup``: ``decay_at`` above.

    A parameter that is not fp32, not on the device or not contiguous is refused by name.  BUFFERS are neither averaged nor
    exchanged: BatchNorm running statistics and ``num_batches_tracked`` stay the live model's, which is
    ``torch.optim.swa_utils.AveragedModel(use_buffers=False)``'s choice.

    A parameter enters the update's table when it first has ``requires_grad`` and then stays in it.  Leaving a frozen one out is
    EXACT, not an approximation: its shadow equals it, and ``e == w`` keeps ``e`` (dd_ema.h).  The host tables are rebuilt when the
    set of tensors changes (``lightning.on_unfreeze`` calls ``refresh()``; a flag or a storage changed by hand is noticed too), not
    per step."""

    def __init__(self, model, decay, every=1, warmup=False):
        decay, every = float(decay), int(every)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"WeightEMA: decay = {decay} is outside [0, 1)")
        if every < 1:
            raise ValueError(f"WeightEMA: every = {every}, at least 1")
        self.model, self.decay, self.every, self.warmup = model, decay, every, bool(warmup)
        self.names, self.params = [], []
        for name, p in model.named_parameters():
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise HotpathError(f"WeightEMA: parameter '{name}' must be a contiguous fp32 device tensor, got {p.dtype} on {p.device} "
                                   f"contiguous={p.is_contiguous()}")
            if p.numel() == 0:
                continue
            self.names.append(name)
            self.params.append(p)
        if not self.params:
            raise ValueError("WeightEMA: the model has no parameters")
        self.shadows = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.params]
        self.steps = 0            # update() calls
        self.num_updates = 0      # of which made an update
        self.is_applied = False
        self._moved = [False] * len(self.params)      # in the update's table: has had requires_grad since its shadow equalled it
        self._key, self._update_table, self._swap_key, self._swap_table = None, None, None, None
        lightning.on_unfreeze(self)

    # ---- the tables ----------------------------------------------------------------------------------------------------------------
    def refresh(self):
        """The set of trainable parameters may have changed (``LightningModule.unfreeze()``): look again at the next update."""
        self._key = None

    def _state_key(self):
        return tuple((p.data_ptr(), p.requires_grad) for p in self.params)

    def _tables(self):
        key = self._state_key()
        if key != self._key:
            for i, (_, grad) in enumerate(key):
                self._moved[i] = self._moved[i] or grad
            pick = [i for i, m in enumerate(self._moved) if m]
            self._update_table = pointer_tables([self.shadows[i] for i in pick], [self.params[i] for i in pick]) if pick else None
            self._key = key
        return self._update_table

    def alpha(self):
        """The next update's alpha (``alpha_at``)."""
        return alpha_at(self.decay, self.every, self.num_updates, self.warmup)

    # ---- the update ----------------------------------------------------------------------------------------------------------------
    def update(self):
        """Call after the optimizer step, on the stream the step ends on.  Counts the step; on every ``every``-th makes ONE
        dd_ema_update_ptrs call over the trainable parameters.  True when an update was made."""
        if self.is_applied:
            raise RuntimeError("WeightEMA.update(): the averaged weights are applied (inside applied(), or after an odd number of swap()): "
                               "the model holds the average and the shadows the weights")
        self.steps += 1
        if self.steps % self.every:
            return False
        table = self._tables()
        if table is not None:
            launch("dd_ema_update_ptrs", *table, self.alpha())
        self.num_updates += 1
        return True

    # ---- the exchange --------------------------------------------------------------------------------------------------------------
    def swap(self):
        """Exchange every parameter with its shadow in place (dd_ema_swap_ptrs): the storages keep their addresses, so a forward after
        it reads the averaged weights.  Frozen parameters are exchanged too, which for them is the identity."""
        key = tuple(p.data_ptr() for p in self.params)
        if key != self._swap_key:
            self._swap_table, self._swap_key = pointer_tables(self.params, self.shadows), key
        launch("dd_ema_swap_ptrs", *self._swap_table)
        self.is_applied = not self.is_applied

    @contextlib.contextmanager
    def applied(self):
        """``with ema.applied():`` the model holds the averaged weights; on exit -- also when the body raises -- the live ones again."""
        if self.is_applied:
            raise RuntimeError("WeightEMA.applied(): the averaged weights are applied already")
        self.swap()
        try:
            yield self.model
        finally:
            self.swap()

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """What resuming training needs: the shadows by parameter name (copies), the counters and the schedule."""
        if self.is_applied:
            raise RuntimeError("WeightEMA.state_dict(): the averaged weights are applied; the shadows hold the live weights")
        return {"shadows": {n: s.detach().clone() for n, s in zip(self.names, self.shadows)}, "num_updates": self.num_updates,
                "steps": self.steps, "decay": self.decay, "every": self.every, "warmup": self.warmup}

    def load_state_dict(self, state):
        if self.is_applied:
            raise RuntimeError("WeightEMA.load_state_dict(): the averaged weights are applied")
        shadows = state["shadows"]
        if set(shadows) != set(self.names):
            odd = sorted(set(shadows) ^ set(self.names))
            raise KeyError(f"WeightEMA.load_state_dict(): the shadows' names differ from the model's parameters: {odd[:8]}")
        for i, (name, mine) in enumerate(zip(self.names, self.shadows)):
            theirs = shadows[name]
            if tuple(theirs.shape) != tuple(mine.shape) or theirs.dtype != torch.float32:
                raise ValueError(f"WeightEMA.load_state_dict(): '{name}' is {theirs.dtype} {tuple(theirs.shape)}, expected fp32 {tuple(mine.shape)}")
            mine.copy_(theirs)      # in place: the shadow keeps its address
            # a shadow that differs from its parameter goes on following it, frozen or not
            self._moved[i] = not torch.equal(mine, self.params[i].detach())
        self.num_updates, self.steps = int(state["num_updates"]), int(state["steps"])
        self.decay, self.every, self.warmup = float(state["decay"]), int(state["every"]), bool(state["warmup"])
        self._key = None

    def save_checkpoint(self, path):
        """``model.save_checkpoint(path)`` with the averaged weights applied: an ordinary checkpoint of the module, which
        ``load_from_checkpoint`` and the prediction tools take as it is.  The live weights are back afterwards."""
        with self.applied():
            self.model.save_checkpoint(path)

    def close(self):
        """Stop listening for ``unfreeze()``."""
        lightning._UNFREEZE_LISTENERS.discard(self)


def add_ema_args(p):
    """``--ema_decay`` / ``--ema_every`` / ``--ema_warmup``, for the ``add_model_specific_args`` of the models ``train.TrainStep`` trains."""
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="keep an exponential moving average of the parameters with this decay per step (0: off); evaluate and save it "
                        "through TrainStep.averaged() / TrainStep.ema.save_checkpoint()")
    p.add_argument("--ema_every", type=int, default=1, help="update the average every N steps, with decay ** N")
    p.add_argument("--ema_warmup", action="store_true", help="decay min(ema_decay, (1 + t) / (10 + t)) at update t")
    return p
