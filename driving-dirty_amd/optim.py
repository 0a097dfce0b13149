"""``HipAdam``: torch.optim.Adam semantics (reference autoencoder.py:119-120, roadmap_bce_v2.py:154-157)
executed by ``dd_adam_step``, one fused read-modify-write pass per parameter tensor.

``grad_scale`` folds the 1/world_size of data-parallel gradient averaging into the same pass, so the
all-reduced SUM never needs a separate divide kernel.

Rank-B mode (``fuse_linear_wgrad(module)``; round 5): the weight gradient of a big ``nn.Linear`` is never written.  ``ops.Linear.backward``
hands its factors -- the layer's input X [rows, in] and output gradient dY [rows, out] -- to ``linear_factors`` instead of launching
``dd_linear_wgrad``, ``weight.grad`` stays None, and ``dd_adam_step_rankb`` forms every gradient element dW[o][i] = sum_b dY[b][o] X[b][i]
in MFMA accumulators inside the optimizer pass (bias: the column sum of dY, updated by the same launch): six passes over the tensor
instead of eight (reference call sites: components.py:105, roadmap_bce_v2.py:75,154-157).  Used when the gradient does not have to
travel as a tensor: one GPU, or ``GradSync`` factor mode (the gathered factors feed the same kernel).  With an all-reduce or a sharded
``GradSync`` the layer keeps its materialised gradient.

Shard mode (``attach(grad_sync)`` / ``overlap_with_backward(grad_sync=...)`` with ``GradSync(shard_optimizer=True)``): a tensor
that travels as reduce-scatter + all-gather is updated only in the slices this rank owns (``grad_sync.shards(p)``), its moments
exist only for those slices (``state[p]["shards"][piece] = (exp_avg, exp_avg_sq)``), and each updated slice is handed straight
back to ``grad_sync.gather_shard`` -- piece k's all-gather is on the links while piece k+1's update runs.  Elementwise, so the
owned elements get bit for bit the update of the whole-tensor pass.

Decoupled weight decay (``weight_decay=``; ``adamw.py``, include/dd_adamw.h): torch.optim.AdamW's step.  A decayed parameter is
multiplied by ``keep = float32(1 - lr * weight_decay)`` in front of its Adam update, inside the same streaming pass (``dd_adamw_step``,
``dd_adamw_step_multi``: no extra HBM bytes); a rank-B tensor, whose kernels do not take the factor, is pre-scaled by ``dd_decay`` on
the same stream directly in front of its pass.  The moments never see the decay.  Off (0, the default) every call is the one made
without the option, and ``adamw`` is never entered.
"""
from types import SimpleNamespace

import torch

from . import _lib, adamw, lightning, ops


class HipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        weight_decay = adamw.check_weight_decay(weight_decay, "HipAdam")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._no_decay = set()     # id(p) of the parameters exclude_from_decay() has marked
        self._side = None
        self._now = None           # this step's bookkeeping: reset_step()
        self.reset_step()
        self._hooks = []
        self._hooked = set()
        self._big_numel = 1 << 20
        self._scale = 1.0
        self._sync = None
        self._fgrad = {}           # p -> persistent buffer of the global-batch gradient formed from gathered factors
        self._rankb = {}           # weight -> bias (or None): Linear layers whose gradient is formed inside the Adam pass
        self._rankb_keys = {}      # data_ptr -> weight
        self._plan_key = self._plan = None      # _rankb_plan()'s last answer
        self._last = False         # passes_last(): c2's data gradient first, the queued passes beside its weight gradient
        self._clip_max = 0.0       # set_clip(): clip the step's gradients to this global 2-norm (0: off)
        self._clip_track = False   # set_clip(): measure the global norm every step
        self._slots = None         # persistent fp64 buffer, one squared norm per launch of the norm kernels
        self._out3 = None          # persistent fp32 {grad_scale * coef, norm, coef} (dd_clip_scale)
        self.grad_norm = None      # device scalars, valid after a step() with set_clip(): views of _out3
        self.clip_coef = None

    SMALL_NUMEL = 1 << 16      # tensors up to this size go into one multi-tensor launch (0: never; tests set it per instance)
    MAX_ROWS = 64      # dd_adam_step_rankb: batch rows (world x batch for gathered factors)
    EARLY_SPARE_CUS = 8      # CUs an "early" pass leaves free of its workgroups (dd_set_adam_spare_cus)

    def reset_step(self):
        """Forget what a backward has left for this step's passes.  ``step()`` ends with it; ``close()`` and ``TrainStep.__call__`` call
        it so that a step abandoned half way (an exception in ``training_step`` or in the backward) leaves nothing for the next one.
        Nothing to forget (every step that ran to its end): no library call, no stream operation, no allocation.  Not called from the
        backward: two backwards before one ``step()`` still add up."""
        if self._now is not None:
            if not any(vars(self._now).values()):
                return
            if self._side is not None:      # launches on the side stream may still read the factors in ``held``
                torch.cuda.current_stream().wait_stream(self._side)
        self._now = SimpleNamespace(
            pending=[],        # (p, group) whose pass is launched on the side stream when backward reaches its MFMA-bound stretch
            early=set(),       # tensors whose pass of this step has been launched
            rankb_now={},      # weight -> (x, dy, bias) of this step's backward, until the pass has been launched
            held=[],           # factors read by launches on the side stream: kept until the side stream has been joined
            fac_now={},        # weight -> gathered Factors that have arrived (factor mode of ddp.GradSync + rank-B)
            factored=[])       # parameters whose factors are on the links (ddp.GradSync, factor mode)

    def _state_of(self, p):
        st = self.state[p]
        if not st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    # ---- decoupled weight decay ----------------------------------------------------------------------------------------------
    def exclude_from_decay(self, params):
        """Mark ``params`` as never decayed (biases, BatchNorm scale and shift): their ``keep`` is 1 whatever the group's
        ``weight_decay``.  One param group stays one param group: the state dict's layout does not change."""
        self._no_decay.update(id(p) for p in params)

    def _keep(self, p, group):
        """The fp32 factor ``p`` is multiplied by in front of its update: 1.0 when the group's decay is 0 (or absent: a state dict
        saved before the option existed) or ``p`` is excluded, else ``adamw.keep_of`` of the group's CURRENT lr (a scheduler moves it)."""
        wd = group.get("weight_decay", 0.0)
        if not wd or id(p) in self._no_decay:
            return 1.0
        return adamw.keep_of(group["lr"], wd)

    def _launch(self, p, g, m, v, group, step, grad_scale, keep=1.0):
        """The one place the elementwise kernel is called (flat fp32 device tensors of equal length).  ``keep``: the factor of the
        parameter these operands are (slices of); 1: dd_adam_step(_dev), else dd_adamw_step with the same operands."""
        b1, b2 = group["betas"]
        if keep == 1.0:
            ops.adam_step_flat(p, g, m, v, group["lr"], b1, b2, group["eps"], step, grad_scale)
        else:
            adamw.step_flat(p, g, m, v, group["lr"], b1, b2, group["eps"], step, grad_scale, keep)

    def _pass(self, p, g, m, v, group, step, grad_scale, keep):
        """``_launch`` for operands of a parameter whose factor is ``keep``.  1 makes the call made before the option existed,
        argument for argument: a subclass that replaces ``_launch`` in that form (tests/test_shard_gloo.py) is served while the decay
        is off."""
        if keep == 1.0:
            return self._launch(p, g, m, v, group, step, grad_scale)
        return self._launch(p, g, m, v, group, step, grad_scale, keep)

    # ---- rank-B mode -----------------------------------------------------------------------------------------------------------
    def fuse_linear_wgrad(self, module, min_numel=None):
        """Register every ``nn.Linear`` of ``module`` whose weight has >= ``min_numel`` elements (default: the big-tensor threshold)
        and belongs to this optimizer: from now on its weight gradient is formed inside its Adam pass (``dd_adam_step_rankb``) and
        ``weight.grad`` / ``bias.grad`` stay None after a backward.  Returns the registered weights."""
        owned = {id(p) for group in self.param_groups for p in group["params"]}
        limit = self._big_numel if min_numel is None else min_numel
        done = []
        for mod in module.modules():
            w = getattr(mod, "weight", None)
            if not isinstance(mod, torch.nn.Linear) or w is None or id(w) not in owned or w.numel() < limit:
                continue
            if not (w.is_cuda and w.dtype == torch.float32 and w.data.is_contiguous() and w.shape[1] % 4 == 0 and w.shape[0] % 4 == 0):
                continue
            b = mod.bias if (mod.bias is not None and id(mod.bias) in owned and mod.bias.dtype == torch.float32) else None
            self._rankb[w] = b
            self._rankb_keys[w.data_ptr()] = w
            ops.RANKB[w.data_ptr()] = self
            done.append(w)
        return done

    def _sync_blocks_rankb(self):
        """A gradient that has to travel as a tensor (all-reduce or reduce-scatter) must exist as one."""
        s = self._sync
        return s is not None and (getattr(s, "active", False) or getattr(s, "shard", False)) and not getattr(s, "factor", False)

    # Beside the backward a rank-B pass needs 72 registers: it fits beside the c2 WEIGHT gradient (440) and beside the small kernels in
    # front of the conv stack's backward, not beside the fused data gradient (475), which cannot start on a CU until the optimizer's
    # workgroup there has drained (the plain 48-register dd_adam_step runs beside all of them).  With the passes last (passes_last) there are
    # two places for a rank-B pass, both sized per batch row (config 2 at 32 rows in brackets):
    #   * the WINDOW beside the weight gradient (~1.2 ms; a pass moves ~2.5 GB/ms there): the largest registered tensor whose p / m / v
    #     bytes fit WINDOW_BYTES_PER_ROW (3.2 GB: fc1's 2.9 GB, 1.26 ms);
    #   * EARLY, on the side stream the moment the factors exist, beside the FC tail's and c3's HBM-bound kernels (1.5-2 ms until the data
    #     gradient is dispatched): the other tensors, smallest first, while they fit EARLY_BYTES_PER_ROW (4 GB: the head's 1.0 GB, 0.37 ms
    #     there; the autoencoder's decoder fc2, 3.9 GB, whose factors exist before the encoder's backward starts: 11.17 -> 10.96 ms).
    # Everything else keeps its materialised gradient and the plain pass.  A/B on one box each (profiles/r05_ab_rankb_schedule.txt): config 2
    # both in the window 7.40, head early 7.29 ms; autoencoder bs 32 with both of its tensors (6.7 GB) queued for the window 12.1 ms -- the data
    # gradient waited 1.6 ms for them --, fc1 in the window and the decoder's fc2 plain 11.0-11.2, fc2 early 10.9-11.0 (no rank-B: 11.1-11.4);
    # hidden 256: the head rides, fc1 (5.8 GB) stays plain.
    WINDOW_BYTES_PER_ROW = 1.0e8
    EARLY_BYTES_PER_ROW = 1.25e8

    def _rankb_plan(self, rows):
        """{tensor: "window" | "early"} for the registered tensors that take the rank-B pass at this batch size (overlap mode)."""
        live = sorted((q for q in self._rankb if q.requires_grad), key=lambda q: q.numel())
        key = (rows, self._last, tuple(id(q) for q in live))
        if self._plan_key == key:
            return self._plan
        cost = lambda q: 24.0 * q.numel()
        plan = {}
        fits = [q for q in live if cost(q) <= self.WINDOW_BYTES_PER_ROW * rows]
        if fits:
            plan[fits[-1]] = "window"
        if self._last:
            budget = self.EARLY_BYTES_PER_ROW * rows
            for q in live:
                if q not in plan and q.numel() >= self._big_numel and cost(q) <= budget:
                    plan[q] = "early"
                    budget -= cost(q)
        else:      # passes in front of the weight gradient (no rank-B window of their own): what fits it together, smallest first
            budget = 1.25 * self.WINDOW_BYTES_PER_ROW * rows
            plan = {}
            for q in live:
                budget -= cost(q)
                if budget < 0:
                    break
                plan[q] = "window"
        self._plan_key, self._plan = key, plan
        return plan

    def _rankb_fits(self, p, rows):
        if self._side is None:
            return True                                       # passes after the backward, by themselves: no window to fit
        return p in self._rankb_plan(rows)

    def _goes_early(self, p, rows):
        return self._rankb_plan(rows).get(p) == "early"

    def linear_factors(self, weight, x, dy):
        """Called by ``ops.Linear.backward`` (on the backward's stream) for a weight registered in ``ops.RANKB``.  Returns 0: declined,
        the caller forms dW and db as usual; 1: the weight's gradient will be formed from (x, dy) inside its Adam pass, the caller
        still owes db; 2: the bias is updated by that pass too."""
        p = self._rankb_keys.get(weight.data_ptr())
        if p is None or not p.requires_grad or p.grad is not None or self._sync_blocks_rankb():
            return 0
        if x.shape[0] > self.MAX_ROWS or (p not in self._now.rankb_now and not self._rankb_fits(p, x.shape[0])):
            return 0
        if not (x.is_contiguous() and dy.is_contiguous() and x.dtype == torch.float32 and dy.dtype == torch.float32):
            return 0
        bias = self._rankb[p]
        if bias is not None and (not bias.requires_grad or bias.grad is not None):
            bias = None
        if p in self._now.early:
            raise RuntimeError("HipAdam (rank-B mode): a Linear layer ran a second backward after its optimizer pass of this step was "
                               "launched; call step() between the backwards or build TrainStep(fuse_linear_wgrad=False)")
        prev = self._now.rankb_now.get(p)
        if prev is not None:      # a second backward through the layer before the step (shared weight, retained graph): the gradients add
            x, dy = torch.cat([prev[0], x]), torch.cat([prev[1], dy])
        else:
            self._queue_rankb(p)
        self._now.rankb_now[p] = (x, dy, bias)
        if prev is None and self._side is not None and self._last and self._goes_early(p, x.shape[0]):
            # the window beside c2's weight gradient belongs to the LARGEST rank-B tensor (it fills it: fc1's pass 1.26 ms beside a 1.21 ms
            # kernel); a smaller one queued in front of it would push it past the kernel's end.  It goes to the side stream now, beside the
            # small HBM-bound kernels between here and the conv stack's backward (head: 0.37 ms there; config 2 7.40 -> 7.29 ms, same box)
            # One CU per XCD stays free of the pass: a single-workgroup kernel of the backward that needs nearly a whole CU's LDS
            # (dd_mlp_tail_bwd, 154 KB) cannot start beside a workgroup of the pass (16 KB) and, with one on every CU, waited for the first
            # of them to retire -- 0.6 ms of the autoencoder's step, whose decoder fc2 pass (1.0 ms) is in flight when the encoder's FC tail
            # comes up (profiles/r05_ae_bs32_kernel_stats.csv: mlp_tail_bwd 626 us there, 40 us by itself)
            ev = torch.cuda.current_stream().record_event()
            with torch.no_grad(), torch.cuda.stream(self._side):
                self._side.wait_event(ev)
                _lib.call("dd_set_adam_spare_cus", self.EARLY_SPARE_CUS)
                try:
                    self._take_rankb(p, self._group_of(p), self._scale)
                finally:
                    _lib.call("dd_set_adam_spare_cus", 0)
            self._now.pending = [(q, g) for q, g in self._now.pending if q is not p]
        return 2 if bias is not None else 1

    def factor_bias(self, weight, rows):
        """Factor mode of ddp.GradSync: whether the pass over the gathered factors (``rows`` = world x batch of them) will update this
        layer's bias too (then the caller owes no bias gradient)."""
        p = self._rankb_keys.get(weight.data_ptr())
        bias = self._rankb.get(p) if p is not None else None
        return (bias is not None and bias.requires_grad and bias.grad is None and rows <= self.MAX_ROWS and not self._sync_blocks_rankb())

    def _queue_rankb(self, p):
        if self._side is not None and p.numel() >= self._big_numel:
            self._now.pending.append((p, self._group_of(p)))      # launched on the side stream when backward reaches its MFMA-bound stretch

    def _update_rankb(self, p, group, grad_scale, x, dy, bias):
        """The one place ``dd_adam_step_rankb`` is called: Adam on ``p`` (and ``bias``) with the gradient dy^T x formed on the fly."""
        st = self._state_of(p)
        if "shards" in st:
            raise RuntimeError("HipAdam: a sharded tensor cannot take a rank-B update")
        st["step"] += 1
        bst = None
        if bias is not None:
            bst = self._state_of(bias)
            bst["step"] += 1
            if bst["step"] != st["step"]:
                raise RuntimeError("HipAdam: a Linear layer's weight and bias have taken different numbers of steps")
            self._now.early.add(bias)
        b1, b2 = group["betas"]
        # decoupled decay: the rank-B kernels do not take the factor, so the tensor is pre-scaled on this stream directly in front of
        # its pass -- behind the backward's last read of the weight by construction, and the bits of the fused form (dd_adamw.h).  8
        # more bytes per element than the pass's 24: WINDOW_BYTES_PER_ROW / EARLY_BYTES_PER_ROW were tuned without them and are NOT
        # changed (the measured effect: DESIGN.md 3.2d)
        keep = self._keep(p, group)
        if keep != 1.0:
            adamw.decay(p.data, keep)
        if bias is not None:
            keep = self._keep(bias, group)
            if keep != 1.0:
                adamw.decay(bias.data, keep)
        ops.adam_step_rankb(p.data, st["exp_avg"], st["exp_avg_sq"], dy, x, None if bias is None else bias.data,
                            None if bst is None else bst["exp_avg"], None if bst is None else bst["exp_avg_sq"],
                            group["lr"], b1, b2, group["eps"], st["step"], grad_scale)
        self._now.held.append((x, dy, bias is not None))      # (the flag: what rankb_sqnorm needs when it measures a pass that already ran)
        self._now.early.add(p)

    def _take_rankb(self, p, group, grad_scale):
        now = self._now.rankb_now.pop(p, None)
        if now is None:
            return False
        self._update_rankb(p, group, grad_scale, *now)
        return True

    def attach(self, grad_sync):
        """Use ``grad_sync`` (ddp.GradSync) for per-piece waits and, in shard mode, for the shards and their all-gathers."""
        self._sync = grad_sync
        if getattr(grad_sync, "factor", False):
            grad_sync.on_factors = lambda p: self._now.factored.append(p)

    def _group_of(self, p):
        for group in self.param_groups:
            if any(q is p for q in group["params"]):
                return group
        raise RuntimeError("HipAdam: factors arrived for a tensor this optimizer does not own")

    def _form_factored(self, p):
        """Factor mode: wait (on the CURRENT stream) for the gathers of the layer's input and output gradient and form the
        global-batch weight gradient dy_all^T x_all into ``p.grad``."""
        fac = self._sync.take_factors(p)
        if fac is None:
            return False
        for work in fac.works:
            work.wait()
        if p in self._rankb and fac.rows <= self.MAX_ROWS:      # rank-B mode: no gradient tensor, the gathered factors go straight into the Adam pass
            self._now.fac_now[p] = fac
            return True
        g = self._fgrad.get(p)
        if g is None or g.shape != p.shape or g.device != p.device:
            g = self._fgrad[p] = torch.empty_like(p, memory_format=torch.contiguous_format)
        ops.linear_wgrad(fac.dy_all, fac.x_all, g)
        p.grad = g
        return True

    def _update_formed(self, p, group, grad_scale):
        """The Adam pass behind ``_form_factored``: from ``p.grad``, or -- rank-B mode -- straight from the gathered factors."""
        fac = self._now.fac_now.pop(p, None)
        if fac is None:
            return self._update(p, group, grad_scale)
        bias = self._rankb[p]
        if bias is not None and (not bias.requires_grad or bias.grad is not None):
            bias = None
        self._update_rankb(p, group, grad_scale, fac.x_all, fac.dy_all, bias)

    def _update_factored(self, p, group, grad_scale):
        if not self._form_factored(p):
            return False
        self._update_formed(p, group, grad_scale)
        return True

    @torch.no_grad()
    def _flush_factored(self):
        """Between c2's two gradient kernels (backward_phase2): the factors gathered since the top of the backward have
        arrived (N = 2: 202 MB over one link in ~3 ms).  The weight-gradient kernels run HERE, on the backward's stream -- on the side
        stream, beside conv kernels that fill every CU with 440-register waves, they starve (measured on a one-rank communicator:
        81 us -> 1.2 ms) -- and the Adam passes, built to run beside those kernels, go to the side stream behind them."""
        if not self._now.factored:
            return
        done = [p for p in self._now.factored if self._form_factored(p)]
        self._now.factored.clear()
        ev = torch.cuda.current_stream().record_event()
        with torch.cuda.stream(self._side):
            self._side.wait_event(ev)
            for p in done:
                self._update_formed(p, self._group_of(p), self._scale)
                self._now.early.add(p)

    def _update_shards(self, p, group, grad_scale, shards):
        """The update of the slices of ``p`` this rank owns: wait (on the current stream) for piece k's reduce-scatter, update the
        slice, start its all-gather behind the update, go on.  Whole moments found in the state (a checkpoint in torch.optim.Adam's
        layout -- the reference's -- or steps taken in all-reduce mode before) are cut into this rank's slices on the way."""
        st = self.state[p]
        if not st:
            st["step"] = 0
            st["shards"] = {}
        whole = None
        if "shards" not in st:
            whole = (st.pop("exp_avg").reshape(-1), st.pop("exp_avg_sq").reshape(-1))
            st["shards"] = {}
        st["step"] += 1
        for sh in shards:
            if sh.work is not None:
                sh.work.wait()
            mv = st["shards"].get(sh.index)
            if mv is None or mv[0].numel() != sh.param.numel():
                if whole is not None:
                    mv = (whole[0][sh.lo:sh.hi].clone(), whole[1][sh.lo:sh.hi].clone())
                else:
                    mv = (torch.zeros_like(sh.param), torch.zeros_like(sh.param))
                st["shards"][sh.index] = mv
            self._pass(sh.param, sh.grad, mv[0], mv[1], group, st["step"], grad_scale, self._keep(p, group))
            self._sync.gather_shard(p, sh)

    # ---- checkpoints of the optimizer ------------------------------------------------------------------------------------------
    def _whole_moments(self, p, st):
        """(exp_avg, exp_avg_sq) of ``p`` as whole tensors: the sharded moments all-gathered piece by piece (a COLLECTIVE when the
        GradSync is live: every rank calls it, for the same tensors in the same order)."""
        sync = self._sync
        if sync is None or not getattr(sync, "shard", False):
            raise RuntimeError("HipAdam: sharded moments but no sharded GradSync attached to put them together")
        import torch.distributed as dist
        m = torch.zeros_like(p, memory_format=torch.contiguous_format)
        v = torch.zeros_like(p, memory_format=torch.contiguous_format)
        mf, vf = m.view(-1), v.view(-1)
        w, r = sync.shard_world, sync.rank
        for k, (a, b) in enumerate(sync._pieces_of(p.numel())):
            n = (b - a) // w
            mv = st["shards"].get(k)
            if mv is None:
                mv = (torch.zeros(n, device=p.device, dtype=p.dtype), torch.zeros(n, device=p.device, dtype=p.dtype))
            if sync.active:
                dist.all_gather_into_tensor(mf[a:b], mv[0], group=sync.group)
                dist.all_gather_into_tensor(vf[a:b], mv[1], group=sync.group)
            else:                                 # simulate_world: one process holds rank 0's slices only
                mf[a + r * n:a + (r + 1) * n].copy_(mv[0])
                vf[a + r * n:a + (r + 1) * n].copy_(mv[1])
        return m, v

    def consolidated_state_dict(self):
        """``state_dict()`` in torch.optim.Adam's layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter: what the reference's
        ``configure_optimizers()`` optimizer writes, autoencoder.py:119-120 / roadmap_bce_v2.py:154-157) whatever mode the steps were
        taken in.  In shard mode each rank holds 1 / world of the moments of a sharded tensor: they are all-gathered here, so EVERY rank
        must call this (the result is the same on all of them; save rank 0's).  Loads into ``torch.optim.Adam`` and into a ``HipAdam``
        of any mode (``_update_shards`` cuts whole moments into slices again)."""
        if self._sync is not None and hasattr(self._sync, "wait_gathers"):
            self._sync.wait_gathers()
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)
        sd = super().state_dict()
        flat = [p for group in self.param_groups for p in group["params"]]
        for idx, p in enumerate(flat):
            st = sd["state"].get(idx)
            if st is None:
                continue
            st = dict(st)
            if "shards" in st:
                m, v = self._whole_moments(p, st)
                del st["shards"]
                st["exp_avg"], st["exp_avg_sq"] = m, v
            sd["state"][idx] = st
        return sd

    def load_state_dict(self, state_dict):
        """Takes torch.optim.Adam's state (whole moments; ``step`` possibly a tensor) as well as this class's own, with or without a
        ``weight_decay`` in its groups (absent: 0).  torch.optim.AdamW's state carries its decay over with the same meaning.  A
        torch.optim.Adam state with a non-zero ``weight_decay`` is L2-COUPLED decay (added to the gradient, seen by the moments), another
        algorithm: refused.  The two are told apart by ``decoupled_weight_decay``, which torch writes into both (False / True)."""
        for group in state_dict["param_groups"]:
            if group.get("weight_decay", 0.0) and group.get("decoupled_weight_decay") is False:
                raise ValueError("HipAdam.load_state_dict: the state is torch.optim.Adam's with weight_decay = "
                                 f"{group['weight_decay']}: L2-coupled decay, which this optimizer does not implement (its "
                                 "weight_decay is torch.optim.AdamW's decoupled one)")
            adamw.check_weight_decay(group.get("weight_decay", 0.0), "HipAdam.load_state_dict")
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if "step" in st and isinstance(st["step"], torch.Tensor):
                st["step"] = int(st["step"].item())

    def _update_pieces(self, p, group, grad_scale, pieces):
        """The update of a tensor whose all-reduce travels in pieces: wait (on the current stream) for piece k, update that
        slice, go on -- the pass over piece k runs while piece k+1 is still on the links."""
        st = self._state_of(p)
        st["step"] += 1
        b1, b2 = group["betas"]
        if not (p.grad.is_contiguous() and p.data.is_contiguous()):
            for work, _, _ in pieces:
                work.wait()
            st["step"] -= 1
            return self._update(p, group, grad_scale)
        pf, gf, mf, vf = p.data.view(-1), p.grad.view(-1), st["exp_avg"].view(-1), st["exp_avg_sq"].view(-1)
        keep = self._keep(p, group)
        for work, off, n in pieces:
            work.wait()
            self._pass(pf[off:off + n], gf[off:off + n], mf[off:off + n], vf[off:off + n], group, st["step"], grad_scale, keep)

    def _update(self, p, group, grad_scale):
        st = self._state_of(p)
        if "shards" in st:
            if self._sync is None or not getattr(self._sync, "shard", False):
                raise RuntimeError("HipAdam: a tensor with sharded moments is updated whole and no sharded GradSync is attached to put "
                                   "them together (GradSync removed while its optimizer lives on?): save with consolidated_state_dict() "
                                   "before leaving shard mode")
            st["exp_avg"], st["exp_avg_sq"] = self._whole_moments(p, st)      # a collective: every rank is here for the same tensor
            del st["shards"]
        st["step"] += 1
        g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
        self._pass(p.data.view(-1), g.view(-1), st["exp_avg"].view(-1), st["exp_avg_sq"].view(-1), group, st["step"], grad_scale,
                   self._keep(p, group))

    def overlap_with_backward(self, big_numel=1 << 20, grad_scale=1.0, grad_sync=None):
        """Run the Adam pass of every parameter of >= ``big_numel`` elements on a side stream the moment autograd has
        finished its gradient (post-accumulate-grad hook) instead of after backward.

        Same arithmetic, different timing: the 481 MB encoder ``fc1`` weight and the 164 MB head weight get their
        gradients at the START of backward, and their optimizer pass is pure HBM streaming (7 passes over the
        tensor), while the conv data/weight-gradient kernels that follow are MFMA-bound and leave most of the HBM
        bandwidth idle -- so ~0.8 of the 1.0 ms Adam time disappears under them.  With ``grad_sync`` (data parallel)
        the side stream first waits for that parameter's all-reduce.  ``step()`` then only handles the small
        parameters and joins the side stream."""
        if self._clip_max > 0:
            raise RuntimeError("HipAdam: a clipped step (set_clip) runs its passes after the backward: no pass may start before every "
                               "gradient exists")
        self._side = torch.cuda.Stream()
        _lib.call("dd_set_adam_blocks_per_cu", 1)      # beside conv kernels: nothing queued ahead of them
        self._scale = grad_scale
        if grad_sync is not None:
            self._sync = grad_sync
        self._big_numel = big_numel
        self._hooked = set()
        if self not in ops.BACKWARD_OBSERVERS:
            ops.BACKWARD_OBSERVERS.append(self)
        self.refresh()
        lightning.on_unfreeze(self)

    def passes_last(self, on=True):
        """Where the queued optimizer passes are launched in the encoder's backward: at phase 1 of the backward (in front of c2's weight
        gradient, then its data gradient: the round-1..4 order) or, ``on``, with c2's DATA gradient first and the passes beside its
        weight gradient, which then goes last (``c2_dgrad_first``).  The rank-B passes (72 registers) fit beside the weight gradient
        only: launched in front of it they are still resident when the 475-register data gradient is dispatched, and that kernel waits
        for them CU by CU (1.9 ms from dispatch to end for 1.4 ms of work).  Same step time either way on one GPU (round 5 A/B: 7.51 /
        7.51 ms), but with the passes last the step's longest kernel runs -- and is timed -- by itself."""
        if self._side is None:
            return
        self._last = bool(on)

    # ---- what ops.BACKWARD_OBSERVERS asks of its members (registered by overlap_with_backward, removed by close) -----------------------
    @property
    def c2_dgrad_first(self):
        """The passes last, or factor mode of ddp.GradSync, where the Adam passes behind the gathered factors run beside c2's weight
        gradient: either way that kernel goes last."""
        return self._last or bool(getattr(self._sync, "factor", False))

    def backward_phase1(self):
        if not self._last:
            self._flush_pending()

    def backward_phase2(self):
        if self._last:
            self._flush_pending()
        self._flush_factored()

    def refresh(self):
        """Hook the big parameters that require a gradient and are not hooked yet: a frozen feature extractor
        (roadmap_bce_v2.py:45-47) gets its hooks when ``LightningModule.unfreeze()`` switches it on.  A big parameter
        that was never hooked is simply updated in ``step()`` with the small ones."""
        if self._side is None:
            return
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad and p.numel() >= self._big_numel and p not in self._hooked:
                    self._hooks.append(p.register_post_accumulate_grad_hook(lambda q, g=group: self._early_step(q, g)))
                    self._hooked.add(p)

    def close(self):
        """Undo overlap_with_backward: remove the gradient hooks and leave ops.BACKWARD_OBSERVERS (an optimizer that is dropped
        while another model is trained in the same process would otherwise stay registered)."""
        for h in self._hooks:
            h.remove()
        self._hooks = []
        self._hooked = set()
        for key in list(self._rankb_keys):
            if ops.RANKB.get(key) is self:
                del ops.RANKB[key]
        self._rankb, self._rankb_keys = {}, {}
        if self in ops.BACKWARD_OBSERVERS:
            ops.BACKWARD_OBSERVERS.remove(self)
        self.reset_step()
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)
        self._side = None
        self._sync = None

    # ---- global gradient norm: clipping and logging ------------------------------------------------------------------------------
    def set_clip(self, max_norm=0.0, track=False):
        """Clip every step's gradients to the global 2-norm ``max_norm`` (torch.nn.utils.clip_grad_norm_'s formula; 0: no clipping)
        and / or -- ``track`` -- only measure it.  The norm is taken over every tensor the step updates, on the device, in fp64: of a
        rank-B layer from its factors (``dd_rankb_sqnorm``: no gradient tensor is formed for it either), of the materialised gradients
        by ``dd_sqnorm`` / ``dd_sqnorm_multi``; ``dd_clip_scale`` turns the sums into {grad_scale x coef, norm, coef}, and with
        ``max_norm > 0`` every update of the step reads its scale from there (the ``_dev`` entry points): nothing comes back to the
        host.  ``grad_norm`` and ``clip_coef`` are device scalars, valid after ``step()``.  The norm is that of the gradients as Adam
        sees them (``step(grad_scale=...)`` included).
        A clipped step cannot start a pass before the last gradient exists: not with ``overlap_with_backward``.  ``track`` alone only
        reads the gradients and factors and works in either arrangement."""
        max_norm = float(max_norm or 0.0)
        if not max_norm >= 0.0:
            raise ValueError(f"HipAdam.set_clip: max_norm = {max_norm}")
        if max_norm > 0 and self._side is not None:
            raise RuntimeError("HipAdam.set_clip: with overlap_with_backward the passes of the big tensors run before the last gradient "
                               "exists; a clipped step needs the after-backward arrangement (TrainStep(adam_overlap=False))")
        self._clip_max, self._clip_track = max_norm, bool(track)

    def _measure(self, grad_scale):
        """The norm kernels of this step (on the current stream) and ``dd_clip_scale``; returns the one-element device tensor
        grad_scale x coef, or None when the step has no gradient at all.  No host synchronisation, no allocation once the buffers exist."""
        s = self._sync
        if s is not None and (getattr(s, "active", False) or getattr(s, "shard", False) or getattr(s, "factor", False)):
            raise NotImplementedError("HipAdam.set_clip: the global norm under a live GradSync (all-reduce, sharded, factor gather) is "
                                      "not implemented")
        factors = [(x, dy, has_bias) for x, dy, has_bias in self._now.held]                  # passes that already ran (track, overlap mode)
        factors += [(x, dy, bias is not None) for x, dy, bias in self._now.rankb_now.values()]
        big, small = [], []
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise RuntimeError(f"HipAdam.set_clip: a gradient of dtype {g.dtype}, contiguous={g.is_contiguous()}: the norm "
                                       "kernels take contiguous fp32 gradients")
                (big if g.numel() > self.SMALL_NUMEL else small).append(g.view(-1))
        count = len(factors) + len(big) + (1 if small else 0)
        if count == 0:
            return None
        dev = (factors[0][0] if factors else (big or small)[0]).device
        if self._slots is None or self._slots.numel() < count or self._slots.device != dev:
            self._slots = torch.zeros(max(count, 8), device=dev, dtype=torch.float64)
        if self._out3 is None or self._out3.device != dev:
            self._out3 = torch.zeros(3, device=dev, dtype=torch.float32)
            self.grad_norm, self.clip_coef = self._out3[1], self._out3[2]
        i = 0
        for x, dy, has_bias in factors:
            ops.rankb_sqnorm(dy, x, has_bias, self._slots[i:i + 1])
            i += 1
        for g in big:
            ops.sqnorm(g, self._slots[i:i + 1])
            i += 1
        if small:
            ops.sqnorm_multi(small, self._slots[i:i + 1])
            i += 1
        ops.clip_scale(self._slots[:count], self._clip_max, grad_scale, self._out3)
        return self._out3[0:1]

    def _early_step(self, p, group):
        if p.grad is not None:
            self._now.pending.append((p, group))      # launched when backward reaches its MFMA-bound stretch

    @torch.no_grad()
    def _flush_pending(self):
        if not self._now.pending:
            return
        ev = torch.cuda.current_stream().record_event()
        with torch.cuda.stream(self._side):
            self._side.wait_event(ev)
            # rank-B passes first: they only fit beside the weight gradient, the plain passes behind them also run beside the data gradient
            for p, group in self._now.pending:
                if p in self._now.rankb_now:
                    self._take_rankb(p, group, self._scale)
            for p, group in self._now.pending:
                if p in self._now.early:
                    continue
                shards = self._sync.shards(p) if self._sync is not None else None
                pieces = self._sync.pieces(p) if self._sync is not None else None
                if shards:                        # sharded optimizer: this rank's slices only, each all-gathered behind its update
                    self._update_shards(p, group, self._scale, shards)
                elif pieces:                      # the side stream (not the host) waits for the all-reduce, piece by piece
                    self._update_pieces(p, group, self._scale, pieces)
                else:
                    self._update(p, group, self._scale)
                self._now.early.add(p)
        self._now.pending = []

    @torch.no_grad()
    def step(self, grad_scale=1.0):
        if self._side is not None:
            self._flush_pending()                 # backward never reached a phase (other models)
        if self._clip_max > 0 or self._clip_track:
            scale = self._measure(grad_scale)
            if self._clip_max > 0 and scale is not None:
                grad_scale = scale                # every update below reads grad_scale x coef from the device
        for group in self.param_groups:
            small = {}                            # step count -> [(p, g, m, v)]: one launch for all the small tensors
            keeps = {}                            # step count -> [keep] of the same tensors
            for p in group["params"]:
                if p in self._now.rankb_now and p not in self._now.early:      # rank-B mode without the side stream: here, after the backward
                    self._take_rankb(p, group, grad_scale)
                    continue
                if p not in self._now.early and self._sync is not None and getattr(self._sync, "factor", False) and self._sync.has_factors(p):
                    self._update_factored(p, group, grad_scale)      # no side stream: here, after the backward
                    continue
                if p.grad is None or p in self._now.early:
                    continue
                shards = self._sync.shards(p) if self._sync is not None else None
                if shards:
                    self._update_shards(p, group, grad_scale, shards)
                    continue
                if p.numel() > self.SMALL_NUMEL or not p.grad.is_contiguous() or not p.data.is_contiguous():
                    self._update(p, group, grad_scale)
                    continue
                st = self._state_of(p)
                st["step"] += 1
                small.setdefault(st["step"], []).append((p.data.view(-1), p.grad.view(-1), st["exp_avg"].view(-1),
                                                          st["exp_avg_sq"].view(-1)))
                keeps.setdefault(st["step"], []).append(self._keep(p, group))
            b1, b2 = group["betas"]
            for step, quads in small.items():
                if all(k == 1.0 for k in keeps[step]):
                    ops.adam_step_multi(quads, group["lr"], b1, b2, group["eps"], step, grad_scale)
                else:      # biases and BatchNorm vectors ride in the same launch with 1.0
                    adamw.step_multi(quads, keeps[step], group["lr"], b1, b2, group["eps"], step, grad_scale)
        self.reset_step()                         # joins the side stream (every pass launched there is in the step's state)
