"""Fused training step of the CNN-LSTM: cross-entropy, Adam and the running statistics in HIP.

Around the model the reference's loop runs ``nn.CrossEntropyLoss()``, ``loss.backward()`` and ``Adam.step()``
(``src/dl_cv_strategies.py:122-125,236-248``).  Through autograd that costs, per replica and step, the packing of the
parameter blob, the unpacking of the gradient blob, the BatchNorm buffer updates and the loss and optimizer kernels of
torch: elementwise work on a few hundred thousand floats spread over 100+ small ops.  Here the blob is written from the
parameters where they live (``rsaf_cnnlstm_pack_params_group``), ``rsaf_cnnlstm_adam_group`` reads the gradient blob and
updates the parameters in their torch layouts, the loss and its gradient come from ``rsaf_ce_loss_group`` and the running
statistics from ``rsaf_bn_running_stats_group``: one launch each per group step.  In a mixed group (replicas of different
architecture, ``mixed=True``) the loss is still one launch; the packing, Adam and the running statistics, whose kernels carry
the segment table of one architecture in their arguments, take one launch per distinct architecture of the group.

Two options of the reference's users stay on this path.  Class weights (``nn.CrossEntropyLoss(weight=w)``, one ``w`` per
replica) go through ``rsaf_ce_loss_weighted_group``, still one launch.  ``FusedAdam(max_grad_norm=...)`` is
``clip_grad_norm_`` between backward and step: ``rsaf_cnnlstm_grad_norm_group`` reduces the gradient to its 2-norm over
the parameters and to the scale ``min(1, max_norm / (norm + 1e-6))``, both left on the device, and
``rsaf_cnnlstm_adam_scaled_group`` reads that scale; two more launches per group step and distinct architecture, no sync.
Without either option the launches are the ones above.

Built on ``cnnlstm_train`` (replica plan, launchers, argument checks); ``cnnlstm`` re-exports the names of this module, so
``CNNLSTM`` is imported where it is needed, not at the top.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .cnnlstm_train import (_Replica, _blob_params, _check_train_group, _chunks, _dims5, _launch_chunked, _launch_group,
                            _tracked_bn, _train_segments, _unbias, _update_running_stats, train_param_offsets)


def _adam_order(model):
    """The parameters in the numbering of ``rsaf_cnnlstm_adam_group`` (blob order; include/rsaf.h)."""
    order = _blob_params(_train_segments(model)[0])
    n = int(_lib.load().rsaf_cnnlstm_adam_param_count(*_dims5(model.dims)))
    if n != len(order) or len(order) != len(list(model.parameters())):
        raise _lib.RsafError(f"CNNLSTM has {len(list(model.parameters()))} parameters, {len(order)} of them in the blob, "
                             f"but rsaf_cnnlstm_adam_group numbers {n}")
    return order


def _pointer_table(rows, device):
    """Device int64 tensor of device pointers; the host copy travels through pinned staging on the current stream."""
    return torch.tensor(rows, dtype=torch.int64).pin_memory().to(device, non_blocking=True)


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam(model.parameters(), lr, betas, eps)`` for one ``CNNLSTM`` on the HIP path: the whole update of
    the model is one launch of ``rsaf_cnnlstm_adam_group`` (published Adam: bias-corrected moments, eps outside the
    square root; no weight decay, no amsgrad).  ``param_groups[0]['lr']`` is read at every step, so the schedulers of
    ``torch.optim.lr_scheduler`` drive it unchanged; ``state_dict()`` / ``load_state_dict()`` use ``torch.optim.Adam``'s
    format (per parameter ``step``, ``exp_avg``, ``exp_avg_sq``) in both directions.

    ``step()`` consumes ordinary ``.grad`` tensors (a parameter without one is skipped, as torch does), so the
    reference's loop works with only the optimizer swapped.  ``cnnlstm_train_step_group`` feeds the gradient blob of the
    group backward to the same kernel and never touches ``.grad``.

    The kernels reach the parameters and moments through a device table of pointers, cached while the pointers are
    stable (``.to()`` or a loaded optimizer state rebuild it).  They write through raw pointers, so after every step the
    versions of everything written are bumped: ``packed_weights()`` and every other version-keyed cache see the change.

    ``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)`` (2-norm) ahead of every
    update, by ``step()``, ``step_blob()`` and the group step alike.  The norm runs over the parameters that the step
    updates (not frozen, and with a gradient); Adam consumes ``g * min(1, max_grad_norm / (norm + 1e-6))``.  ``+inf``
    clips nothing and still reports the norm.  ``step()`` does NOT modify ``.grad``: the scale is applied where Adam reads
    the gradient.  ``last_grad_norm`` and ``last_grad_scale`` are device scalars of the last clipped step (``None`` before
    it); reading them is the caller's sync, the step itself makes none.  The option is an attribute of the optimizer,
    not an entry of ``param_groups``, which keep ``torch.optim.Adam``'s keys.

    ``layer_mix``: a ``LayerMix`` in front of the model, learned with it.  The optimizer then owns ``layer_mix.weights`` as a
    second param group with the learning rate ``layer_mix_lr`` (``None``: the classifier's ``lr``) and the same betas and eps:
    the format of ``torch.optim.Adam([{"params": model.parameters()}, {"params": [layer_mix.weights], "lr": ...}])``, which
    state dicts follow in both directions and whose two groups the schedulers scale.  ``step()`` updates the weights from
    ``weights.grad`` by one ``rsaf_layer_mix_adam_group`` launch (its ``dw`` mode), which also leaves the softmax of the new
    weights on the device (``mix_p()``); ``cnnlstm_mix_train_step_group`` feeds the same kernel ``dL/dp``.
    ``max_grad_norm`` keeps clipping over the classifier's parameters only, as ``clip_grad_norm_(model.parameters(), ...)``
    says: the mix weights are not part of the norm and are not clipped.  Without ``layer_mix`` nothing changes."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False,
                 max_grad_norm=None, layer_mix=None, layer_mix_lr=None):
        from .cnnlstm import CNNLSTM
        if not isinstance(model, CNNLSTM):
            raise ValueError(f"FusedAdam: model must be a CNNLSTM, got {type(model).__name__}")
        if weight_decay != 0:
            raise ValueError("FusedAdam: weight_decay is not supported (the reference uses Adam's default, 0)")
        if amsgrad:
            raise ValueError("FusedAdam: amsgrad is not supported")
        if maximize:
            raise ValueError("FusedAdam: maximize is not supported")
        if not 0.0 <= lr:
            raise ValueError(f"FusedAdam: invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"FusedAdam: invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdam: invalid betas: {betas}")
        _check_max_grad_norm(max_grad_norm)
        params = list(model.parameters())
        if any(not p.is_cuda for p in params):
            raise ValueError("FusedAdam: the CNNLSTM must be on a HIP device (model.to('cuda') first): there is no CPU fallback")
        if any(p.dtype != torch.float32 for p in params):
            raise ValueError("FusedAdam: the parameters must be float32")
        # the keys of torch.optim.Adam's own param_groups, so that state dicts load in both directions
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps).defaults)
        if layer_mix is None:
            if layer_mix_lr is not None:
                raise ValueError("FusedAdam: layer_mix_lr without a layer_mix")
            super().__init__(params, defaults)
        else:
            from .layer_mix import LayerMix
            if not isinstance(layer_mix, LayerMix):
                raise ValueError(f"FusedAdam: layer_mix must be a LayerMix, got {type(layer_mix).__name__}")
            w = layer_mix.weights
            if w.device != params[0].device or w.dtype != torch.float32 or not w.is_contiguous():
                raise ValueError(f"FusedAdam: layer_mix.weights must be contiguous float32 on the model's device {params[0].device}, "
                                 f"got {w.dtype} on {w.device}")
            if layer_mix_lr is not None and not 0.0 <= layer_mix_lr:
                raise ValueError(f"FusedAdam: invalid learning rate of the layer mix: {layer_mix_lr}")
            super().__init__([{"params": params}, {"params": [w], "lr": lr if layer_mix_lr is None else layer_mix_lr}], defaults)
        self.layer_mix = layer_mix
        self._mix_p = self._mix_p_key = None    # softmax of the mix weights, cached against their version
        self.last_mix_dp = None                 # dL/dp of the last fused mix step, on the device
        self.model = model
        self._order = _adam_order(model)
        self._steps = None                  # step count per parameter of _order (host mirror of state[p]['step']), None = unknown
        self._state_gen = 0                 # bumped whenever a moment tensor is created or replaced
        self._table = self._table_key = None
        self._blob = None                   # blob buffer of the fused step, rewritten from the parameters every step
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = self.last_grad_scale = None
        self._partials = None               # scratch of rsaf_cnnlstm_grad_norm_group

    # -- skip masks: bit i set = parameter i of _order sits this step out ---------------------------------------------------
    def _all_skipped(self, skip):
        return skip == (1 << len(self._order)) - 1

    def _live(self, skip):
        """The parameters that ``skip`` leaves in."""
        return [p for i, p in enumerate(self._order) if not (skip >> i) & 1]

    # -- optimizer state ------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps = None
        self._state_gen += 1

    def _hyper(self):
        g = self.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("FusedAdam: weight_decay, amsgrad and maximize are not supported")
        return float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])

    # -- the layer mix: a second param group of one parameter ----------------------------------------------------------------
    def _mix_hyper(self):
        g = self.param_groups[1]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("FusedAdam: weight_decay, amsgrad and maximize are not supported")
        return float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])

    def _mix_state(self):
        """The moments of the mix weights, created as ``torch.optim.Adam`` creates them, float32 and contiguous."""
        w = self.layer_mix.weights
        st = self.state[w]
        if "exp_avg" not in st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(w, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(w, memory_format=torch.contiguous_format)
        if not torch.is_tensor(st["step"]):
            st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
        for key in ("exp_avg", "exp_avg_sq"):
            if st[key].dtype != torch.float32 or not st[key].is_contiguous() or st[key].device != w.device:
                st[key] = st[key].to(w.device, torch.float32).contiguous()
        return st

    def _mix_p_buffer(self):
        w = self.layer_mix.weights
        if self._mix_p is None or self._mix_p.device != w.device:
            self._mix_p, self._mix_p_key = torch.empty_like(w, requires_grad=False), None
        return self._mix_p

    def _mix_p_current(self):
        """The cached softmax stands for the weights as they are (same storage, same version)."""
        w = self.layer_mix.weights
        return self._mix_p is not None and self._mix_p_key == (w.data_ptr(), w._version)

    def _mix_p_written(self):
        w = self.layer_mix.weights
        self._mix_p_key = (w.data_ptr(), w._version)

    @torch.no_grad()
    def mix_p(self):
        """``softmax(layer_mix.weights)`` as the step kernel leaves it (computed in double, rounded to float once), on the
        device.  Cached against the version counter of the weights: after a step of this optimizer it is there already;
        weights changed from outside (``load_state_dict``, ``copy_``) cost one softmax-only launch."""
        return mix_p_group([self])[0]

    def _ensure_state(self, skip):
        """Moments of every parameter that is about to be updated (created as torch.optim.Adam creates them)."""
        if self._steps is None:
            for p in self._order:
                st = self.state.get(p)
                if st and not torch.is_tensor(st["step"]):
                    st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
                if st and not (st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous()
                               and st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32):
                    st["exp_avg"] = st["exp_avg"].to(torch.float32).contiguous()
                    st["exp_avg_sq"] = st["exp_avg_sq"].to(torch.float32).contiguous()
            self._steps = [int(self.state[p]["step"]) if self.state.get(p) else 0 for p in self._order]
        for p in self._live(skip):
            if "exp_avg" not in self.state[p]:
                st = self.state[p]
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                self._state_gen += 1

    def _rows(self):
        rows = [[], [], []]
        for p in self._order:
            if not p.is_contiguous():
                raise _lib.RsafError("FusedAdam: the parameters must be contiguous")
            st = self.state.get(p) or {}
            rows[0].append(p.data_ptr())
            rows[1].append(st["exp_avg"].data_ptr() if "exp_avg" in st else 0)
            rows[2].append(st["exp_avg_sq"].data_ptr() if "exp_avg_sq" in st else 0)
        return rows

    def _cached_table(self):
        """[3][P] device table of parameter / exp_avg / exp_avg_sq pointers, cached while the pointers are stable."""
        tkey = (self._state_gen,) + tuple(p.data_ptr() for p in self._order)
        if self._table is None or self._table_key != tkey:
            self._table = _pointer_table(self._rows(), self._order[0].device)
            self._table_key = tkey
        return self._table

    def _launches(self, skip):
        """[(step, skip mask)]: one launch per distinct step count among the parameters to update (one, unless some
        parameter sat out earlier steps: torch keeps a step count per parameter)."""
        by_step = {}
        for i in range(len(self._order)):
            if not (skip >> i) & 1:
                by_step[self._steps[i] + 1] = by_step.get(self._steps[i] + 1, 0) | (1 << i)
        full = (1 << len(self._order)) - 1
        return [(t, full & ~mask) for t, mask in sorted(by_step.items())]

    def _stepped(self, skip):
        torch._foreach_add_([self.state[p]["step"] for p in self._live(skip)], 1)
        for i in range(len(self._order)):
            if not (skip >> i) & 1:
                self._steps[i] += 1

    def _frozen(self):
        skip = 0
        for i, p in enumerate(self._order):
            if not p.requires_grad:
                skip |= 1 << i
        return skip

    def _blob_buffer(self):
        """Zero-initialised buffer for the parameter blob (its padding floats are never written again)."""
        device = self._order[0].device
        if self._blob is None or self._blob.device != device:
            total = train_param_offsets(self.model.dims)[1]
            self._blob = torch.zeros(total, dtype=torch.float32, device=device)
        return self._blob

    def _partials_buffer(self):
        """Scratch for the partial sums of the gradient norm: one double per workgroup of the Adam launch."""
        device = self._order[0].device
        if self._partials is None or self._partials.device != device:
            n = int(_lib.load().rsaf_cnnlstm_grad_norm_partials(*_dims5(self.model.dims)))
            self._partials = torch.empty(n, dtype=torch.float64, device=device)
        return self._partials

    def _written(self, tensors):
        """The kernels wrote ``tensors`` through raw pointers: bump their versions, as an in-place torch op would."""
        torch.autograd.graph.increment_version(tensors)

    def packed_blob(self):
        """The parameters in the blob layout of ``rsaf_cnnlstm_train_param_offsets``, packed on the device
        (``rsaf_cnnlstm_pack_params_group``); equal to what ``_pack_train_blob`` builds with torch ops, bit for bit.
        The tensor is the optimizer's own buffer and is overwritten by the next fused step."""
        return _pack_group([self])[0]

    @torch.no_grad()
    def step_blob(self, grads):
        """One Adam step from a gradient blob in the layout of ``rsaf_cnnlstm_train_param_offsets`` (what
        ``rsaf_cnnlstm_train_backward_group`` writes); parameters with ``requires_grad = False`` are left alone (and
        left out of the norm that ``max_grad_norm`` clips)."""
        total = train_param_offsets(self.model.dims)[1]
        if not grads.is_cuda or grads.dtype != torch.float32 or grads.shape != (total,) or not grads.is_contiguous():
            raise ValueError(f"expected a contiguous float32 HIP (cuda) gradient blob of {total} floats")
        skip = self._frozen()
        if self._all_skipped(skip):
            return
        self._ensure_state(skip)
        _adam_group([(self, grads, self._cached_table(), skip)])
        self._written(self._live(skip))

    @torch.no_grad()
    def step(self, closure=None):
        """``torch.optim.Adam.step`` on the ``.grad`` tensors.  With ``max_grad_norm`` the update is the one that follows
        ``clip_grad_norm_(model.parameters(), max_grad_norm)``, but ``.grad`` itself is not modified: the norm is taken
        over the gradients where they are, and the kernel scales what it reads."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        skip, grads = 0, []
        for i, p in enumerate(self._order):
            g = p.grad
            if g is None:
                skip |= 1 << i
                grads.append(None)
                continue
            if g.is_sparse or not g.is_cuda:
                raise _lib.RsafError("FusedAdam: gradients must be dense HIP (cuda) tensors")
            grads.append(g.to(torch.float32).contiguous())
        if not self._all_skipped(skip):
            self._ensure_state(skip)
            rows = self._rows() + [[g.data_ptr() if g is not None else 0 for g in grads]]
            table = _pointer_table(rows, self._order[0].device)
            _adam_group([(self, None, table, skip)])
            self._written(self._live(skip))
        if self.layer_mix is not None and self.layer_mix.weights.grad is not None:        # as torch.optim.Adam: whatever has a .grad
            g = self.layer_mix.weights.grad
            if g.is_sparse or not g.is_cuda:
                raise _lib.RsafError("FusedAdam: gradients must be dense HIP (cuda) tensors")
            mix_adam_group([self], dws=[g.to(torch.float32).contiguous()])
        return loss


def _by_dims(records, dims_of):
    """``records`` split by the model dimensions the blob layout depends on, in order of first appearance: one list per
    distinct ``_dims5`` (a group of one architecture gives one list)."""
    parts = {}
    for rec in records:
        parts.setdefault(_dims5(dims_of(rec)), []).append(rec)
    return list(parts.items())


def _check_max_grad_norm(value):
    if value is not None and not float(value) > 0:
        raise ValueError(f"FusedAdam: max_grad_norm must be > 0 (None: no clipping; inf: the norm alone), got {value}")


def _grad_norm_group(entries):
    """Norm and clipping scale of the entries (as ``_adam_group`` takes them) whose optimizer has a ``max_grad_norm``:
    ``rsaf_cnnlstm_grad_norm_group`` once per chunk and distinct architecture, over the parameters that the entry's skip
    mask leaves in.  The results stay on the device as ``last_grad_norm`` / ``last_grad_scale`` of each optimizer."""
    clipped = [e for e in entries if e[0].max_grad_norm is not None]
    if not clipped:
        return
    out = torch.empty((len(clipped), 2), dtype=torch.float32, device=clipped[0][2].device)
    for i, (opt, _, _, _) in enumerate(clipped):
        _check_max_grad_norm(opt.max_grad_norm)
        opt.last_grad_norm, opt.last_grad_scale = out[i, 0], out[i, 1]

    def fill(it, e, _k):
        opt, grads, table, skip = e
        part = opt._partials_buffer()
        it.grads = grads.data_ptr() if grads is not None else None
        it.table, it.skip, it.max_norm = table.data_ptr(), skip, float(opt.max_grad_norm)
        it.partials, it.partials_count = part.data_ptr(), part.numel()
        it.norm_out, it.scale_out = opt.last_grad_norm.data_ptr(), opt.last_grad_scale.data_ptr()

    for dims5, part in _by_dims(clipped, lambda e: e[0].model.dims):
        _launch_chunked("rsaf_cnnlstm_grad_norm_group", _lib.GradNormItem, part, fill, *dims5)


def _adam_group(entries):
    """``entries``: [(optimizer, gradient blob or None, pointer table, skip mask)] -> ``rsaf_cnnlstm_adam_group`` in
    chunks of ``train_group_max()``, one series of launches per distinct architecture among the entries; a replica whose
    parameters stand at different step counts takes one launch per count.  Entries of optimizers with a ``max_grad_norm``
    are clipped first (``_grad_norm_group``); an architecture with such an entry goes through
    ``rsaf_cnnlstm_adam_scaled_group``, every launch of a replica reading the replica's one scale."""
    _grad_norm_group(entries)

    def fill(it, rec, _k):
        (opt, grads, table, _), (t, mask) = rec
        it.grads = grads.data_ptr() if grads is not None else None
        it.table, it.skip, it.step = table.data_ptr(), mask, t
        it.lr, it.beta1, it.beta2, it.eps = opt._hyper()

    def fill_scaled(it, rec, k):
        fill(it, rec, k)
        opt = rec[0][0]
        it.grad_scale = opt.last_grad_scale.data_ptr() if opt.max_grad_norm is not None else None

    for dims5, part in _by_dims(entries, lambda e: e[0].model.dims):
        plans = [opt._launches(skip) for opt, _, _, skip in part]
        scaled = any(opt.max_grad_norm is not None for opt, _, _, _ in part)
        for j in range(max(len(pl) for pl in plans)):
            live = [(e, pl[j]) for e, pl in zip(part, plans) if j < len(pl)]
            if scaled:
                _launch_chunked("rsaf_cnnlstm_adam_scaled_group", _lib.AdamScaledItem, live, fill_scaled, *dims5)
            else:
                _launch_chunked("rsaf_cnnlstm_adam_group", _lib.AdamItem, live, fill, *dims5)
    for opt, _, _, skip in entries:
        opt._stepped(skip)


def _check_mix_owners(optimizers, who):
    for k, opt in enumerate(optimizers):
        if not isinstance(opt, FusedAdam) or opt.layer_mix is None:
            raise ValueError(f"{who}: optimizers[{k}] is not a FusedAdam that owns a layer mix (FusedAdam(model, layer_mix=...))")


@torch.no_grad()
def mix_p_group(optimizers):
    """``[opt.mix_p()]`` of the optimizers: the cached softmax of every mix's weights; those whose weights changed since it
    was written (another version or storage) are brought up to date together by one softmax-only launch of
    ``rsaf_layer_mix_adam_group`` per ``train_group_max()`` of them.  In steady state no launch at all."""
    optimizers = list(optimizers)
    _check_mix_owners(optimizers, "mix_p_group")
    stale = [opt for opt in optimizers if not opt._mix_p_current()]

    def fill(it, opt, _k):
        w = opt.layer_mix.weights
        it.L, it.mode = w.numel(), _lib.LAYER_MIX_SOFTMAX_ONLY
        it.w, it.p_next = w.data_ptr(), opt._mix_p_buffer().data_ptr()

    if stale:
        _launch_chunked("rsaf_layer_mix_adam_group", _lib.LayerMixAdamItem, stale, fill)
        for opt in stale:
            opt._mix_p_written()
    return [opt._mix_p for opt in optimizers]


@torch.no_grad()
def mix_adam_group(optimizers, ps=None, dps=None, dws=None, dw_outs=None):
    """One Adam step of the mix weights of K optimizers in one ``rsaf_layer_mix_adam_group`` launch (per
    ``train_group_max()`` of them).  Either ``ps`` and ``dps`` (float32 ``[L]`` device tensors: the kernel applies the softmax
    Jacobian in double; ``dw_outs[k]``, where given, receives the gradient it formed) or ``dws`` (the gradient of the
    weights as it is).  The launch leaves the softmax of the new weights in every optimizer's ``mix_p()`` buffer."""
    optimizers = list(optimizers)
    _check_mix_owners(optimizers, "mix_adam_group")
    if (dws is None) == (ps is None or dps is None):
        raise ValueError("mix_adam_group: give either ps and dps, or dws")
    states = [opt._mix_state() for opt in optimizers]

    def fill(it, k, _j):
        opt, st = optimizers[k], states[k]
        w = opt.layer_mix.weights
        it.L = w.numel()
        if dws is None:
            it.mode, it.p, it.dp = _lib.LAYER_MIX_FROM_DP, ps[k].data_ptr(), dps[k].data_ptr()
            it.dw_out = dw_outs[k].data_ptr() if dw_outs is not None and dw_outs[k] is not None else None
        else:
            it.mode, it.dw = _lib.LAYER_MIX_FROM_DW, dws[k].data_ptr()
        it.w, it.exp_avg, it.exp_avg_sq = w.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        it.p_next = opt._mix_p_buffer().data_ptr()
        it.lr, it.beta1, it.beta2, it.eps = opt._mix_hyper()
        it.step = int(st["step"]) + 1

    _launch_chunked("rsaf_layer_mix_adam_group", _lib.LayerMixAdamItem, list(range(len(optimizers))), fill)
    torch._foreach_add_([st["step"] for st in states], 1)
    for opt, st in zip(optimizers, states):
        opt._written([opt.layer_mix.weights, st["exp_avg"], st["exp_avg_sq"]])
        opt._mix_p_written()


def _pack_group(optimizers):
    """The parameter blobs of the optimizers' models, written on the device from the parameters where they live: one
    launch of ``rsaf_cnnlstm_pack_params_group`` per chunk of ``train_group_max()`` and distinct architecture."""
    pairs = [(opt._cached_table(), opt._blob_buffer(), opt.model.dims) for opt in optimizers]

    def fill(it, pair, _k):
        it.table, it.params = pair[0].data_ptr(), pair[1].data_ptr()

    for dims5, part in _by_dims(pairs, lambda pair: pair[2]):
        _launch_chunked("rsaf_cnnlstm_pack_params_group", _lib.PackItem, part, fill, *dims5)
    return [blob for _, blob, _ in pairs]


def _check_class_weights(weights, K, nc, device, who):
    """``weights`` of a group call as a list of K contiguous float32 ``[nc]`` tensors on ``device`` or ``None`` entries; a
    list of ``None`` alone comes back as ``None`` (the unweighted entry is called)."""
    if weights is None:
        return None
    weights = list(weights)
    if len(weights) != K:
        raise ValueError(f"{who}: {K} items but {len(weights)} class-weight entries")
    for k, w in enumerate(weights):
        if w is None:
            continue
        if not torch.is_tensor(w) or w.dtype != torch.float32 or w.shape != (nc,) or w.device != device:
            what = f"{w.dtype} {tuple(w.shape)} on {w.device}" if torch.is_tensor(w) else type(w).__name__
            raise ValueError(f"{who}: item {k}: class weights must be a float32 tensor [{nc}] on {device}, got {what}")
    if all(w is None for w in weights):
        return None
    return [w if w is None else w.contiguous() for w in weights]


def ce_loss_group(logits, labels, with_grad=True, weights=None):
    """Mean-reduced cross-entropy of K (logits [B_k, nc], int64 labels [B_k]) pairs in one launch of
    ``rsaf_ce_loss_group`` (``nn.CrossEntropyLoss()`` with its defaults) -> (losses [K] on the device, list of
    d loss_k / d logits_k, or None without ``with_grad``).  Lists longer than ``train_group_max()`` are chunked.

    ``weights``: per item a float32 ``[nc]`` device tensor of class weights (``nn.CrossEntropyLoss(weight=w)``: the mean is
    the one weighted by ``w[label]``) or ``None``; the call is then one launch of ``rsaf_ce_loss_weighted_group``, in which
    an item without weights gets the bits of the unweighted entry.  With no weights at all that entry itself is called."""
    logits, labels = list(logits), list(labels)
    if len(logits) != len(labels) or not logits:
        raise ValueError(f"{len(logits)} logits but {len(labels)} label tensors")
    nc, device = logits[0].shape[1], logits[0].device
    weights = _check_class_weights(weights, len(logits), nc, device, "ce_loss_group")
    labs = []
    for k, (o, lab) in enumerate(zip(logits, labels)):
        if not o.is_cuda:
            raise _lib.RsafError(f"ce_loss_group needs HIP (cuda) tensors (item {k}): there is no CPU fallback")
        if o.dim() != 2 or o.shape[1] != nc or o.dtype != torch.float32 or not o.is_contiguous():
            raise ValueError(f"item {k}: expected contiguous float32 logits [B, {nc}], got {o.dtype} {tuple(o.shape)}")
        if lab.dim() != 1 or lab.shape[0] != o.shape[0] or lab.dtype.is_floating_point:
            raise ValueError(f"item {k}: expected {o.shape[0]} integer class labels, got {lab.dtype} {tuple(lab.shape)}")
        labs.append(lab.to(device, torch.int64).contiguous())
    losses = torch.empty(len(logits), dtype=torch.float32, device=device)
    dl = [torch.empty_like(o) for o in logits] if with_grad else None

    def fill(it, pair, k):
        it.logits, it.labels, it.B = pair[0].data_ptr(), pair[1].data_ptr(), pair[0].shape[0]
        it.loss_out = losses.data_ptr() + 4 * k
        it.dlogits_out = dl[k].data_ptr() if with_grad else None

    def fill_weighted(it, rec, k):
        fill(it, rec, k)
        it.class_weight = rec[2].data_ptr() if rec[2] is not None else None

    if weights is None:
        _launch_chunked("rsaf_ce_loss_group", _lib.CeLossItem, list(zip(logits, labs)), fill, nc)
    else:
        _launch_chunked("rsaf_ce_loss_weighted_group", _lib.CeLossWeightedItem, list(zip(logits, labs, weights)), fill_weighted, nc)
    return losses, dl


def _bn_running_group(reps):
    """Running statistics of the replicas ``reps`` (``_Replica`` records) after a step: one launch of
    ``rsaf_bn_running_stats_group`` per chunk and distinct channel count, ``num_batches_tracked`` incremented on the host
    side in one foreach op.
    A replica with a ``momentum=None`` layer (cumulative average) takes the torch ops of ``_update_running_stats``.
    Returns the buffers written."""
    fused, counters, written = [], [], []
    for r in reps:
        bns = [bn for _, bn, _ in _tracked_bn(r.model, r.B, r.T)]
        written += [t for bn in bns for t in (bn.running_mean, bn.running_var)]
        if any(bn.momentum is None for bn in bns):
            _update_running_stats(r.model, r.stats, r.B, r.T)
        elif bns:
            fused.append(r)
            counters += [bn.num_batches_tracked for bn in bns]

    def fill(it, r, _k):
        it.stats = r.stats.data_ptr()
        for i, bn, n in _tracked_bn(r.model, r.B, r.T):
            if not (bn.running_mean.is_contiguous() and bn.running_var.is_contiguous()
                    and bn.running_mean.dtype == bn.running_var.dtype == torch.float32):
                raise _lib.RsafError("the BatchNorm running statistics must be contiguous float32 tensors")
            it.running_mean[i], it.running_var[i] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
            it.momentum[i], it.unbias[i] = float(bn.momentum), _unbias(n)

    by_channels = {}
    for r in fused:
        by_channels.setdefault(r.model.dims["channels"], []).append(r)
    for channels, part in by_channels.items():
        _launch_chunked("rsaf_bn_running_stats_group", _lib.BnRunningItem, part, fill, channels)
    if counters:
        torch._foreach_add_(counters, 1)
    return written


def _train_step_chunk(models, optimizers, xs, labels, masks, weights, mixed=False, with_dx=None):
    """The fused step of up to ``train_group_max()`` replicas -> (losses [K], [logits_k]).  The statistics and gradient
    blobs of the replicas are slices of one allocation each, of every replica's own size (in a mixed group the channel
    count and the blob length differ; every size is a multiple of 4 floats, so the slices stay 16-byte aligned).
    ``with_dx``: a callable; the backward then returns the gradient of every input too (the ``_dx`` entries), and
    ``with_dx([dx_k])`` runs between the backward and Adam (the fused mix step: dL/dp from the resident stacks)."""
    device = xs[0].device
    nc = models[0].dims["num_classes"]
    rows = [x.shape[0] for x in xs]
    logits_all = torch.empty((sum(rows), nc), dtype=torch.float32, device=device)
    logits = list(torch.split(logits_all, rows))
    stats = [t.view(5, 3, -1) for t in torch.split(torch.empty(sum(15 * m.dims["channels"] for m in models), dtype=torch.float32,
                                                               device=device), [15 * m.dims["channels"] for m in models])]
    blobs = _pack_group(optimizers)
    reps = [_Replica(model, x, mk, blobs[k], logits[k], stats[k]) for k, (model, x, mk) in enumerate(zip(models, xs, masks))]
    _launch_group(reps, False, mixed)
    losses, dl = ce_loss_group(logits, labels, weights=weights)
    sizes = [b.numel() for b in blobs]
    grads = torch.split(torch.zeros(sum(sizes), dtype=torch.float32, device=device), sizes)     # one zero fill for the group
    for k, r in enumerate(reps):
        r.dlogits, r.grads = dl[k], grads[k]
        if with_dx is not None:
            r.want_dx()
    _launch_group(reps, True, mixed)
    if with_dx is not None:
        with_dx([r.dx for r in reps])
    entries = []
    for k, opt in enumerate(optimizers):
        skip = opt._frozen()
        opt._ensure_state(skip)
        entries.append((opt, grads[k], opt._cached_table(), skip))
    live = [e for e in entries if not e[0]._all_skipped(e[3])]
    if live:
        _adam_group(live)
    buffers = _bn_running_group(reps)
    for opt, _, _, skip in entries:
        own = set(id(t) for t in opt.model.buffers())
        opt._written(opt._live(skip) + [t for t in buffers if id(t) in own])
    return losses, logits


def cnnlstm_train_step_group(models, optimizers, xs, labels, masks=None, mixed=False, class_weights=None):
    """One whole training step of K independent ``CNNLSTM`` replicas, ``optimizers[k]`` the ``FusedAdam`` of ``models[k]``:
    group forward in training mode, ``nn.CrossEntropyLoss()`` (defaults) of ``labels[k]``, group backward, Adam and the
    BatchNorm running statistics -> ``(losses [K] on the device, [logits_k])``.  No autograd graph is built and ``.grad``
    is not touched (an input that requires a gradient is a ``ValueError``: ``cnnlstm_train_group`` returns it); the packing of
    the parameter blobs, the loss, the optimizer and the running statistics are one launch each for the group.  A parameter with ``requires_grad = False`` keeps its value and its moments.

    Arguments are checked as ``cnnlstm_train_group`` checks them; ``masks`` as there (``forced_masks`` and
    ``dropout_stream`` are honoured, and masks from torch's RNG are drawn replica by replica in the same order, so with
    equal RNG state both paths see equal masks).  Lists longer than ``train_group_max()`` are split into chunks of that
    size, in list order.

    ``mixed=True``: replicas of different architecture, as in ``cnnlstm_train_group``.  Forward and backward of a chunk are
    one mixed call each and the loss stays one launch; the packing, Adam and the running statistics run once per distinct
    architecture of the chunk.  Results equal those of one group step per architecture, bit for bit.

    ``class_weights``: one entry per replica, a float32 ``[num_classes]`` device tensor (the ``weight`` of
    ``nn.CrossEntropyLoss``) or ``None``.  An optimizer with ``max_grad_norm`` clips its replica's gradient by its norm ahead
    of Adam (``FusedAdam``); norm and scale stay on the device (``last_grad_norm``, ``last_grad_scale``).  Both are per
    replica: the results of a replica do not depend on what the others of the group use."""
    optimizers, labels = list(optimizers), list(labels)
    models, xs, mks = _check_train_group(models, xs, masks, "cnnlstm_train_step_group", mixed, graph=False)
    if not (len(optimizers) == len(labels) == len(models)):
        raise ValueError(f"{len(models)} models, {len(optimizers)} optimizers and {len(labels)} label tensors")
    for k, (m, opt) in enumerate(zip(models, optimizers)):
        if not isinstance(opt, FusedAdam) or opt.model is not m:
            raise ValueError(f"optimizers[{k}] is not the FusedAdam of models[{k}]")
    for k, (x, lab) in enumerate(zip(xs, labels)):
        if lab.dim() != 1 or lab.shape[0] != x.shape[0] or lab.dtype.is_floating_point:
            raise ValueError(f"replica {k}: expected {x.shape[0]} integer class labels, got {lab.dtype} {tuple(lab.shape)}")
    weights = _check_class_weights(class_weights, len(models), models[0].dims["num_classes"], xs[0].device, "cnnlstm_train_step_group")
    if weights is None:
        weights = [None] * len(models)
    losses, logits = [], []
    with torch.no_grad():
        # every chunk is a whole step of its replicas, so the chunks are cut here and not call by call
        for _, chunk in _chunks(list(zip(models, optimizers, xs, labels, mks, weights))):
            ls, lg = _train_step_chunk(*zip(*chunk), mixed=mixed)
            losses.append(ls)
            logits += lg
    return (losses[0] if len(losses) == 1 else torch.cat(losses)), logits


def _loss_list(loss_fn, K):
    """``loss_fn`` of the lockstep loops as K losses: one loss for all replicas, or a sequence of K (per-fold weights)."""
    if isinstance(loss_fn, (list, tuple)):
        if len(loss_fn) != K:
            raise ValueError(f"{K} replicas but {len(loss_fn)} losses")
        return list(loss_fn)
    return [loss_fn] * K


def _fused_loss(loss_fn, model):
    """``nn.CrossEntropyLoss`` with its default options, or with those and a ``weight`` the kernel can read as it is: a
    float32 ``[num_classes]`` tensor on the model's device."""
    if type(loss_fn) is not nn.CrossEntropyLoss or loss_fn.reduction != "mean" \
            or loss_fn.label_smoothing != 0 or loss_fn.ignore_index != -100:
        return False
    w = loss_fn.weight
    if w is None:
        return True
    return (torch.is_tensor(w) and w.dtype == torch.float32 and w.shape == (model.dims["num_classes"],)
            and w.device == next(model.parameters()).device)


def _class_weights(loss_fns):
    """The ``weight`` tensors of the losses for ``class_weights=``, or ``None`` when no loss has one."""
    weights = [fn.weight for fn in loss_fns]
    return None if all(w is None for w in weights) else weights


def _fused_step_applies(optimizers, models, loss_fn):
    """The lockstep loops take the fused step when the loss (every loss of a sequence of K) is ``nn.CrossEntropyLoss``
    with its default options, or with those and a float32 ``[num_classes]`` ``weight`` on the model's device, and every
    optimizer is the ``FusedAdam`` of its model."""
    models = list(models)
    if not all(_fused_loss(fn, m) for fn, m in zip(_loss_list(loss_fn, len(models)), models)):
        return False
    return all(isinstance(o, FusedAdam) and o.model is m for o, m in zip(optimizers, models))
