"""The learned layer mix on resident layer stacks: the mixed, padded batch straight out of the collate launch.

A ``DeviceSequenceStore(layers=L)`` keeps every sequence's ``[L, T_i, D]`` stack on the device.  Training a ``LayerMix`` on
it through ``LayerMix(h)`` would first build the padded stack ``h [B, L, T, D]``, L + 1 times the size of the batch the
classifier reads, and read it again.  Here

* ``collate_mix_batches(plans, mixes)`` assembles ``x [B, T, D] = sum_l p_l h_l`` of any number of planned batches in one
  ``rsaf_collate_mix_group`` launch per ``train_group_max()`` of them, on the autograd graph of every mix's weights;
  the backward is one ``rsaf_collate_mix_backward_group`` call for all batches that received a gradient (dL/dp from the
  resident stacks and ``dx``; the softmax Jacobian is torch's);
* ``cnnlstm_mix_train_step_group`` is the graph-free fused step (``cnnlstm_train_step_group``) over such plans: p from the
  optimizer's cache, the collate-mix launch, the classifier's step with the gradient of its input, dL/dp, and the step of
  the mix weights by ``rsaf_layer_mix_adam_group``: K replicas at a constant number of launches.

The bits are those of ``LayerMix`` on the zero-padded stack that iterating the loader yields.  ``cnnlstm`` re-exports the
names of this module.
"""
from __future__ import annotations

import torch

from . import _lib
from .cnnlstm_fused import (FusedAdam, _check_class_weights, _train_step_chunk, mix_adam_group, mix_p_group)
from .cnnlstm_train import _check_train_group, _chunks, _launch_chunked
from .device_data import BatchPlan
from .layer_mix import LayerMix


def check_mix_plans(plans, mixes, who):
    """Every plan is a ``BatchPlan`` over a store of layer stacks, every mix a ``LayerMix`` of the store's L on its device."""
    plans, mixes = list(plans), list(mixes)
    if len(plans) != len(mixes):
        raise ValueError(f"{who}: {len(plans)} plans but {len(mixes)} mixes")
    for k, (p, mix) in enumerate(zip(plans, mixes)):
        if not isinstance(p, BatchPlan):
            raise TypeError(f"{who}: plans[{k}] is a {type(p).__name__}, not a BatchPlan")
        if not isinstance(mix, LayerMix):
            raise TypeError(f"{who}: mixes[{k}] is a {type(mix).__name__}, not a LayerMix")
        store = p.dataset.store
        if p.layers is None:
            raise ValueError(f"{who}: plans[{k}] comes from a plain DeviceSequenceStore: a layer mix needs a store of layer stacks "
                             "(DeviceSequenceStore(..., layers=L))")
        if mix.num_layers != p.layers:
            raise ValueError(f"{who}: mixes[{k}] has num_layers={mix.num_layers}, but the store of plans[{k}] has layers={p.layers}")
        if mix.weights.device != store.device:
            raise ValueError(f"{who}: mixes[{k}] is on '{mix.weights.device}', but the store of plans[{k}] is on '{store.device}'")
    return plans, mixes


def _fill_addressing(it, p):
    store = p.dataset.store
    it.arena, it.arena_rows = store.arena.data_ptr(), int(store.arena.shape[0])
    it.row_start = p.row_start.data_ptr() + 8 * p.first
    it.row_count = p.row_count.data_ptr() + 4 * p.first
    it.B, it.T, it.L, it.frames = p.B, p.T, p.layers, p.frames


def _by_width(plans, members):
    """The indices ``members`` of ``plans`` by (device, width) of their stores, in order of first appearance; plans of T = 0
    left out (nothing to launch)."""
    groups = {}
    for k in members:
        p = plans[k]
        if p.T > 0:
            groups.setdefault((p.dataset.store.device, p.dataset.store.width), []).append(k)
    return groups.items()


def collate_mix_forward(plans, ps):
    """``[(x [B, T, D], labels)]`` of checked plans with the mixing probabilities ``ps[k]`` (float32 ``[L]``, contiguous, on the
    device): the forward launch alone, no graph."""
    outs = []
    for p in plans:
        store = p.dataset.store
        with torch.cuda.device(store.device):
            x = torch.empty((p.B, p.T, store.width), dtype=torch.float32, device=store.device)
            if p.T == 0:                    # members of no frames only: nothing to launch
                outs.append((x, p.dataset.labels[p.label_index[p.first:p.first + p.B]]))
            else:
                outs.append((x, torch.empty((p.B,), dtype=torch.int64, device=store.device)))

    def fill(it, k, _j):
        p = plans[k]
        _fill_addressing(it, p)
        it.p, it.out = ps[k].data_ptr(), outs[k][0].data_ptr()
        it.label_src, it.label_count = p.dataset.labels.data_ptr(), int(p.dataset.labels.numel())
        it.label_index = p.label_index.data_ptr() + 8 * p.first
        it.label_out = outs[k][1].data_ptr()

    for (device, width), members in _by_width(plans, range(len(plans))):
        with torch.cuda.device(device):
            _launch_chunked("rsaf_collate_mix_group", _lib.CollateMixItem, members, fill, width)
    return outs


def collate_mix_backward(plans, dxs):
    """``[dp [L]]`` of checked plans from the gradients ``dxs[k]`` [B, T, D] of their mixed batches (``None``: no gradient, and
    ``None`` comes back): one ``rsaf_collate_mix_backward_group`` call per ``train_group_max()`` plans of one width."""
    lib = _lib.load()
    dps, parts = [None] * len(plans), [None] * len(plans)
    live = [k for k, dx in enumerate(dxs) if dx is not None]
    for k in live:
        p = plans[k]
        device, width = p.dataset.store.device, p.dataset.store.width
        if tuple(dxs[k].shape) != (p.B, p.T, width):
            raise ValueError(f"gradient of batch {k} has shape {tuple(dxs[k].shape)}, expected {(p.B, p.T, width)}")
        if p.T == 0:
            dps[k] = torch.zeros(p.layers, dtype=torch.float32, device=device)
            continue
        n = int(lib.rsaf_layer_mix_partials(p.B, p.layers, p.T, width))
        if n < 0:
            raise ValueError(f"rsaf_layer_mix_partials refuses the shape {(p.B, p.layers, p.T, width)}")
        with torch.cuda.device(device):
            parts[k] = torch.empty(n, dtype=torch.float64, device=device)
            dps[k] = torch.empty(p.layers, dtype=torch.float32, device=device)

    def fill(it, k, _j):
        _fill_addressing(it, plans[k])
        it.dx, it.dp_out = dxs[k].data_ptr(), dps[k].data_ptr()
        it.partials, it.partials_count = parts[k].data_ptr(), parts[k].numel()

    for (device, width), members in _by_width(plans, live):
        with torch.cuda.device(device):
            _launch_chunked("rsaf_collate_mix_backward_group", _lib.CollateMixBackwardItem, members, fill, width)
    return dps


class _CollateMix(torch.autograd.Function):
    """(x_0, ..., x_K-1) of K planned batches over stores of layer stacks from the K probability vectors ``ps``; the backward
    is one group call over every batch whose output received a gradient and returns dL/dp of those.  The K label tensors
    that the same launch gathered follow the K batches in the outputs (not differentiable)."""

    @staticmethod
    def forward(ctx, plans, *ps):
        ctx.set_materialize_grads(False)
        ctx.plans = plans
        outs = collate_mix_forward(plans, ps)
        labels = tuple(lab for _, lab in outs)
        ctx.mark_non_differentiable(*labels)
        return tuple(x for x, _ in outs) + labels

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        dxs = [None if dx is None or not ctx.needs_input_grad[1 + k] else dx.to(torch.float32).contiguous()
               for k, dx in enumerate(grads[:len(ctx.plans)])]
        return (None, *collate_mix_backward(ctx.plans, dxs))


def collate_mix_batches(plans, mixes):
    """``[(x [B, T, D], labels)]`` of the planned batches of ``DeviceBatchLoader``s over stores of layer stacks, mixed by
    ``mixes[k]`` inside the collate launch: ``x = sum_l p_l h_l`` with ``p = softmax(mixes[k].weights)`` as in
    ``LayerMix.forward``, the bits of ``mixes[k](h)`` on the zero-padded stack ``h [B, L, T, D]``, which never exists.  One
    ``rsaf_collate_mix_group`` launch per ``train_group_max()`` plans of one width; ``x`` is on the autograd graph of
    ``mixes[k].weights`` (autograd applies the softmax Jacobian), and a backward in which several batches received gradients
    is one ``rsaf_collate_mix_backward_group`` call.  Under ``torch.no_grad()`` only the forward launch runs."""
    plans, mixes = check_mix_plans(plans, mixes, "collate_mix_batches")
    if not plans:
        return []
    ps = [torch.softmax(m.weights.to(torch.float32), dim=0).contiguous() for m in mixes]
    if not torch.is_grad_enabled():
        return collate_mix_forward(plans, ps)
    out = _CollateMix.apply(plans, *ps)
    return list(zip(out[:len(plans)], out[len(plans):]))


def cnnlstm_mix_train_step_group(models, mixes, optimizers, plans, masks=None, mixed=False, class_weights=None):
    """``cnnlstm_train_step_group`` over planned batches of layer stacks with a learned mix in front of every replica: one
    whole training step of K (``LayerMix``, ``CNNLSTM``) pairs, ``optimizers[k]`` the ``FusedAdam(models[k],
    layer_mix=mixes[k])``, without an autograd graph -> ``(losses [K] on the device, [logits_k])``.

    Per chunk of ``train_group_max()`` replicas: p from every optimizer's cache (no launch in steady state; one
    softmax-only launch for the group after weights were changed from outside), ONE ``rsaf_collate_mix_group`` launch, the
    step of ``cnnlstm_train_step_group`` with the backward through the ``_dx`` entries, ONE
    ``rsaf_collate_mix_backward_group`` call (two launches), the classifier's Adam and running statistics, ONE
    ``rsaf_layer_mix_adam_group`` launch (softmax Jacobian in double, Adam, the next step's p).  ``dL/dp`` of the step stays
    on the device as ``optimizers[k].last_mix_dp``.  A mix whose weights do not require a gradient is mixed but not updated.
    Arguments are checked as ``cnnlstm_train_step_group`` and ``collate_mix_batches`` check them."""
    who = "cnnlstm_mix_train_step_group"
    models, optimizers = list(models), list(optimizers)
    plans, mixes = check_mix_plans(plans, mixes, who)
    if not (len(models) == len(optimizers) == len(plans)):
        raise ValueError(f"{who}: {len(models)} models, {len(optimizers)} optimizers and {len(plans)} plans")
    for k, (m, opt, mix) in enumerate(zip(models, optimizers, mixes)):
        if not isinstance(opt, FusedAdam) or opt.model is not m:
            raise ValueError(f"{who}: optimizers[{k}] is not the FusedAdam of models[{k}]")
        if opt.layer_mix is not mix:
            raise ValueError(f"{who}: optimizers[{k}].layer_mix is not mixes[{k}] (FusedAdam(models[{k}], layer_mix=mixes[{k}]))")
    for k, p in enumerate(plans):
        if p.T == 0:
            raise ValueError(f"{who}: replica {k}: a batch of no frames")
    losses, logits = [], []
    with torch.no_grad():
        for _, chunk in _chunks(list(range(len(models)))):
            ms, opts, pls = [models[k] for k in chunk], [optimizers[k] for k in chunk], [plans[k] for k in chunk]
            ps = mix_p_group(opts)
            data = collate_mix_forward(pls, ps)
            xs, labels = [x for x, _ in data], [lab for _, lab in data]
            ms, xs, mks = _check_train_group(ms, xs, None if masks is None else [masks[k] for k in chunk], who, mixed, graph=False)
            weights = _check_class_weights(None if class_weights is None else [class_weights[k] for k in chunk], len(ms),
                                           ms[0].dims["num_classes"], xs[0].device, who) or [None] * len(ms)
            dps = []

            def dp_of(dxs):
                dps.extend(collate_mix_backward(pls, dxs))

            ls, lg = _train_step_chunk(ms, opts, xs, labels, mks, weights, mixed=mixed, with_dx=dp_of)
            for opt, dp in zip(opts, dps):
                opt.last_mix_dp = dp
            learn = [j for j, opt in enumerate(opts) if opt.layer_mix.weights.requires_grad]
            if learn:
                mix_adam_group([opts[j] for j in learn], ps=[ps[j] for j in learn], dps=[dps[j] for j in learn])
            losses.append(ls)
            logits += lg
    return (losses[0] if len(losses) == 1 else torch.cat(losses)), logits
