"""Training and evaluation loops of the reference for K CNN-LSTM replicas in lock step (``CNNLSTMGroup``,
``train_replicas_lockstep``, ``eval_replicas_lockstep``, ``train_eval_replicas_lockstep``): every step of the loops is
one group call of ``cnnlstm_train`` / ``cnnlstm_fused`` (training) or of ``cnnlstm.cnnlstm_forward_group`` (validation).

``cnnlstm`` re-exports the names of this module, so what the loops need of it (``CNNLSTM``, ``cnnlstm_forward_group``,
``eval_outputs``) is imported where it is used, not at the top.
"""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.nn as nn

from .cnnlstm_fused import FusedAdam, _class_weights, _fused_step_applies, _loss_list, ce_loss_group, cnnlstm_train_step_group
from .cnnlstm_train import cnnlstm_train_group, train_group_max
from .device_data import BatchPlan, DeviceBatchLoader, batches_to_device, check_loader_devices, epoch_iterator
from .layer_mix import LayerMix
from .layer_mix_train import cnnlstm_mix_train_step_group, collate_mix_batches


def _check_mixes(loaders, mixes, who):
    """``mixes`` of a lock-step loop as a list of K ``LayerMix`` or ``None``: a replica with a mix needs a
    ``DeviceBatchLoader`` over a store of layer stacks of the mix's L, and such a loader needs a mix."""
    K = len(loaders)
    mixes = [None] * K if mixes is None else list(mixes)
    if len(mixes) != K:
        raise ValueError(f"{who}: {K} loaders but {len(mixes)} mixes")
    for k, (ld, mix) in enumerate(zip(loaders, mixes)):
        layers = ld.dataset.store.layers if isinstance(ld, DeviceBatchLoader) else None
        if mix is None:
            if layers is not None:
                raise ValueError(f"{who}: loader {k} is a DeviceBatchLoader over a store of layer stacks (layers={layers}), "
                                 f"but mixes[{k}] is None: such a loader needs a LayerMix({layers})")
            continue
        if not isinstance(mix, LayerMix):
            raise TypeError(f"{who}: mixes[{k}] is a {type(mix).__name__}, not a LayerMix")
        if layers is None:
            raise ValueError(f"{who}: mixes[{k}] is a LayerMix, but loader {k} is not a DeviceBatchLoader over a store of layer "
                             "stacks (DeviceSequenceStore(..., layers=L))")
        if mix.num_layers != layers:
            raise ValueError(f"{who}: mixes[{k}] has num_layers={mix.num_layers}, but the store of loader {k} has layers={layers}")
    return mixes


def _assemble(batches, mixes, device):
    """``batches_to_device`` for batches of which some are plans over stores of layer stacks (``mixes[k]`` not ``None``):
    those are mixed inside one collate-mix launch per group (``collate_mix_batches``), the others assembled as before."""
    mixed_k = [k for k, m in enumerate(mixes) if m is not None]
    if not mixed_k:
        return batches_to_device(batches, device)
    plain_k = [k for k, m in enumerate(mixes) if m is None]
    out = [None] * len(batches)
    for k, xb in zip(plain_k, batches_to_device([batches[k] for k in plain_k], device) if plain_k else []):
        out[k] = xb
    for k, xb in zip(mixed_k, collate_mix_batches([batches[k] for k in mixed_k], [mixes[k] for k in mixed_k])):
        out[k] = xb
    return out


class CNNLSTMGroup(nn.Module):
    """K ``CNNLSTM`` replicas of one architecture (``mixed=True``: of any mix of architectures that share ``input_dim``,
    ``num_classes`` and ``lstm_layers``) that train side by side.  ``forward(xs)`` takes one batch per replica
    (``None``: the replica sits out and its output is ``None``): in training mode the group step over the others, in
    eval mode the group inference forward over them (``cnnlstm_forward_group``).  ``state_dict`` keys are ``models.<k>.<reference key>``, so a
    replica's weights load into a plain ``CNNLSTM``."""

    def __init__(self, models, mixed=False):
        from .cnnlstm import CNNLSTM
        super().__init__()
        self.models = nn.ModuleList(models)
        self.mixed = bool(mixed)
        if len(self.models) == 0:
            raise ValueError("CNNLSTMGroup needs at least one replica")
        for k, m in enumerate(self.models):
            if not isinstance(m, CNNLSTM):
                raise TypeError(f"replica {k} is a {type(m).__name__}, not a CNNLSTM")

    def forward(self, xs):
        from .cnnlstm import cnnlstm_forward_group
        xs = list(xs)
        if len(xs) != len(self.models):
            raise ValueError(f"{len(self.models)} replicas but {len(xs)} inputs")
        live = [k for k, x in enumerate(xs) if x is not None]
        outs = [None] * len(xs)
        if self.training:
            if live:
                for k, o in zip(live, cnnlstm_train_group([self.models[k] for k in live], [xs[k] for k in live], mixed=self.mixed)):
                    outs[k] = o
        elif live:
            for k, o in zip(live, cnnlstm_forward_group([self.models[k] for k in live], [xs[k] for k in live], mixed=self.mixed)):
                outs[k] = o
        return outs


def train_replicas_lockstep(models, optimizers, loaders, loss_fn, epochs, device, mixed=False, mixes=None):
    """The reference's inner training loop (``src/dl_cv_strategies.py:244-248``: ``zero_grad / model(seq) / loss /
    backward / step`` per batch, a fixed number of epochs) for K replicas over K loaders in lock step: step i of an
    epoch takes batch i of every loader through one group step.  Loaders may differ in length; a replica whose epoch
    is exhausted sits out until the others finish theirs.  Returns the mean training loss per epoch of every replica
    (``histories[k][epoch]``, accumulated as the reference's ``train_model`` does, ``:120-129``); the K losses of a
    step come to the host in one copy.

    Parameters, buffers and losses equal those of K sequential trainings bit for bit as long as the replicas see the
    same batches and dropout masks.  When ``loss_fn`` is ``nn.CrossEntropyLoss()`` with its default options and every
    optimizer of the call is the ``FusedAdam`` of its model, a step is one ``cnnlstm_train_step_group`` call (loss, Adam and running
    statistics in HIP, no autograd graph); anything else runs the loop above as written.  ``loss_fn`` may be a sequence of K
    losses, one per replica (class weights of every fold's own balance); a ``weight`` that is a float32 ``[num_classes]``
    tensor on the model's device keeps the fused step, and the decision is taken over all K losses.  ``FusedAdam(max_grad_norm=...)``
    clips the gradient by its norm on both paths (in the fused step, and in ``FusedAdam.step()`` on the autograd loop).  Note that ``DataLoader(shuffle=True)`` without a ``generator`` of its own draws
    its permutations from torch's global RNG: in lock step the K loaders draw in a different order than K sequential
    trainings would, so give every loader its own ``torch.Generator`` where the batch order matters.  Dropout masks
    of a model that carries a ``DropoutStream`` (``model.dropout_stream``) are a function of the stream's seed and of the
    number of steps the model has taken, so they are those of its sequential training whatever the grouping, and a
    replica that sits out a step does not advance its stream.  Without a stream the masks come from torch's device RNG
    replica by replica within a step, in another order than K sequential trainings draw them.

    ``mixed=True``: the replicas may differ in architecture (``cnnlstm_train_group``): several trials of a hyper-parameter
    search, each with its folds, in one lock-step training.

    Any loader may be a ``device_data.DeviceBatchLoader`` (sequences resident on the device) in place of a ``DataLoader``,
    in any mix: the batches that such loaders contribute to a group step are assembled on the device by one
    ``rsaf_collate_pad_group`` launch (per ``train_group_max()`` of them), in the ``DataLoader``'s order and with
    ``collate_fn``'s bits, so the results are the same.  ``DataLoader`` entries are padded on the host and copied as before.

    ``mixes``: a sequence of K ``LayerMix`` or ``None`` entries (``None`` for the argument: no replica has one, and the loop is
    what it was).  A replica with a mix learns it in front of its model; its loader must be a ``DeviceBatchLoader`` over a
    store of layer stacks of the mix's L (``DeviceSequenceStore(..., layers=L)``), and such a loader needs a mix: both are
    refused by name before the first step.  The mixed batches come straight out of the collate launch.  When the fused
    step applies (above) and every mixed replica's optimizer owns its mix (``FusedAdam(model, layer_mix=mix)``), the mixed
    replicas of a step take one ``cnnlstm_mix_train_step_group`` call and the others one ``cnnlstm_train_step_group``
    call; otherwise the mixed replicas run the autograd loop over ``collate_mix_batches``, where ``optimizers[k].step()``
    must be the one that updates the mix (a ``FusedAdam(layer_mix=...)`` or any optimizer over both parameter sets); a
    ``FusedAdam`` that does not own its replica's mix would leave it where it started and is refused by name."""
    models, optimizers, loaders = list(models), list(optimizers), list(loaders)
    if not (len(models) == len(optimizers) == len(loaders)):
        raise ValueError(f"{len(models)} models, {len(optimizers)} optimizers and {len(loaders)} loaders")
    check_loader_devices(loaders, device, "train_replicas_lockstep")
    mixes = _check_mixes(loaders, mixes, "train_replicas_lockstep")
    for k, (opt, mix) in enumerate(zip(optimizers, mixes)):
        if mix is not None and isinstance(opt, FusedAdam) and opt.layer_mix is not mix:      # its step() would never move the mix
            raise ValueError(f"train_replicas_lockstep: optimizers[{k}] is a FusedAdam that does not own mixes[{k}], so the mix would "
                             f"never be updated: build it as FusedAdam(models[{k}], layer_mix=mixes[{k}])")
    histories = [[] for _ in models]
    loss_fns = _loss_list(loss_fn, len(models))
    fused = _fused_step_applies(optimizers, models, loss_fns)     # decided once for the call: no replica changes path mid-epoch
    weights = _class_weights(loss_fns) if fused else None
    # the mixed replicas take the fused mix step when the fused step applies and every one's optimizer owns its mix
    fused_mix = fused and all(opt.layer_mix is mix for opt, mix in zip(optimizers, mixes) if mix is not None)

    def autograd_step(ks, xs, labs):
        for k in ks:
            optimizers[k].zero_grad()
        outs = cnnlstm_train_group([models[k] for k in ks], xs, mixed=mixed)
        losses = [loss_fns[k](o, lab) for k, o, lab in zip(ks, outs, labs)]
        torch.stack(losses).sum().backward()
        for k in ks:
            optimizers[k].step()
        return torch.stack([ls.detach() for ls in losses])

    def fused_step(ks, xs, labs):
        return cnnlstm_train_step_group([models[k] for k in ks], [optimizers[k] for k in ks], xs, labs, mixed=mixed,
                                        class_weights=weights and [weights[k] for k in ks])[0]

    for _ in range(epochs):
        for m in models:
            m.train()
        its = [epoch_iterator(ld) for ld in loaders]
        total, count = [0.0] * len(models), [0] * len(models)
        while True:
            batches = [next(it, None) for it in its]
            live = [k for k, b in enumerate(batches) if b is not None]
            if not live:
                break
            with_mix = [k for k in live if mixes[k] is not None]
            if not with_mix:
                xs, labs = zip(*batches_to_device([batches[k] for k in live], device))
                step_losses = (fused_step if fused else autograd_step)(live, list(xs), list(labs))
            elif fused_mix:                     # each kind takes its own step function
                plain = [k for k in live if mixes[k] is None]
                parts = []
                if plain:
                    xs, labs = zip(*batches_to_device([batches[k] for k in plain], device))
                    parts.append(fused_step(plain, list(xs), list(labs)))
                parts.append(cnnlstm_mix_train_step_group(
                    [models[k] for k in with_mix], [mixes[k] for k in with_mix], [optimizers[k] for k in with_mix],
                    [batches[k] for k in with_mix], mixed=mixed, class_weights=weights and [weights[k] for k in with_mix])[0])
                live = plain + with_mix
                step_losses = torch.cat(parts)
            else:                               # the autograd loop over collate_mix_batches
                plain = [k for k in live if mixes[k] is None]
                parts = []
                if plain and fused:
                    xs, labs = zip(*batches_to_device([batches[k] for k in plain], device))
                    parts.append(fused_step(plain, list(xs), list(labs)))
                    rest = with_mix
                else:
                    rest = list(live)
                xs, labs = zip(*_assemble([batches[k] for k in rest], [mixes[k] for k in rest], device))
                parts.append(autograd_step(rest, list(xs), list(labs)))
                live = (plain if plain and fused else []) + rest
                step_losses = torch.cat(parts)
            for k, v in zip(live, step_losses.tolist()):
                total[k] += v
                count[k] += 1
        for k in range(len(models)):
            histories[k].append(total[k] / max(count[k], 1))
    return histories


def _eval_pairs(tagged):
    """``tagged``: iterable of ``(tag, model, loader, mix)`` -> the ``(tag, model, seq, lab, mix)`` of ``_grouped_eval_batches``,
    loader by loader; a ``DeviceBatchLoader`` gives its batches as plans."""
    for tag, model, ld, mix in tagged:
        for b in epoch_iterator(ld):
            yield (tag, model, b, None, mix) if isinstance(b, BatchPlan) else (tag, model, b[0], b[1], mix)


def _grouped_eval_batches(pairs, device, mixed=False):
    """``pairs``: iterable of ``(tag, model, seq, lab, mix)`` in any mix of models (``mixed``: of architectures too) -> yields ``(tag, logits, lab on the device)``
    in the same order, the forwards pooled into group calls of up to ``train_group_max()`` batches.  The batches stay as
    collated: zero padding is not masked (``src/dl_cv_strategies.py:81-84``), so regrouping sequences would change the
    results.  ``seq`` may be a ``BatchPlan`` of a device loader (``lab`` is then ignored): the plans of a group call are
    assembled by one ``rsaf_collate_pad_group`` launch; those over stores of layer stacks (``mix`` not ``None``) are mixed by
    one ``rsaf_collate_mix_group`` launch per group call, the forward launch alone."""
    from .cnnlstm import cnnlstm_forward_group
    gmax = train_group_max()
    pend = []

    def flush():
        data = _assemble([p[2] for p in pend], [p[3] for p in pend], device)
        outs = cnnlstm_forward_group([p[1] for p in pend], [x for x, _ in data], mixed=mixed)
        res = [(p[0], o, lab) for p, o, (_, lab) in zip(pend, outs, data)]
        pend.clear()
        return res

    for tag, model, seq, lab, mix in pairs:
        pend.append((tag, model, seq if isinstance(seq, BatchPlan) else (seq, lab), mix))
        if len(pend) == gmax:
            yield from flush()
    if pend:
        yield from flush()


def eval_replicas_lockstep(models, loaders, device, mixed=False, mixes=None):
    """``_eval_model`` (``src/dl_cv_strategies.py:183-194``) for K models over K loaders: all (model, batch) pairs are
    pooled into group calls.  Returns K triples ``(labels, preds, probs)`` of NumPy arrays in loader order, equal to
    what the reference's loop returns model by model; the results of a replica come to the host in one copy each.
    ``mixed=True``: the models may differ in architecture (``cnnlstm_forward_group``).  Loaders may be
    ``DeviceBatchLoader``s in any mix with ``DataLoader``s; their batches are assembled on the device, one launch per group call.
    ``mixes``: as in ``train_replicas_lockstep``; the batches of a replica with a mix are mixed inside the collate launch with
    ``p = softmax(weights)`` as ``LayerMix.forward`` forms it (the forward launch alone, one per group call), so the logits are
    those of the model on ``mix(h)`` of the zero-padded stack."""
    from .cnnlstm import eval_outputs
    models, loaders = list(models), list(loaders)
    if len(models) != len(loaders):
        raise ValueError(f"{len(models)} models but {len(loaders)} loaders")
    check_loader_devices(loaders, device, "eval_replicas_lockstep")
    mixes = _check_mixes(loaders, mixes, "eval_replicas_lockstep")
    for m in models:
        m.eval()
    parts = [([], [], []) for _ in models]
    with torch.no_grad():
        pairs = _eval_pairs((k, m, ld, mix) for k, (m, ld, mix) in enumerate(zip(models, loaders, mixes)))
        for k, out, lab in _grouped_eval_batches(pairs, device, mixed):
            prob, pred = eval_outputs(out)
            for lst, v in zip(parts[k], (lab, pred, prob)):
                lst.append(v)
    res = []
    for labs, preds, probs in parts:
        if not labs:
            res.append((np.array([]), np.array([]), np.array([])))
            continue
        res.append(tuple(torch.cat(v).cpu().numpy() for v in (labs, preds, probs)))
    return res


def eval_model_grouped(model, data_loader, device):
    """``_eval_model`` (``src/dl_cv_strategies.py:183-194``) with all batches of the loader as items of group calls:
    ``(labels, preds, probs)`` as NumPy arrays in loader order."""
    return eval_replicas_lockstep([model], [data_loader], device)[0]


def train_eval_replicas_lockstep(models, optimizers, schedulers, train_loaders, val_loaders, loss_fn, epochs, patience, device,
                                 mixed=False, mixes=None):
    """``_train_eval_loop`` (``src/dl_cv_strategies.py:112-165``) for K replicas: per epoch the training pass of
    ``train_replicas_lockstep`` over the replicas still running, then the validation pass of all of them in group calls
    (``val_loss`` accumulated batch by batch in loader order; the losses of a pass come to the host in one copy), then per
    replica ``scheduler.step(avg_val_loss)`` (``schedulers[k]`` may be ``None``), best-weights checkpointing and early
    stopping as the reference does them.  ``loss_fn``: one loss or a sequence of K, as in ``train_replicas_lockstep``; the
    validation losses of a replica are those of its own loss (its class weights).  A replica that stopped early sits out of the later epochs.  Returns
    ``[(model, train_loss_history, val_loss_history)]``, every model with its best weights loaded.  ``mixed=True``: the
    replicas may differ in architecture, in the training pass and in the validation pass alike.  Training and validation
    loaders may be ``DeviceBatchLoader``s in any mix with ``DataLoader``s, as in the two loops above.  ``mixes``: as in
    ``train_replicas_lockstep``, for the training and the validation loaders alike; the ``state_dict`` of a replica's mix is
    checkpointed and restored together with the model's, so best weights mean the best mix too."""
    models, optimizers, schedulers = list(models), list(optimizers), list(schedulers)
    train_loaders, val_loaders = list(train_loaders), list(val_loaders)
    K = len(models)
    if not (K == len(optimizers) == len(schedulers) == len(train_loaders) == len(val_loaders)):
        raise ValueError(f"{K} models, {len(optimizers)} optimizers, {len(schedulers)} schedulers, {len(train_loaders)} training "
                         f"loaders and {len(val_loaders)} validation loaders")
    check_loader_devices(train_loaders, device, "train_eval_replicas_lockstep (train_loaders)")
    check_loader_devices(val_loaders, device, "train_eval_replicas_lockstep (val_loaders)")
    mixes = _check_mixes(train_loaders, mixes, "train_eval_replicas_lockstep (train_loaders)")
    _check_mixes(val_loaders, mixes, "train_eval_replicas_lockstep (val_loaders)")
    train_hist, val_hist = [[] for _ in models], [[] for _ in models]
    loss_fns = _loss_list(loss_fn, K)
    best_val_loss = [float("inf")] * K
    epochs_no_improve = [0] * K
    best_model_weights = [None] * K
    best_mix_weights = [None] * K
    running = list(range(K))
    for _ in range(epochs):
        if not running:
            break
        hist = train_replicas_lockstep([models[k] for k in running], [optimizers[k] for k in running],
                                       [train_loaders[k] for k in running], [loss_fns[k] for k in running], 1, device, mixed=mixed,
                                       mixes=[mixes[k] for k in running])
        for k, h in zip(running, hist):
            train_hist[k].append(h[0])
        for k in running:
            models[k].eval()
        tags, outs, labs = [], [], []
        fused = _fused_step_applies([optimizers[k] for k in running], [models[k] for k in running], [loss_fns[k] for k in running])
        weights = _class_weights(loss_fns) if fused else None
        with torch.no_grad():
            pairs = _eval_pairs((k, models[k], val_loaders[k], mixes[k]) for k in running)
            for k, out, lab in _grouped_eval_batches(pairs, device, mixed):
                tags.append(k)
                outs.append(out)
                labs.append(lab)
            if not outs:
                losses = []
            elif fused and all(o.shape[0] > 0 for o in outs):           # the losses of the pass in group launches, no gradient
                losses = ce_loss_group(outs, labs, with_grad=False, weights=weights and [weights[k] for k in tags])[0].tolist()
            else:
                losses = torch.stack([loss_fns[k](o, lab) for k, o, lab in zip(tags, outs, labs)]).tolist()
        val_loss, count = {k: 0 for k in running}, {k: 0 for k in running}
        for k, v in zip(tags, losses):
            val_loss[k] += v
            count[k] += 1
        still = []
        for k in running:
            avg_val_loss = val_loss[k] / count[k]
            val_hist[k].append(avg_val_loss)
            if schedulers[k] is not None:
                schedulers[k].step(avg_val_loss)
            if avg_val_loss < best_val_loss[k]:
                best_val_loss[k] = avg_val_loss
                best_model_weights[k] = copy.deepcopy(models[k].state_dict())
                if mixes[k] is not None:
                    best_mix_weights[k] = copy.deepcopy(mixes[k].state_dict())
                epochs_no_improve[k] = 0
            else:
                epochs_no_improve[k] += 1
            if epochs_no_improve[k] < patience:
                still.append(k)
        running = still
    for k in range(K):
        if best_model_weights[k]:
            models[k].load_state_dict(best_model_weights[k])
        if best_mix_weights[k]:
            mixes[k].load_state_dict(best_mix_weights[k])
    return [(models[k], train_hist[k], val_hist[k]) for k in range(K)]
