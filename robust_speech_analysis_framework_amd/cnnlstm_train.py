"""Training step of the CNN-LSTM on the HIP path: blob layout, replica plan, launchers, autograd function, group step.

``model(x)`` in training mode and ``cnnlstm_train_group`` are one ``torch.autograd.Function`` over a list of replicas.
Each replica's step is planned once (``_Replica``: sizes, saved activations, scratch, mask pointers, outputs); the plan
is read by ``_launch_single`` (``rsaf_cnnlstm_train_forward`` / ``_backward``, the one-replica case) and by
``_launch_chunked`` (every ``*_group`` entry of the library, ``train_group_max()`` items per call).

Group training step: K independent replicas of one architecture in one step (``mixed=True``: of any mix of
``cnn_out_channels``, ``lstm_hidden_dim`` and activation, see ``cnnlstm_train_group``).
The reference trains models of identical architecture and hyper-parameters on different data one after another (the
inner folds of an Optuna trial, ``src/dl_cv_strategies.py:224-251``; the folds of ``:399-422``).  One such training
keeps 2 of the chip's 256 CUs busy during its LSTM recurrences, which are most of the step; K of them side by side
put the recurrences of all replicas into one launch per layer and pass (``rsaf_cnnlstm_train_forward_group`` /
``_backward_group``).  Everything else runs per replica, so the results are those of K separate steps, bit for bit.
The eval-mode half of the same loops (the validation pass of every epoch, ``:131-139``; ``_eval_model``, ``:183-194``)
is grouped in ``cnnlstm.cnnlstm_forward_group``: there every batch of every model is an item of its own, since no
weight changes during a pass.

This module imports nothing from ``cnnlstm``; ``cnnlstm`` re-exports its names.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple

import torch

from . import _lib

_ACT_CODE = {"gelu": 1, "silu": 2}


def _dims5(d):
    """The five model dimensions in the order of the C entries."""
    return d["input_dim"], d["channels"], d["hidden"], d["num_classes"], d["layers"]


def _sizes6(B, T, d):
    """(B, T, D, C, H, L): the argument of the workspace / saved / scratch size queries."""
    return B, T, d["input_dim"], d["channels"], d["hidden"], d["layers"]


# ---- launchers and argument checks of the group calls -------------------------------------------------------------------
def train_group_max():
    """Replicas per C call (``rsaf_cnnlstm_train_group_max``); longer lists are split into chunks of this size."""
    return int(_lib.load().rsaf_cnnlstm_train_group_max())


def _chunks(records):
    """``(index of the chunk's first record, chunk)`` over chunks of ``train_group_max()`` records."""
    gmax = train_group_max()
    for c0 in range(0, len(records), gmax):
        yield c0, records[c0:c0 + gmax]


def _launch_chunked(entry, item_type, records, fill, *tail, arch=None):
    """One call of the library's ``entry(items, n, *tail, stream)`` per chunk of ``records``; ``fill(item, record, k)``
    writes the ctypes ``item_type`` of record ``k``, ``k`` counting over all of ``records``.  ``arch(record)`` (the
    ``*_mixed`` entries): the ``(channels, hidden, act code)`` of a record; the call is then ``entry(items, archs, n,
    *tail, stream)``."""
    fn = getattr(_lib.load(), entry)
    for c0, chunk in _chunks(records):
        items = (item_type * len(chunk))()
        for j, (it, r) in enumerate(zip(items, chunk)):
            fill(it, r, c0 + j)
        head = (items,) if arch is None else (items, (_lib.Arch * len(chunk))(*[_lib.Arch(*arch(r)) for r in chunk]))
        _lib.check(fn(*head, len(chunk), *tail, _lib.stream_ptr(None)), entry)


def _arch(model):
    """What may differ between the replicas of a mixed group, as ``rsaf_cnnlstm_arch`` takes it."""
    return model.dims["channels"], model.dims["hidden"], _ACT_CODE[model.activation_name]


_SHARED_DIMS = ("input_dim", "num_classes", "layers")        # what the replicas of a mixed group have in common


def _check_input(x, D, where=""):
    if x.dim() != 3 or x.shape[2] != D:
        raise ValueError(f"{where}expected input [B, T, {D}], got {tuple(x.shape)}")


def _check_group(models, xs, who, check_model, check_input, mixed=False):
    """The checks every group call makes: one architecture (``mixed``: one ``input_dim``, ``num_classes`` and number of
    LSTM layers), inputs [B, T, D], HIP tensors.  ``check_model(k, m)`` and ``check_input(k, x)`` are the caller's own
    checks of a replica, made right after the shared one of that replica."""
    first = models[0]
    for k, m in enumerate(models):
        if mixed:
            for field in _SHARED_DIMS:
                if m.dims[field] != first.dims[field]:
                    raise ValueError(f"replica {k} differs from replica 0 in {field}: {m.dims[field]} against "
                                     f"{first.dims[field]} (a mixed group shares {', '.join(_SHARED_DIMS)})")
        elif m.dims != first.dims or m.activation_name != first.activation_name:
            raise ValueError(f"replica {k} differs from replica 0: dims {m.dims} / activation {m.activation_name!r} against "
                             f"{first.dims} / {first.activation_name!r}")
        check_model(k, m)
    for k, x in enumerate(xs):
        _check_input(x, first.dims["input_dim"], f"replica {k}: ")
        check_input(k, x)
    for k, x in enumerate(xs):
        if not x.is_cuda:
            raise _lib.RsafError(f"{who} needs HIP (cuda) tensors (replica {k}): there is no CPU fallback")


# ---- blob layout ------------------------------------------------------------------------------------------------------------
def train_param_offsets(dims):
    lib = _lib.load()
    buf = (C.c_int64 * 48)()
    n = C.c_int(0)
    a = _dims5(dims)
    _lib.check(lib.rsaf_cnnlstm_train_param_offsets(*a, buf, 48, C.byref(n)), "rsaf_cnnlstm_train_param_offsets")
    return [int(buf[i]) for i in range(n.value)], int(lib.rsaf_cnnlstm_train_param_floats(*a))


class Segment(NamedTuple):
    """One blob segment: ``pack() -> flat tensor``; ``outs``: [(parameter, unpack(grad segment) -> grad of that parameter)]."""
    offset: int
    n: int
    pack: Callable
    outs: list


def _train_segments(model):
    """Blob segments in the order of ``rsaf_cnnlstm_train_param_offsets`` (include/rsaf.h): a list of
    ``(offset, n_floats, pack() -> flat tensor, [(parameter, unpack(grad segment) -> grad of that parameter)])``."""
    d = model.dims
    offs, total = train_param_offsets(d)
    it = iter(offs)
    H, L = d["hidden"], d["layers"]
    segs = []

    def plain(prm):
        segs.append(Segment(next(it), prm.numel(), (lambda q=prm: q.reshape(-1)), [(prm, lambda g, q=prm: g.view(q.shape))]))

    def conv(cv, bn):
        cout, cin, k = cv.weight.shape                          # stored tap-major [Cout][k][Cin]
        segs.append(Segment(next(it), cv.weight.numel(), (lambda w=cv.weight: w.permute(0, 2, 1).reshape(-1)),
                            [(cv.weight, lambda g, a=cout, b=k, c=cin: g.view(a, b, c).permute(0, 2, 1))]))
        for prm in (cv.bias, bn.weight, bn.bias):
            plain(prm)

    r1, r2 = model.res_block1, model.res_block2
    conv(r1.conv1, r1.bn1)
    if len(r1.shortcut) > 0:
        conv(r1.shortcut[0], r1.shortcut[1])
    else:
        for _ in range(4):
            next(it)
    conv(r1.conv2, r1.bn2)
    conv(r2.conv1, r2.bn1)
    conv(r2.conv2, r2.bn2)
    for l in range(L):
        g = lambda n: getattr(model.lstm, n)                                         # noqa: E731
        wf, wr = g(f"weight_ih_l{l}"), g(f"weight_ih_l{l}_reverse")
        segs.append(Segment(next(it), 2 * wf.numel(), (lambda a=wf, b=wr: torch.cat([a, b], 0).reshape(-1)),
                            [(wf, lambda gr: gr.view(8 * H, -1)[:4 * H]), (wr, lambda gr: gr.view(8 * H, -1)[4 * H:])]))
        bs = [g(f"bias_ih_l{l}"), g(f"bias_hh_l{l}"), g(f"bias_ih_l{l}_reverse"), g(f"bias_hh_l{l}_reverse")]
        segs.append(Segment(next(it), 8 * H, (lambda b=bs: torch.cat([b[0] + b[1], b[2] + b[3]])),
                            [(bs[0], lambda gr: gr[:4 * H]), (bs[1], lambda gr: gr[:4 * H]),
                             (bs[2], lambda gr: gr[4 * H:]), (bs[3], lambda gr: gr[4 * H:])]))
        hf, hr = g(f"weight_hh_l{l}"), g(f"weight_hh_l{l}_reverse")
        segs.append(Segment(next(it), 2 * hf.numel(), (lambda a=hf, b=hr: torch.stack([a, b]).reshape(-1)),
                            [(hf, lambda gr: gr.view(2, 4 * H, H)[0]), (hr, lambda gr: gr.view(2, 4 * H, H)[1])]))
    aw = model.attention_pooling.attention_weights
    for prm in (aw.weight, aw.bias, model.fc.weight, model.fc.bias):
        plain(prm)
    return segs, total


def _blob_params(segs):
    """The parameters in blob order."""
    return [p for s in segs for p, _ in s.outs]


def _pack_train_blob(model, device, segments=None):
    """The module's parameters in the blob layout of ``rsaf_cnnlstm_train_param_offsets``: (segments, blob).
    ``segments``: what ``_train_segments(model)`` returned, where the caller has it already."""
    segs, total = segments if segments is not None else _train_segments(model)
    blob = torch.zeros(total, dtype=torch.float32, device=device)
    with torch.no_grad():
        for s in segs:
            blob[s.offset:s.offset + s.n] = s.pack()
    return segs, blob


def _unpack_grads(segs, params, grads):
    by_param = {id(prm): (off, n, unpack) for off, n, _, outs in segs for prm, unpack in outs}
    out, taken = [], set()
    for prm in params:
        off, n, unpack = by_param[id(prm)]
        g = unpack(grads[off:off + n]).reshape(prm.shape).contiguous()
        # b_ih and b_hh of a direction receive the same run of the blob; each gets memory of its own, since whatever edits
        # `.grad` in place (clip_grad_norm_ multiplies it) would otherwise reach the shared floats once per parameter
        if g.data_ptr() in taken:
            g = g.clone()
        taken.add(g.data_ptr())
        out.append(g)
    return out


# ---- dropout masks and running statistics ---------------------------------------------------------------------------------
def draw_masks(model, B, T, device):
    """Dropout keep masks of one training step (float32 0 or 1/(1-p); None where p == 0), from torch's device RNG."""
    d = model.dims
    Tp = T // 2

    def mk(shape, p):
        if p <= 0.0:
            return None
        if p >= 1.0:
            return torch.zeros(shape, dtype=torch.float32, device=device)
        return (torch.rand(shape, device=device) >= p).to(torch.float32) / (1.0 - p)

    p_l = float(model.lstm.dropout)
    return {"res_block1": mk((B, T, d["channels"]), float(model.res_block1.dropout.p)),
            "res_block2": mk((B, Tp, d["channels"]), float(model.res_block2.dropout.p)),
            "lstm": [mk((B, Tp, 2 * d["hidden"]), p_l) for _ in range(d["layers"] - 1)],
            "fc": mk((B, 2 * d["hidden"]), float(model.dropout.p))}


class DropoutStream:
    """Where a model's dropout masks come from when they are not torch's: ``seed`` (0 <= seed < 2**64) names the stream,
    ``step`` counts the training steps that consulted it.  Every mask element is a pure function of (seed, step, mask
    slot, element index) (``rsaf_dropout_masks_group``, include/rsaf.h), so the masks of a training do not depend on what
    else draws random numbers, on how replicas are grouped or on their order, and ``state_dict()`` is all a checkpoint
    needs to continue them.  Host state only: it is no module buffer, and ``model.state_dict()`` keeps the reference's keys.
    Set it as ``model.dropout_stream``; one stream belongs to one model."""

    def __init__(self, seed, step=0):
        self.load_state_dict({"seed": seed, "step": step})

    def state_dict(self):
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state):
        seed, step = int(state["seed"]), int(state["step"])
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"DropoutStream: seed must be in [0, 2**64), got {seed}")
        if not 0 <= step < 2 ** 64:
            raise ValueError(f"DropoutStream: step must be in [0, 2**64), got {step}")
        self.seed, self.step = seed, step

    def __repr__(self):
        return f"DropoutStream(seed={self.seed}, step={self.step})"


def _mask_slots(model, B, T):
    """``(slot, shape, p)`` of the up to six masks of a step with input [B, T, D], slots as ``rsaf_dropout_masks_group``
    numbers them: 0 res_block1, 1 res_block2, 2 fc, 3 + l the LSTM inter-layer mask l."""
    d = model.dims
    Tp, p_l = T // 2, float(model.lstm.dropout)
    return [(0, (B, T, d["channels"]), float(model.res_block1.dropout.p)),
            (1, (B, Tp, d["channels"]), float(model.res_block2.dropout.p)),
            (2, (B, 2 * d["hidden"]), float(model.dropout.p))] + \
           [(3 + l, (B, Tp, 2 * d["hidden"]), p_l) for l in range(d["layers"] - 1)]


def draw_masks_group(models, shapes, streams, device):
    """Dropout keep masks of one training step of K replicas, ``shapes[k] = (B_k, T_k)``, from ``streams[k]`` (a
    ``DropoutStream`` each, no stream twice): a list of mask dicts in the format of ``draw_masks`` (None where p == 0).
    All masks of up to ``train_group_max()`` replicas are views of one allocation (each starting at a multiple of 4
    floats) and are written by one launch of ``rsaf_dropout_masks_group``.  The ``step`` of every stream that had a mask
    to draw is used once and then incremented."""
    models, shapes, streams = list(models), list(shapes), list(streams)
    if not (len(models) == len(shapes) == len(streams)):
        raise ValueError(f"{len(models)} models, {len(shapes)} shapes and {len(streams)} streams")
    if torch.device(device).type != "cuda":
        raise _lib.RsafError("draw_masks_group needs a HIP (cuda) device: there is no CPU fallback")
    seen = {}
    for k, st in enumerate(streams):
        if not isinstance(st, DropoutStream):
            raise ValueError(f"replica {k}: expected a DropoutStream, got {type(st).__name__}")
        if id(st) in seen:
            raise ValueError(f"replicas {seen[id(st)]} and {k} share one DropoutStream")
        seen[id(st)] = k
    records = []                                    # per replica: its stream and the (slot, shape, p) of the masks to draw
    for model, (B, T), st in zip(models, shapes, streams):
        records.append((st, [(slot, shape, p) for slot, shape, p in _mask_slots(model, int(B), int(T)) if p > 0.0]))
    out = []
    for _, chunk in _chunks(records):
        total, placed = 0, []
        for st, slots in chunk:
            row = []
            for slot, shape, p in slots:
                n = 1
                for v in shape:
                    n *= v
                row.append((slot, shape, p, total, n))
                total += (n + 3) // 4 * 4
            placed.append((st, row))
        buf = torch.empty(total, dtype=torch.float32, device=device)
        base = buf.data_ptr()

        def fill(it, rec, _k):
            st, row = rec
            it.seed, it.step = st.seed, st.step
            for slot, _, p, off, n in row:
                it.mask[slot], it.n[slot], it.p[slot] = base + 4 * off, n, p

        if total:                                   # a chunk of replicas without dropout has nothing to launch
            _launch_chunked("rsaf_dropout_masks_group", _lib.DropoutItem, placed, fill)
        for st, row in placed:
            views = {slot: buf[off:off + n].view(shape) for slot, shape, _, off, n in row}
            out.append(views)
            if row:
                st.step += 1
    res = []
    for model, views in zip(models, out):
        res.append({"res_block1": views.get(0), "res_block2": views.get(1), "fc": views.get(2),
                    "lstm": [views.get(3 + l) for l in range(model.dims["layers"] - 1)]})
    return res


def _masks_for(model, x):
    """Masks of a single-model training forward: ``forced_masks``, else the model's ``dropout_stream``, else torch's RNG."""
    if model.forced_masks is not None:
        return model.forced_masks
    if model.dropout_stream is not None:
        return draw_masks_group([model], [(x.shape[0], x.shape[1])], [model.dropout_stream], x.device)[0]
    return draw_masks(model, x.shape[0], x.shape[1], x.device)


def _tracked_bn(model, B, T):
    """``(index, layer, rows it normalised over)`` of the BatchNorm layers that keep running statistics, out of the
    five of a step with input [B, T, D] (index 1, the shortcut's, exists only where the shortcut is a convolution)."""
    r1, r2 = model.res_block1, model.res_block2
    bns = (r1.bn1, r1.shortcut[1] if len(r1.shortcut) > 0 else None, r1.bn2, r2.bn1, r2.bn2)
    for i, (bn, n) in enumerate(zip(bns, (B * T, B * T, B * T, B * (T // 2), B * (T // 2)))):
        if bn is not None and bn.track_running_stats and bn.running_mean is not None:
            yield i, bn, n


def _unbias(n):
    return n / (n - 1.0) if n > 1 else 1.0


def _update_running_stats(model, stats, B, T):
    """Running statistics, as nn.BatchNorm1d in training mode (momentum, unbiased variance); stats [5][3][C] of the step."""
    with torch.no_grad():
        for i, bn, n in _tracked_bn(model, B, T):
            bn.num_batches_tracked += 1
            m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            bn.running_mean.mul_(1 - m).add_(stats[i, 0], alpha=m)
            bn.running_var.mul_(1 - m).add_(stats[i, 1], alpha=m * _unbias(n))


# ---- replica plan -------------------------------------------------------------------------------------------------------------
class _Replica:
    """Record of one replica's training step: what the forward and backward entries read and write.  ``blob``: the
    packed parameters; ``logits`` / ``stats``: views to write into, allocated here when not given.  ``segs`` / ``params``
    (autograd path) and ``dlogits`` / ``grads`` (backward) are filled in by whoever needs them."""

    def __init__(self, model, x, masks, blob, logits=None, stats=None):
        lib = _lib.load()
        d = model.dims
        B, T = x.shape[0], x.shape[1]
        sizes = _sizes6(B, T, d)
        n_saved, n_scr = int(lib.rsaf_cnnlstm_train_saved_floats(*sizes)), int(lib.rsaf_cnnlstm_train_scratch_floats(*sizes))
        if n_saved < 0 or n_scr < 0:
            raise ValueError("sequence length must be >= 2")
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)                   # noqa: E731
        if model._train_scratch is None or model._train_scratch.numel() < n_scr or model._train_scratch.device != x.device:
            model._train_scratch = new(n_scr)
        self.model, self.x, self.B, self.T, self.masks, self.blob = model, x, B, T, masks, blob
        lm = masks["lstm"]
        self.lstm_ptrs = (C.c_void_p * len(lm))(*[_lib.optr(m) for m in lm]) if lm else None
        self.saved, self.scratch = new(n_saved), model._train_scratch
        self.logits = logits if logits is not None else new(B, d["num_classes"])
        self.stats = stats if stats is not None else new(5, 3, d["channels"])
        self.segs = self.params = self.dlogits = self.grads = None
        self.dx = self.dx_scratch = None                  # backward: the gradient of ``x`` and its scratch, where one is wanted

    def backward_scratch(self):
        """The scratch is the model's cached buffer, shared with its later forwards.  Once the model has replaced it (a
        later forward needed a larger one, or one on another device), the backward takes a buffer of its own."""
        if self.scratch is not self.model._train_scratch:
            self.scratch = torch.empty_like(self.scratch)

    def want_dx(self):
        """The backward is to return the gradient of ``x`` as well: takes ``dx`` and the model's cached ``dx_scratch``
        (``rsaf_cnnlstm_train_dx_scratch_floats``; kept while it is large enough, like the training scratch)."""
        m, d = self.model, self.model.dims
        n = int(_lib.load().rsaf_cnnlstm_train_dx_scratch_floats(d["input_dim"], d["channels"]))
        if m._train_dx_scratch is None or m._train_dx_scratch.numel() < n or m._train_dx_scratch.device != self.x.device:
            m._train_dx_scratch = torch.empty(n, dtype=torch.float32, device=self.x.device)
        self.dx, self.dx_scratch = _new_dx(self.x), m._train_dx_scratch


def _new_dx(x):
    """Where the gradient of ``x`` [B, T, D] is written (every row; the kernels do not accumulate)."""
    return torch.empty_like(x)


def _fill_train_item(backward):
    def fill(it, r, _k):
        mk = r.masks
        it.x, it.B, it.T, it.params = r.x.data_ptr(), r.B, r.T, r.blob.data_ptr()
        it.mask_block1, it.mask_block2, it.mask_fc = _lib.optr(mk["res_block1"]), _lib.optr(mk["res_block2"]), _lib.optr(mk["fc"])
        it.mask_lstm_host = C.cast(r.lstm_ptrs, C.c_void_p) if r.lstm_ptrs is not None else None
        it.saved, it.saved_floats = r.saved.data_ptr(), r.saved.numel()
        it.scratch, it.scratch_floats = r.scratch.data_ptr(), r.scratch.numel()
        if backward:
            it.dlogits, it.grads = r.dlogits.data_ptr(), r.grads.data_ptr()
            if r.dx is not None:                       # only an ``rsaf_cnnlstm_train_dx_item`` has these (``_launch_group``)
                it.dx, it.dx_scratch, it.dx_scratch_floats = r.dx.data_ptr(), r.dx_scratch.data_ptr(), r.dx_scratch.numel()
        else:
            it.logits, it.bn_stats_out = r.logits.data_ptr(), r.stats.data_ptr()
    return fill


def _launch_group(reps, backward, mixed=False):
    """``rsaf_cnnlstm_train_{forward,backward}_group`` over the replicas ``reps`` of one architecture; ``mixed``: the
    ``_group_mixed`` entries over replicas of any mix of architectures.  A backward in which a replica wants the gradient of
    its input goes through the ``_dx`` entries (the others of the group leave ``dx`` NULL); one in which none does is the
    call it has always been."""
    if not reps:
        return
    d = reps[0].model.dims
    entry = f"rsaf_cnnlstm_train_{'backward' if backward else 'forward'}_group"
    dx = backward and any(r.dx is not None for r in reps)
    item_type, suffix = (_lib.TrainDxItem, "_dx") if dx else (_lib.TrainItem, "")
    if mixed:
        _launch_chunked(entry + "_mixed" + suffix, item_type, reps, _fill_train_item(backward),
                        *[d[f] for f in _SHARED_DIMS], arch=lambda r: _arch(r.model))
    else:
        _launch_chunked(entry + suffix, item_type, reps, _fill_train_item(backward), *_dims5(d),
                        _ACT_CODE[reps[0].model.activation_name])


def _launch_single(r, backward):
    """``rsaf_cnnlstm_train_{forward,backward}`` of one replica: the path of ``model(x)``.  It runs ``lstm_rec4_kernel`` /
    ``lstm_bwd4_kernel`` where the group entries run their ``_group`` twins, and it is what the group paths are
    compared with bit for bit, so a group of one does not replace it."""
    dx = backward and r.dx is not None
    entry = f"rsaf_cnnlstm_train_{'backward' if backward else 'forward'}{'_dx' if dx else ''}"
    mk, m = r.masks, r.model
    out = (r.dlogits, r.grads) if backward else (r.logits, r.stats)
    tail = (_lib.ptr(r.dx), _lib.ptr(r.dx_scratch), r.dx_scratch.numel()) if dx else ()
    _lib.check(getattr(_lib.load(), entry)(
        _lib.ptr(r.x), r.B, r.T, *_dims5(m.dims), _ACT_CODE[m.activation_name], _lib.ptr(r.blob), _lib.optr(mk["res_block1"]),
        _lib.optr(mk["res_block2"]), r.lstm_ptrs, _lib.optr(mk["fc"]), _lib.ptr(r.saved), r.saved.numel(), _lib.ptr(r.scratch),
        r.scratch.numel(), _lib.ptr(out[0]), _lib.ptr(out[1]), *tail, _lib.stream_ptr(None)), entry)


def _launch(reps, backward, path):
    """``path``: "single" (the one replica of ``model(x)``), "group" or "mixed"."""
    if path == "single":
        for r in reps:
            _launch_single(r, backward)
    else:
        _launch_group(reps, backward, mixed=path == "mixed")


# ---- autograd function ------------------------------------------------------------------------------------------------------
class _TrainStep(torch.autograd.Function):
    """(logits_0, ..., logits_K-1) of K replicas in training mode; backward fills the parameter gradients of every
    replica whose output received a gradient, and returns the gradient of every input that requires one (float32
    [B, T, D], zero-padded frames included: nothing is masked).  A backward in which no input requires a gradient runs
    the launches it ran before inputs could.  ``tensors``: the K inputs (float32, contiguous), then the parameters.
    Double backward is not supported.  ``path``: "single" is the one replica of ``model(x)``, which goes through the single
    entries; "group" / "mixed" as ``_launch`` takes it."""

    @staticmethod
    def forward(ctx, models, masks, segments, path, K, *tensors):
        ctx.set_materialize_grads(False)          # an output outside the loss arrives as None, not as zeros
        xs = tensors[:K]
        reps = []
        for model, x, mk, sg in zip(models, xs, masks, segments):
            r = _Replica(model, x, mk, _pack_train_blob(model, x.device, sg)[1])
            r.segs, r.params = sg[0], _blob_params(sg[0])        # ``params``, replica by replica: the order of the gradients
            reps.append(r)
        ctx.reps, ctx.path = reps, path
        _launch(reps, False, path)
        for r in reps:
            _update_running_stats(r.model, r.stats, r.B, r.T)
        return tuple(r.logits for r in reps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *dlogits):
        if ctx.reps is None:
            raise RuntimeError(f"CNNLSTM {'' if ctx.path == 'single' else 'group '}training step: backward can run once per forward "
                               "(the saved activations are consumed)")
        live = []
        for k, (r, dl) in enumerate(zip(ctx.reps, dlogits)):
            if dl is None:
                continue
            r.backward_scratch()
            r.dlogits = dl.to(torch.float32).contiguous()
            r.grads = torch.zeros_like(r.blob)
            if ctx.needs_input_grad[5 + k]:
                r.want_dx()
            live.append(r)
        _launch(live, True, ctx.path)
        out = []
        for r, dl in zip(ctx.reps, dlogits):
            out += [None] * len(r.params) if dl is None else _unpack_grads(r.segs, r.params, r.grads)
        dxs = [r.dx for r in ctx.reps]            # None: no gradient asked for, or the output stayed out of the loss
        ctx.reps = None
        return (None, None, None, None, None, *dxs, *out)


def _train_step(models, xs, masks, single=False, mixed=False):
    """Training-mode forward of checked replicas -> tuple of logits on the autograd graph of their parameters and of the
    inputs ``xs`` (float32, contiguous) that require a gradient."""
    segments = [_train_segments(m) for m in models]
    path = "single" if single else "mixed" if mixed else "group"
    return _TrainStep.apply(models, masks, segments, path, len(xs), *xs, *[p for sg in segments for p in _blob_params(sg[0])])


# ---- group step ---------------------------------------------------------------------------------------------------------------
def _check_train_group(models, xs, masks, who, mixed=False, graph=True):
    """Argument checks of a group training step; returns (models, float32 contiguous inputs, one mask set per replica:
    ``masks[k]``, else the model's ``forced_masks``, else from its ``dropout_stream`` (the replicas that come this far in
    one launch), else drawn from torch's device RNG, replica by replica).
    ``graph``: the inputs stay on their autograd graph; ``graph=False`` (the fused step, which builds none) refuses an input
    that requires a gradient instead of dropping it."""
    models, xs = list(models), list(xs)
    if not models:
        raise ValueError(f"{who} needs at least one replica")
    if len(models) != len(xs):
        raise ValueError(f"{len(models)} models but {len(xs)} inputs")
    if masks is not None and len(masks) != len(models):
        raise ValueError(f"{len(models)} models but {len(masks)} mask sets")
    seen_modules, seen_params = {}, {}

    def check_model(k, m):
        if not m.training:
            raise ValueError(f"replica {k} is in eval mode: the group step is the training step (model.train())")
        if id(m) in seen_modules:
            raise ValueError(f"replicas {seen_modules[id(m)]} and {k} are the same module")
        seen_modules[id(m)] = k
        for name, prm in m.named_parameters():
            if id(prm) in seen_params:
                raise ValueError(f"replicas {seen_params[id(prm)]} and {k} share the parameter {name}")
        for prm in m.parameters():
            seen_params[id(prm)] = k

    def check_input(k, x):
        if x.shape[0] * (x.shape[1] // 2) <= 1:
            raise ValueError(f"replica {k}: Expected more than 1 value per channel when training")

    _check_group(models, xs, who, check_model, check_input, mixed)
    if not graph:
        for k, x in enumerate(xs):
            if x.requires_grad:
                raise ValueError(f"replica {k}: the input requires a gradient, and {who} builds no autograd graph: "
                                 "use cnnlstm_train_group, whose backward returns it")
    xs = [(x if graph else x.detach()).to(torch.float32).contiguous() for x in xs]
    mks, streamed = [], []
    for k, (m, x) in enumerate(zip(models, xs)):
        mk = masks[k] if masks is not None else None
        if mk is None and m.forced_masks is None and m.dropout_stream is not None:
            streamed.append(k)                     # drawn below, all such replicas in one launch
        mks.append(mk if mk is not None else m.forced_masks if m.forced_masks is not None
                   else None if m.dropout_stream is not None else draw_masks(m, x.shape[0], x.shape[1], x.device))
    if streamed:
        drawn = draw_masks_group([models[k] for k in streamed], [(xs[k].shape[0], xs[k].shape[1]) for k in streamed],
                                 [models[k].dropout_stream for k in streamed], xs[0].device)
        for k, mk in zip(streamed, drawn):
            mks[k] = mk
    return models, xs, mks


def cnnlstm_train_group(models, xs, masks=None, mixed=False):
    """One training-mode forward of K independent ``CNNLSTM`` replicas (same ``dims`` and activation; own weights, own
    batch ``xs[k]`` of own shape [B_k, T_k, D]) -> list of K logits tensors.  Sum the K losses and call ``backward()``
    once: the replicas share nothing, so each model's ``.grad`` is the gradient of its own loss, and an output that
    stays out of the loss leaves its model without gradients.  Logits, gradients and BatchNorm buffers are those of K
    separate ``model(x)`` steps, bit for bit; the LSTM recurrences of all replicas run in one launch per layer and pass.
    An input that requires a gradient receives it (``xs[k].grad`` after ``backward()``, as from ``model(x)``); a group may
    mix such inputs with inputs that do not.

    ``masks[k]``: dropout keep masks in the format of ``draw_masks``; ``None`` (for the list or an entry) uses the
    model's ``forced_masks`` if set, else its ``dropout_stream`` if set (``draw_masks_group``: the masks of all such
    replicas in one launch, each a function of its stream's seed and step alone), and draws them from torch's device RNG
    otherwise, replica by replica.  A stream advances by one per step that consulted it.

    ``mixed=True``: the replicas may differ in ``cnn_out_channels``, ``lstm_hidden_dim`` (64 or 128) and activation (the
    trials of a hyper-parameter search side by side); they share ``input_dim``, ``num_classes`` and ``lstm_layers``.  One
    launch per layer and pass still carries the recurrences of all replicas (``rsaf_cnnlstm_train_forward_group_mixed``
    / ``_backward_group_mixed``), and the results are still those of K separate steps, bit for bit."""
    return list(_train_step(*_check_train_group(models, xs, masks, "cnnlstm_train_group", mixed), mixed=mixed))
