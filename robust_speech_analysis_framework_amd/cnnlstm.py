"""CNN-LSTM-with-attention classifier on the HIP path (drop-in for ``src/models.py``).

``CNNLSTM`` keeps the reference's constructor signature, attribute tree and ``state_dict`` keys
(``src/models.py:129-159``) so the shipped checkpoints load unchanged and
``model.res_block1.conv1.weight`` style access (``src/dl_cv_strategies.py:336,426``) works.  The
parameters live in ordinary ``torch.nn`` containers; ``forward`` does not call them: in eval mode
it folds BatchNorm into the convolutions, packs everything into one device blob and runs
``rsaf_cnnlstm_forward`` (fp32 MFMA GEMMs + persistent LSTM kernel).

Training: in ``model.train()`` mode ``forward`` runs ``rsaf_cnnlstm_train_forward``
(BatchNorm on batch statistics, dropout masks drawn from torch's device RNG or, with ``model.dropout_stream`` set, from
the counter-based generator of ``rsaf_dropout_masks_group``, running statistics updated as ``nn.BatchNorm1d`` does) inside a ``torch.autograd.Function`` whose backward is ``rsaf_cnnlstm_train_backward``:
``loss.backward()`` fills ``.grad`` of the ordinary parameters, so the reference's loops
(``src/dl_cv_strategies.py:118-125,241-243``) and ``torch.optim.Adam(model.parameters())`` work unchanged.
``forward`` raises for CPU tensors instead of silently using a PyTorch fallback.

This module holds the ``nn.Module`` drop-in, the folded eval-mode blob and the eval-mode forwards (one model, stages,
group).  The training step is ``cnnlstm_train``, the fused step (cross-entropy, Adam, running statistics in HIP) is
``cnnlstm_fused`` and the lockstep loops are ``cnnlstm_loops``; their names are re-exported at the end of this file, which
stays the import path of all of them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .cnnlstm_train import (_ACT_CODE, _SHARED_DIMS, _arch, _check_group, _check_input, _chunks, _dims5, _launch_chunked,
                            _masks_for, _sizes6, _train_step)

BN_EPS = 1e-5


def get_activation_fn(name):
    """Same contract as ``src/models.py:7-25``: 'silu' / 'gelu', else ValueError."""
    table = {"silu": F.silu, "gelu": F.gelu}
    if name not in table:
        raise ValueError(f"Unsupported activation function: {name}")
    return table[name]


def _version_key(module, device):
    """Changes whenever a parameter or buffer of ``module`` is replaced or written in place: the key of the folded caches."""
    return (str(device),) + tuple((p.data_ptr(), p._version) for p in list(module.parameters()) + list(module.buffers()))


class ResidualBlock(nn.Module):
    """Parameter container with the reference's layout (``src/models.py:43-62``)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dropout=0.2, activation_fn="silu"):
        super().__init__()
        self.activation = get_activation_fn(activation_fn)
        self.activation_name = activation_fn
        pad = (kernel_size - 1) // 2
        self.conv1 = nn.Conv1d(in_channels, out_channels, kernel_size, stride, padding=pad)
        self.bn1 = nn.BatchNorm1d(out_channels)
        self.conv2 = nn.Conv1d(out_channels, out_channels, kernel_size, stride, padding=pad)
        self.bn2 = nn.BatchNorm1d(out_channels)
        self.dropout = nn.Dropout(dropout)
        self.shortcut = nn.Sequential()
        if in_channels != out_channels:
            self.shortcut = nn.Sequential(nn.Conv1d(in_channels, out_channels, kernel_size=1, stride=stride),
                                          nn.BatchNorm1d(out_channels))

        self._packed = None
        self._packed_key = None
        self._workspace = None

    def _folded(self, device):
        key = _version_key(self, device)
        if self._packed is None or self._packed_key != key:
            parts = list(_fold_conv_bn(self.conv1, self.bn1))
            parts += list(_fold_conv_bn(self.shortcut[0], self.shortcut[1])) if len(self.shortcut) > 0 else [None, None]
            parts += list(_fold_conv_bn(self.conv2, self.bn2))
            self._packed = [None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
                            for a in parts]
            self._packed_key = key
        return self._packed

    def forward(self, x):
        """Standalone block (``src/models.py:64-76``): x [B, Cin, T] -> [B, Cout, T], eval mode, on the HIP path
        (``rsaf_cnn_resblock_forward``; the kernels are channels-last, so the two permutes are real copies here while
        ``CNNLSTM.forward`` reads its [B, T, D] input in place)."""
        if not x.is_cuda:
            raise _lib.RsafError("ResidualBlock.forward needs a HIP (cuda) tensor: there is no CPU fallback")
        if self.training:
            raise NotImplementedError("a standalone ResidualBlock runs in eval mode on the HIP path; the training step "
                                      "(batch statistics, dropout, backward) runs through CNNLSTM")
        if any(c.stride[0] != 1 or c.kernel_size[0] != k for c, k in ((self.conv1, 3), (self.conv2, 3))):
            raise NotImplementedError("the HIP block implements kernel_size 3 / stride 1 (all the reference uses)")
        cin, cout = self.conv1.in_channels, self.conv1.out_channels
        if x.dim() != 3 or x.shape[1] != cin:
            raise ValueError(f"expected input [B, {cin}, T], got {tuple(x.shape)}")
        lib = _lib.load()
        w1, b1, wsc, bsc, w2, b2 = self._folded(x.device)
        xt = x.to(torch.float32).permute(0, 2, 1).contiguous()
        B, T = xt.shape[0], xt.shape[1]
        need = max(int(lib.rsaf_cnn_resblock_workspace_bytes(B, T, cout)), 16)
        if self._workspace is None or self._workspace.numel() * 4 < need or self._workspace.device != x.device:
            self._workspace = torch.empty(need // 4, dtype=torch.float32, device=x.device)
        y = torch.empty((B, T, cout), dtype=torch.float32, device=x.device)
        with torch.no_grad():
            _lib.check(lib.rsaf_cnn_resblock_forward(
                _lib.ptr(xt), B, T, cin, cout, _ACT_CODE[self.activation_name], _lib.ptr(w1), _lib.ptr(b1), _lib.optr(wsc),
                _lib.optr(bsc), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(self._workspace), self._workspace.numel() * 4,
                _lib.ptr(y), _lib.stream_ptr(None)), "rsaf_cnn_resblock_forward")
        return y.permute(0, 2, 1)


class AttentionPooling(nn.Module):
    """Parameter container (``src/models.py:88-92``)."""

    def __init__(self, input_dim):
        super().__init__()
        self.attention_weights = nn.Linear(input_dim, 1)

    def forward(self, lstm_out):
        """Standalone pooling (``src/models.py:94-107``): [B, T, F] -> [B, F] through ``rsaf_attnpool_forward``."""
        if not lstm_out.is_cuda:
            raise _lib.RsafError("AttentionPooling.forward needs a HIP (cuda) tensor: there is no CPU fallback")
        F_ = self.attention_weights.in_features
        if lstm_out.dim() != 3 or lstm_out.shape[2] != F_:
            raise ValueError(f"expected input [B, T, {F_}], got {tuple(lstm_out.shape)}")
        if F_ not in (128, 256):
            raise NotImplementedError("the HIP pooling kernel covers 2 * lstm_hidden_dim = 128 or 256")
        lib = _lib.load()
        x = lstm_out.detach().to(torch.float32).contiguous()
        w = self.attention_weights.weight.detach().to(torch.float32).reshape(-1).contiguous()
        b = self.attention_weights.bias.detach().to(torch.float32).contiguous()
        out = torch.empty((x.shape[0], F_), dtype=torch.float32, device=x.device)
        _lib.check(lib.rsaf_attnpool_forward(_lib.ptr(x), x.shape[0], x.shape[1], F_, _lib.ptr(w), _lib.ptr(b),
                                             _lib.ptr(out), _lib.stream_ptr(None)), "rsaf_attnpool_forward")
        return out


def _f64(t):
    return t.detach().to("cpu", torch.float64).numpy()


def _fold_conv_bn(conv, bn):
    """BN(conv(x)) in eval mode == conv'(x): returns tap-major [Cout, k*Cin] weights and bias."""
    w, b = _f64(conv.weight), _f64(conv.bias)
    s = _f64(bn.weight) / np.sqrt(_f64(bn.running_var) + bn.eps)
    wf = w * s[:, None, None]
    bf = (b - _f64(bn.running_mean)) * s + _f64(bn.bias)
    return np.ascontiguousarray(wf.transpose(0, 2, 1)).reshape(w.shape[0], -1), bf


def weight_offsets(input_dim, channels, hidden, num_classes, layers):
    lib = _lib.load()
    buf = (C.c_int64 * 32)()
    n = C.c_int(0)
    _lib.check(lib.rsaf_cnnlstm_weight_offsets(input_dim, channels, hidden, num_classes, layers, buf, 32,
                                               C.byref(n)), "rsaf_cnnlstm_weight_offsets")
    total = lib.rsaf_cnnlstm_weight_floats(input_dim, channels, hidden, num_classes, layers)
    return [int(buf[i]) for i in range(n.value)], int(total)


def pack_weights(model: "CNNLSTM") -> np.ndarray:
    """Fold + pack the module's parameters into the blob layout of ``rsaf_cnnlstm_forward``."""
    d = model.dims
    offs, total = weight_offsets(*_dims5(d))
    blob = np.zeros(total, dtype=np.float32)
    it = iter(offs)

    def put(arr):
        o = next(it)
        if o >= 0:
            a = np.asarray(arr, dtype=np.float64).reshape(-1)
            blob[o:o + a.size] = a.astype(np.float32)

    r1, r2 = model.res_block1, model.res_block2
    for part in _fold_conv_bn(r1.conv1, r1.bn1):
        put(part)
    if len(r1.shortcut) > 0:
        for part in _fold_conv_bn(r1.shortcut[0], r1.shortcut[1]):
            put(part)
    else:
        next(it), next(it)
    for conv, bn in ((r1.conv2, r1.bn2), (r2.conv1, r2.bn1), (r2.conv2, r2.bn2)):
        for part in _fold_conv_bn(conv, bn):
            put(part)
    for l in range(d["layers"]):
        g = lambda n: _f64(getattr(model.lstm, n))                                   # noqa: E731
        put(np.concatenate([g(f"weight_ih_l{l}"), g(f"weight_ih_l{l}_reverse")], axis=0))
        put(np.concatenate([g(f"bias_ih_l{l}") + g(f"bias_hh_l{l}"),
                            g(f"bias_ih_l{l}_reverse") + g(f"bias_hh_l{l}_reverse")]))
        put(np.stack([g(f"weight_hh_l{l}"), g(f"weight_hh_l{l}_reverse")]))
    put(_f64(model.attention_pooling.attention_weights.weight))
    put(_f64(model.attention_pooling.attention_weights.bias))
    put(_f64(model.fc.weight))
    put(_f64(model.fc.bias))
    return blob


def _workspace(x, dims, cached=None, empty_ok=True):
    """Workspace of one eval-mode forward of ``x`` [B, T, D]: ``cached`` if it is large enough, else a new tensor."""
    B, T = x.shape[0], x.shape[1]
    need = _lib.load().rsaf_cnnlstm_workspace_bytes(*_sizes6(B, T, dims))
    if need < 0 and (B > 0 or not empty_ok):
        raise ValueError("sequence length must be >= 2")
    if cached is None or cached.numel() * cached.element_size() < need:
        cached = torch.empty(max(int(need), 16) // 4, dtype=torch.float32, device=x.device)
    return cached


def cnnlstm_forward_packed(x, blob, dims, act, workspace=None, stream=None):
    """x float32 [B,T,D] on the device, blob = packed weights on the same device -> logits [B,NC]."""
    lib = _lib.load()
    _check_input(x, dims["input_dim"])
    x = x.contiguous()
    B, T = x.shape[0], x.shape[1]
    workspace = _workspace(x, dims, workspace)
    logits = torch.empty((B, dims["num_classes"]), dtype=torch.float32, device=x.device)
    _lib.check(lib.rsaf_cnnlstm_forward(
        _lib.ptr(x), B, T, *_dims5(dims), _ACT_CODE[act], _lib.ptr(blob), _lib.ptr(workspace), workspace.numel() * 4, _lib.ptr(logits),
        _lib.stream_ptr(stream)), "rsaf_cnnlstm_forward")
    return logits, workspace


class CNNLSTM(nn.Module):
    """Drop-in for ``src/models.py:109-193`` (constructor signature and state_dict keys identical)."""

    def __init__(self, input_dim=768, num_classes=2, cnn_out_channels=128, lstm_hidden_dim=128,
                 lstm_layers=2, dropout_rate=0.5, activation_fn="silu"):
        super().__init__()
        get_activation_fn(activation_fn)                       # ValueError for unknown names
        self.activation_name = activation_fn
        self.res_block1 = ResidualBlock(input_dim, cnn_out_channels, activation_fn=activation_fn)
        self.res_block2 = ResidualBlock(cnn_out_channels, cnn_out_channels, activation_fn=activation_fn)
        self.lstm = nn.LSTM(input_size=cnn_out_channels, hidden_size=lstm_hidden_dim, num_layers=lstm_layers,
                            batch_first=True, bidirectional=True,
                            dropout=dropout_rate if lstm_layers > 1 else 0)
        self.attention_pooling = AttentionPooling(input_dim=lstm_hidden_dim * 2)
        self.dropout = nn.Dropout(dropout_rate)
        self.fc = nn.Linear(lstm_hidden_dim * 2, num_classes)
        self.dims = {"input_dim": input_dim, "channels": cnn_out_channels, "hidden": lstm_hidden_dim,
                     "num_classes": num_classes, "layers": lstm_layers}
        self._packed = None
        self._packed_key = None
        self._workspace = None
        self._train_scratch = None
        self._train_dx_scratch = None       # scratch of the input gradient of the training step (cnnlstm_train._Replica.want_dx)
        self.forced_masks = None            # tests: explicit dropout masks for the next training-mode forward
        self.dropout_stream = None          # a DropoutStream: masks from the counter-based generator instead of torch's RNG

    def packed_weights(self, device):
        """Folded weight blob on ``device`` (rebuilt when any parameter/buffer changed)."""
        key = _version_key(self, device)
        if self._packed is None or self._packed_key != key:
            self._packed = torch.from_numpy(pack_weights(self)).to(device)
            self._packed_key = key
        return self._packed

    def forward(self, x):
        """Training mode: the training step on the autograd graph of the parameters and of ``x`` (``x.grad`` after
        ``loss.backward()`` when ``x`` requires a gradient, so a trainable module in front of the classifier learns).
        Eval mode: the inference forward, under ``no_grad`` and with no graph, for the input as for the parameters."""
        if not x.is_cuda:
            raise _lib.RsafError("CNNLSTM.forward needs a HIP (cuda) tensor: there is no CPU fallback")
        x = x.to(torch.float32)
        if self.training:
            _check_input(x, self.dims["input_dim"])
            if x.shape[0] * (x.shape[1] // 2) <= 1:
                # nn.BatchNorm1d in training mode (res_block2 sees B * (T // 2) values per channel)
                raise ValueError("Expected more than 1 value per channel when training")
            x = x.contiguous()
            return _train_step([self], [x], [_masks_for(self, x)], single=True)[0]
        blob = self.packed_weights(x.device)
        with torch.no_grad():
            logits, self._workspace = cnnlstm_forward_packed(x, blob, self.dims, self.activation_name,
                                                             self._workspace)
        return logits


def cnnlstm_forward_stages(model: "CNNLSTM", x, workspace=None):
    """Eval-mode forward that also returns what the reference's sub-modules return (forward hooks on
    ``res_block1`` / ``res_block2`` / ``lstm`` / ``attention_pooling`` of ``src/models.py``), channels-last:
    dict(res1 [B,T,C], res2 [B,T/2,C], lstm [B,T/2,2H], pooled [B,2H], logits [B,NC]).  ``workspace``: a float32 device
    tensor to work in when it is large enough (``rsaf_cnnlstm_workspace_bytes``), else a new one is taken."""
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.RsafError("cnnlstm_forward_stages needs a HIP (cuda) tensor")
    d = model.dims
    x = x.to(torch.float32).contiguous()
    B, T, _ = x.shape
    blob = model.packed_weights(x.device)
    ws = _workspace(x, d, workspace, empty_ok=False)
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)            # noqa: E731
    out = {"res1": e(B, T, d["channels"]), "res2": e(B, T // 2, d["channels"]), "lstm": e(B, T // 2, 2 * d["hidden"]),
           "pooled": e(B, 2 * d["hidden"]), "logits": e(B, d["num_classes"])}
    _lib.check(lib.rsaf_cnnlstm_forward_stages(
        _lib.ptr(x), B, T, *_dims5(d), _ACT_CODE[model.activation_name],
        _lib.ptr(blob), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(out["logits"]), _lib.ptr(out["res1"]), _lib.ptr(out["res2"]),
        _lib.ptr(out["lstm"]), _lib.ptr(out["pooled"]), _lib.stream_ptr(None)), "rsaf_cnnlstm_forward_stages")
    return out


def collate_zero_pad(seqs, device="cuda"):
    """Batch assembly of the reference harness (``src/dl_cv_strategies.py:81-84``): right zero-padding
    to the batch maximum, float32, no mask."""
    T = max(int(s.shape[0]) for s in seqs)
    out = torch.zeros((len(seqs), T, int(seqs[0].shape[1])), dtype=torch.float32, device=device)
    for i, s in enumerate(seqs):
        out[i, :s.shape[0]] = torch.as_tensor(s, dtype=torch.float32)
    return out


def eval_outputs(logits):
    """``_eval_model`` post-processing (``src/dl_cv_strategies.py:183-194``): P(class 1) and argmax."""
    return torch.softmax(logits, dim=1)[:, 1], torch.argmax(logits, dim=1)


# ---- group eval forward: K independent eval-mode forwards of one architecture in one call --------------------------------
# ``rsaf_cnnlstm_forward_group``: the recurrences of all items in one launch per layer, their heads in one launch, the
# fp16 planes of the weights once per distinct model; everything else per item.  The logits are those of ``model(x)``,
# bit for bit.

_group_workspace = {}               # device -> cached workspace tensor of the group calls (grown on demand)
_WS_ALIGN = 256                     # bytes between the items' slices


def cnnlstm_forward_group(models, xs, mixed=False):
    """Eval-mode forward of the pairs ``(models[i], xs[i])`` (same ``dims`` and activation; ``xs[i]`` of own shape
    [B_i, T_i, D]) under ``no_grad`` -> list of logits tensors, each equal to ``models[i](xs[i])`` bit for bit.  ``models``
    may name the same module several times (the batches of one validation loader): its weights are packed and split
    once.  Lists longer than ``train_group_max()`` are split into chunks of that size.

    ``mixed=True``: the models may differ in ``cnn_out_channels``, ``lstm_hidden_dim`` (64 or 128) and activation; they share
    ``input_dim``, ``num_classes`` and ``lstm_layers``.  The recurrences of all items still run in one launch per layer and
    their heads in one launch (``rsaf_cnnlstm_forward_group_mixed``); the logits are the same bits."""
    models, xs = list(models), list(xs)
    if not models:
        raise ValueError("cnnlstm_forward_group needs at least one (model, input) pair")
    if len(models) != len(xs):
        raise ValueError(f"{len(models)} models but {len(xs)} inputs")
    def check_model(k, m):
        if m.training:
            raise ValueError(f"replica {k} is in training mode: the group forward is the inference forward (model.eval())")

    def check_input(k, x):
        if x.shape[0] > 0 and x.shape[1] < 2:
            raise ValueError(f"replica {k}: sequence length must be >= 2")

    _check_group(models, xs, "cnnlstm_forward_group", check_model, check_input, mixed)
    lib = _lib.load()
    dims, device = models[0].dims, xs[0].device
    with torch.no_grad():
        blobs = {}
        for m in models:
            if id(m) not in blobs:
                blobs[id(m)] = m.packed_weights(device)
        xs = [x.detach().to(torch.float32).contiguous() for x in xs]
        rows = [x.shape[0] for x in xs]
        outs = list(torch.split(torch.empty((sum(rows), dims["num_classes"]), dtype=torch.float32, device=device), rows))
        live = [k for k, B in enumerate(rows) if B > 0]                 # an empty batch is no item: its logits are [0, NC]
        needs = [int(lib.rsaf_cnnlstm_workspace_bytes(*_sizes6(rows[k], xs[k].shape[1], models[k].dims))) for k in live]
        offs, total = [], 0                                             # the items of a call side by side in one workspace
        for _, chunk in _chunks(needs):
            end = 0
            for n in chunk:
                offs.append(end)
                end += (n + _WS_ALIGN - 1) // _WS_ALIGN * _WS_ALIGN
            total = max(total, end)
        ws = _group_workspace.get(str(device))
        if ws is None or ws.numel() * 4 < total:
            ws = _group_workspace[str(device)] = torch.empty(total // 4, dtype=torch.float32, device=device)

        def fill(it, k, j):
            it.x, it.B, it.T, it.weights = xs[k].data_ptr(), rows[k], xs[k].shape[1], blobs[id(models[k])].data_ptr()
            it.workspace, it.workspace_bytes = ws.data_ptr() + offs[j], needs[j]
            it.logits = outs[k].data_ptr()

        if mixed:
            _launch_chunked("rsaf_cnnlstm_forward_group_mixed", _lib.ForwardItem, live, fill, *[dims[f] for f in _SHARED_DIMS],
                            arch=lambda k: _arch(models[k]))
        else:
            _launch_chunked("rsaf_cnnlstm_forward_group", _lib.ForwardItem, live, fill, *_dims5(dims),
                            _ACT_CODE[models[0].activation_name])
    return outs


# ---- the other three modules of the CNN-LSTM path, under this import path ------------------------------------------------
from .cnnlstm_train import (DropoutStream, Segment, _pack_train_blob, _train_segments, _unpack_grads,  # noqa: E402,F401
                            cnnlstm_train_group, draw_masks, draw_masks_group, train_group_max, train_param_offsets)
from .cnnlstm_fused import FusedAdam, _adam_order, ce_loss_group, cnnlstm_train_step_group  # noqa: E402,F401
from .cnnlstm_loops import (CNNLSTMGroup, eval_model_grouped, eval_replicas_lockstep,  # noqa: E402,F401
                            train_eval_replicas_lockstep, train_replicas_lockstep)
from .augment import AugmentStream, Compose, FeatureMask, GaussianNoise, Scale, TimeMask  # noqa: E402,F401
from .device_data import (DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore,  # noqa: E402,F401
                          batch_indices, collate_batches)
from .layer_mix_train import cnnlstm_mix_train_step_group, collate_mix_batches  # noqa: E402,F401
