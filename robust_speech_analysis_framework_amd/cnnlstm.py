"""CNN-LSTM-with-attention classifier on the HIP path (drop-in for ``src/models.py``).

``CNNLSTM`` keeps the reference's constructor signature, attribute tree and ``state_dict`` keys
(``src/models.py:129-159``) so the shipped checkpoints load unchanged and
``model.res_block1.conv1.weight`` style access (``src/dl_cv_strategies.py:336,426``) works.  The
parameters live in ordinary ``torch.nn`` containers; ``forward`` does not call them: in eval mode
it folds BatchNorm into the convolutions, packs everything into one device blob and runs
``rsaf_cnnlstm_forward`` (fp32 MFMA GEMMs + persistent LSTM kernel).

Training: in ``model.train()`` mode ``forward`` runs ``rsaf_cnnlstm_train_forward``
(BatchNorm on batch statistics, dropout masks drawn from torch's device RNG, running statistics updated as
``nn.BatchNorm1d`` does) inside a ``torch.autograd.Function`` whose backward is ``rsaf_cnnlstm_train_backward``:
``loss.backward()`` fills ``.grad`` of the ordinary parameters, so the reference's loops
(``src/dl_cv_strategies.py:118-125,241-243``) and ``torch.optim.Adam(model.parameters())`` work unchanged.
``forward`` raises for CPU tensors instead of silently using a PyTorch fallback.
"""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

_ACT_CODE = {"gelu": 1, "silu": 2}
BN_EPS = 1e-5


def get_activation_fn(name):
    """Same contract as ``src/models.py:7-25``: 'silu' / 'gelu', else ValueError."""
    table = {"silu": F.silu, "gelu": F.gelu}
    if name not in table:
        raise ValueError(f"Unsupported activation function: {name}")
    return table[name]


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
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))
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
        optr = lambda t: _lib.ptr(t) if t is not None else None                      # noqa: E731
        with torch.no_grad():
            _lib.check(lib.rsaf_cnn_resblock_forward(
                _lib.ptr(xt), B, T, cin, cout, _ACT_CODE[self.activation_name], _lib.ptr(w1), _lib.ptr(b1), optr(wsc),
                optr(bsc), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(self._workspace), self._workspace.numel() * 4,
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
    offs, total = weight_offsets(d["input_dim"], d["channels"], d["hidden"], d["num_classes"], d["layers"])
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


def cnnlstm_forward_packed(x, blob, dims, act, workspace=None, stream=None):
    """x float32 [B,T,D] on the device, blob = packed weights on the same device -> logits [B,NC]."""
    lib = _lib.load()
    if x.dim() != 3 or x.shape[2] != dims["input_dim"]:
        raise ValueError(f"expected input [B, T, {dims['input_dim']}], got {tuple(x.shape)}")
    x = x.contiguous()
    B, T, D = x.shape
    need = lib.rsaf_cnnlstm_workspace_bytes(B, T, D, dims["channels"], dims["hidden"], dims["layers"])
    if B > 0 and need < 0:
        raise ValueError("sequence length must be >= 2")
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(int(need), 16) // 4, dtype=torch.float32, device=x.device)
    logits = torch.empty((B, dims["num_classes"]), dtype=torch.float32, device=x.device)
    _lib.check(lib.rsaf_cnnlstm_forward(
        _lib.ptr(x), B, T, D, dims["channels"], dims["hidden"], dims["num_classes"], dims["layers"],
        _ACT_CODE[act], _lib.ptr(blob), _lib.ptr(workspace), workspace.numel() * 4, _lib.ptr(logits),
        _lib.stream_ptr(stream)), "rsaf_cnnlstm_forward")
    return logits, workspace


def train_param_offsets(dims):
    lib = _lib.load()
    buf = (C.c_int64 * 48)()
    n = C.c_int(0)
    a = (dims["input_dim"], dims["channels"], dims["hidden"], dims["num_classes"], dims["layers"])
    _lib.check(lib.rsaf_cnnlstm_train_param_offsets(*a, buf, 48, C.byref(n)), "rsaf_cnnlstm_train_param_offsets")
    return [int(buf[i]) for i in range(n.value)], int(lib.rsaf_cnnlstm_train_param_floats(*a))


def _train_segments(model):
    """Blob segments in the order of ``rsaf_cnnlstm_train_param_offsets`` (include/rsaf.h): a list of
    ``(offset, n_floats, pack() -> flat tensor, [(parameter, unpack(grad segment) -> grad of that parameter)])``."""
    d = model.dims
    offs, total = train_param_offsets(d)
    it = iter(offs)
    H, L = d["hidden"], d["layers"]
    segs = []

    def plain(prm):
        segs.append((next(it), prm.numel(), (lambda q=prm: q.reshape(-1)), [(prm, lambda g, q=prm: g.view(q.shape))]))

    def conv(cv, bn):
        cout, cin, k = cv.weight.shape                          # stored tap-major [Cout][k][Cin]
        segs.append((next(it), cv.weight.numel(), (lambda w=cv.weight: w.permute(0, 2, 1).reshape(-1)),
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
        segs.append((next(it), 2 * wf.numel(), (lambda a=wf, b=wr: torch.cat([a, b], 0).reshape(-1)),
                     [(wf, lambda gr: gr.view(8 * H, -1)[:4 * H]), (wr, lambda gr: gr.view(8 * H, -1)[4 * H:])]))
        bs = [g(f"bias_ih_l{l}"), g(f"bias_hh_l{l}"), g(f"bias_ih_l{l}_reverse"), g(f"bias_hh_l{l}_reverse")]
        segs.append((next(it), 8 * H, (lambda b=bs: torch.cat([b[0] + b[1], b[2] + b[3]])),
                     [(bs[0], lambda gr: gr[:4 * H]), (bs[1], lambda gr: gr[:4 * H]),
                      (bs[2], lambda gr: gr[4 * H:]), (bs[3], lambda gr: gr[4 * H:])]))
        hf, hr = g(f"weight_hh_l{l}"), g(f"weight_hh_l{l}_reverse")
        segs.append((next(it), 2 * hf.numel(), (lambda a=hf, b=hr: torch.stack([a, b]).reshape(-1)),
                     [(hf, lambda gr: gr.view(2, 4 * H, H)[0]), (hr, lambda gr: gr.view(2, 4 * H, H)[1])]))
    aw = model.attention_pooling.attention_weights
    for prm in (aw.weight, aw.bias, model.fc.weight, model.fc.bias):
        plain(prm)
    return segs, total


def _bn_modules(model):
    r1, r2 = model.res_block1, model.res_block2
    return [r1.bn1, r1.shortcut[1] if len(r1.shortcut) > 0 else None, r1.bn2, r2.bn1, r2.bn2]


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


def _pack_train_blob(model, device):
    """The module's parameters in the blob layout of ``rsaf_cnnlstm_train_param_offsets``: (segments, blob)."""
    segs, total = _train_segments(model)
    blob = torch.zeros(total, dtype=torch.float32, device=device)
    with torch.no_grad():
        for off, n, pack, _ in segs:
            blob[off:off + n] = pack()
    return segs, blob


def _update_running_stats(model, stats, B, T):
    """Running statistics, as nn.BatchNorm1d in training mode (momentum, unbiased variance); stats [5][3][C] of the step."""
    with torch.no_grad():
        for i, (bn, n) in enumerate(zip(_bn_modules(model), (B * T, B * T, B * T, B * (T // 2), B * (T // 2)))):
            if bn is None or not bn.track_running_stats or bn.running_mean is None:
                continue
            bn.num_batches_tracked += 1
            m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            bn.running_mean.mul_(1 - m).add_(stats[i, 0], alpha=m)
            bn.running_var.mul_(1 - m).add_(stats[i, 1], alpha=m * (n / (n - 1.0) if n > 1 else 1.0))


def _unpack_grads(segs, params, grads):
    by_param = {id(prm): (off, n, unpack) for off, n, _, outs in segs for prm, unpack in outs}
    out = []
    for prm in params:
        off, n, unpack = by_param[id(prm)]
        out.append(unpack(grads[off:off + n]).reshape(prm.shape).contiguous())
    return out


def _lstm_mask_ptrs(masks):
    lm = masks["lstm"]
    return (C.c_void_p * max(len(lm), 1))(*[(_lib.ptr(m) if m is not None else None) for m in lm]) if lm else None


class _TrainStep(torch.autograd.Function):
    """logits = CNNLSTM(x) in training mode; backward fills the parameter gradients (none for x)."""

    @staticmethod
    def forward(ctx, x, model, masks, *params):
        lib = _lib.load()
        d = model.dims
        B, T, D = x.shape
        segs, blob = _pack_train_blob(model, x.device)
        a = (B, T, D, d["channels"], d["hidden"], d["layers"])
        n_saved, n_scr = int(lib.rsaf_cnnlstm_train_saved_floats(*a)), int(lib.rsaf_cnnlstm_train_scratch_floats(*a))
        if n_saved < 0 or n_scr < 0:
            raise ValueError("sequence length must be >= 2")
        saved = torch.empty(n_saved, dtype=torch.float32, device=x.device)
        if model._train_scratch is None or model._train_scratch.numel() < n_scr or model._train_scratch.device != x.device:
            model._train_scratch = torch.empty(n_scr, dtype=torch.float32, device=x.device)
        scratch = model._train_scratch
        logits = torch.empty((B, d["num_classes"]), dtype=torch.float32, device=x.device)
        stats = torch.empty((5, 3, d["channels"]), dtype=torch.float32, device=x.device)
        lstm_ptrs = _lstm_mask_ptrs(masks)
        ctx.call = (x, B, T, D, d["channels"], d["hidden"], d["num_classes"], d["layers"], _ACT_CODE[model.activation_name])
        ctx.bufs = (blob, masks, lstm_ptrs, saved, scratch)
        ctx.segs = segs
        ctx.params = params
        ctx.model = model
        optr = lambda t: _lib.ptr(t) if t is not None else None                      # noqa: E731
        _lib.check(lib.rsaf_cnnlstm_train_forward(
            _lib.ptr(x), *ctx.call[1:], _lib.ptr(blob), optr(masks["res_block1"]), optr(masks["res_block2"]), lstm_ptrs,
            optr(masks["fc"]), _lib.ptr(saved), n_saved, _lib.ptr(scratch), scratch.numel(), _lib.ptr(logits),
            _lib.ptr(stats), _lib.stream_ptr(None)), "rsaf_cnnlstm_train_forward")
        _update_running_stats(model, stats, B, T)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        lib = _lib.load()
        if ctx.bufs is None:
            raise RuntimeError("CNNLSTM training step: backward can run once per forward (the saved activations are consumed)")
        blob, masks, lstm_ptrs, saved, scratch = ctx.bufs
        x = ctx.call[0]
        if scratch is not ctx.model._train_scratch:
            scratch = torch.empty_like(scratch)
        grads = torch.zeros_like(blob)
        dl = dlogits.to(torch.float32).contiguous()
        optr = lambda t: _lib.ptr(t) if t is not None else None                      # noqa: E731
        _lib.check(lib.rsaf_cnnlstm_train_backward(
            _lib.ptr(x), *ctx.call[1:], _lib.ptr(blob), optr(masks["res_block1"]), optr(masks["res_block2"]), lstm_ptrs,
            optr(masks["fc"]), _lib.ptr(saved), saved.numel(), _lib.ptr(scratch), scratch.numel(), _lib.ptr(dl),
            _lib.ptr(grads), _lib.stream_ptr(None)), "rsaf_cnnlstm_train_backward")
        ctx.bufs = None
        return (None, None, None, *_unpack_grads(ctx.segs, ctx.params, grads))


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
        self.forced_masks = None            # tests: explicit dropout masks for the next training-mode forward

    def _weights_key(self, device):
        return (str(device),) + tuple((p.data_ptr(), p._version) for p in
                                      list(self.parameters()) + list(self.buffers()))

    def packed_weights(self, device):
        """Folded weight blob on ``device`` (rebuilt when any parameter/buffer changed)."""
        key = self._weights_key(device)
        if self._packed is None or self._packed_key != key:
            self._packed = torch.from_numpy(pack_weights(self)).to(device)
            self._packed_key = key
        return self._packed

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.RsafError("CNNLSTM.forward needs a HIP (cuda) tensor: there is no CPU fallback")
        x = x.to(torch.float32)
        if self.training:
            if x.dim() != 3 or x.shape[2] != self.dims["input_dim"]:
                raise ValueError(f"expected input [B, T, {self.dims['input_dim']}], got {tuple(x.shape)}")
            if x.shape[0] * (x.shape[1] // 2) <= 1:
                # nn.BatchNorm1d in training mode (res_block2 sees B * (T // 2) values per channel)
                raise ValueError("Expected more than 1 value per channel when training")
            x = x.contiguous()
            masks = self.forced_masks if self.forced_masks is not None else draw_masks(self, x.shape[0], x.shape[1], x.device)
            params = [p for _, _, _, outs in _train_segments(self)[0] for p, _ in outs]
            return _TrainStep.apply(x.detach(), self, masks, *params)
        blob = self.packed_weights(x.device)
        with torch.no_grad():
            logits, self._workspace = cnnlstm_forward_packed(x, blob, self.dims, self.activation_name,
                                                             self._workspace)
        return logits


def cnnlstm_forward_stages(model: "CNNLSTM", x):
    """Eval-mode forward that also returns what the reference's sub-modules return (forward hooks on
    ``res_block1`` / ``res_block2`` / ``lstm`` / ``attention_pooling`` of ``src/models.py``), channels-last:
    dict(res1 [B,T,C], res2 [B,T/2,C], lstm [B,T/2,2H], pooled [B,2H], logits [B,NC])."""
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.RsafError("cnnlstm_forward_stages needs a HIP (cuda) tensor")
    d = model.dims
    x = x.to(torch.float32).contiguous()
    B, T, D = x.shape
    blob = model.packed_weights(x.device)
    need = lib.rsaf_cnnlstm_workspace_bytes(B, T, D, d["channels"], d["hidden"], d["layers"])
    if need < 0:
        raise ValueError("sequence length must be >= 2")
    ws = torch.empty(max(int(need), 16) // 4, dtype=torch.float32, device=x.device)
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)            # noqa: E731
    out = {"res1": e(B, T, d["channels"]), "res2": e(B, T // 2, d["channels"]), "lstm": e(B, T // 2, 2 * d["hidden"]),
           "pooled": e(B, 2 * d["hidden"]), "logits": e(B, d["num_classes"])}
    _lib.check(lib.rsaf_cnnlstm_forward_stages(
        _lib.ptr(x), B, T, D, d["channels"], d["hidden"], d["num_classes"], d["layers"], _ACT_CODE[model.activation_name],
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


# ---- group training step: K independent replicas of one architecture in one step --------------------------------------
# The reference trains models of identical architecture and hyper-parameters on different data one after another (the
# inner folds of an Optuna trial, ``src/dl_cv_strategies.py:224-251``; the folds of ``:399-422``).  One such training
# keeps 2 of the chip's 256 CUs busy during its LSTM recurrences, which are most of the step; K of them side by side
# put the recurrences of all replicas into one launch per layer and pass (``rsaf_cnnlstm_train_forward_group`` /
# ``_backward_group``).  Everything else runs per replica, so the results are those of K separate steps, bit for bit.
# The eval-mode half of the same loops (the validation pass of every epoch, ``:131-139``; ``_eval_model``, ``:183-194``)
# is grouped further below (``cnnlstm_forward_group``): there every batch of every model is an item of its own, since no
# weight changes during a pass.

def train_group_max():
    """Replicas per C call (``rsaf_cnnlstm_train_group_max``); longer lists are split into chunks of this size."""
    return int(_lib.load().rsaf_cnnlstm_train_group_max())


def _group_call(fn, what, reps, dims, act, backward):
    """One ``rsaf_cnnlstm_train_{forward,backward}_group`` call per chunk of ``train_group_max()`` replicas."""
    gmax = train_group_max()
    optr = lambda t: t.data_ptr() if t is not None else None                         # noqa: E731
    for c0 in range(0, len(reps), gmax):
        chunk = reps[c0:c0 + gmax]
        items = (_lib.TrainItem * len(chunk))()
        for it, r in zip(items, chunk):
            mk = r["masks"]
            it.x, it.B, it.T, it.params = r["x"].data_ptr(), r["B"], r["T"], r["blob"].data_ptr()
            it.mask_block1, it.mask_block2, it.mask_fc = optr(mk["res_block1"]), optr(mk["res_block2"]), optr(mk["fc"])
            it.mask_lstm_host = C.cast(r["lstm_ptrs"], C.c_void_p) if r["lstm_ptrs"] is not None else None
            it.saved, it.saved_floats = r["saved"].data_ptr(), r["saved"].numel()
            it.scratch, it.scratch_floats = r["scratch"].data_ptr(), r["scratch"].numel()
            if backward:
                it.dlogits, it.grads = r["dlogits"].data_ptr(), r["grads"].data_ptr()
            else:
                it.logits, it.bn_stats_out = r["logits"].data_ptr(), r["stats"].data_ptr()
        _lib.check(fn(items, len(chunk), dims["input_dim"], dims["channels"], dims["hidden"], dims["num_classes"],
                      dims["layers"], _ACT_CODE[act], _lib.stream_ptr(None)), what)


class _TrainGroupStep(torch.autograd.Function):
    """(logits_0, ..., logits_K-1) of K replicas in training mode; backward fills the parameter gradients of every
    replica whose output received a gradient."""

    @staticmethod
    def forward(ctx, models, xs, masks, *params):
        lib = _lib.load()
        ctx.set_materialize_grads(False)          # an output outside the loss arrives as None, not as zeros
        d = models[0].dims
        reps, p0 = [], 0
        for model, x, mk in zip(models, xs, masks):
            B, T, D = x.shape
            segs, blob = _pack_train_blob(model, x.device)
            a = (B, T, D, d["channels"], d["hidden"], d["layers"])
            n_saved, n_scr = int(lib.rsaf_cnnlstm_train_saved_floats(*a)), int(lib.rsaf_cnnlstm_train_scratch_floats(*a))
            if n_saved < 0 or n_scr < 0:
                raise ValueError("sequence length must be >= 2")
            if model._train_scratch is None or model._train_scratch.numel() < n_scr or model._train_scratch.device != x.device:
                model._train_scratch = torch.empty(n_scr, dtype=torch.float32, device=x.device)
            n_par = sum(len(outs) for _, _, _, outs in segs)
            reps.append({"model": model, "x": x, "B": B, "T": T, "segs": segs, "blob": blob, "masks": mk,
                         "lstm_ptrs": _lstm_mask_ptrs(mk), "scratch": model._train_scratch,
                         "saved": torch.empty(n_saved, dtype=torch.float32, device=x.device),
                         "logits": torch.empty((B, d["num_classes"]), dtype=torch.float32, device=x.device),
                         "stats": torch.empty((5, 3, d["channels"]), dtype=torch.float32, device=x.device),
                         "params": params[p0:p0 + n_par]})
            p0 += n_par
        ctx.reps, ctx.dims, ctx.act = reps, d, models[0].activation_name
        _group_call(lib.rsaf_cnnlstm_train_forward_group, "rsaf_cnnlstm_train_forward_group", reps, d, ctx.act, False)
        for r in reps:
            _update_running_stats(r["model"], r["stats"], r["B"], r["T"])
        return tuple(r["logits"] for r in reps)

    @staticmethod
    def backward(ctx, *dlogits):
        lib = _lib.load()
        if ctx.reps is None:
            raise RuntimeError("CNNLSTM group training step: backward can run once per forward (the saved activations "
                               "are consumed)")
        live = []
        for r, dl in zip(ctx.reps, dlogits):
            if dl is None:
                continue
            if r["scratch"] is not r["model"]._train_scratch:
                r["scratch"] = torch.empty_like(r["scratch"])
            r["dlogits"] = dl.to(torch.float32).contiguous()
            r["grads"] = torch.zeros_like(r["blob"])
            live.append(r)
        _group_call(lib.rsaf_cnnlstm_train_backward_group, "rsaf_cnnlstm_train_backward_group", live, ctx.dims, ctx.act, True)
        out = []
        for r, dl in zip(ctx.reps, dlogits):
            out += [None] * len(r["params"]) if dl is None else _unpack_grads(r["segs"], r["params"], r["grads"])
        ctx.reps = None
        return (None, None, None, *out)


def _check_train_group(models, xs, masks, who):
    """Argument checks of a group training step; returns (models, float32 contiguous inputs, one mask set per replica:
    ``masks[k]``, else the model's ``forced_masks``, else drawn from torch's device RNG, replica by replica)."""
    models, xs = list(models), list(xs)
    if not models:
        raise ValueError(f"{who} needs at least one replica")
    if len(models) != len(xs):
        raise ValueError(f"{len(models)} models but {len(xs)} inputs")
    if masks is not None and len(masks) != len(models):
        raise ValueError(f"{len(models)} models but {len(masks)} mask sets")
    first = models[0]
    seen_modules, seen_params = {}, {}
    for k, m in enumerate(models):
        if m.dims != first.dims or m.activation_name != first.activation_name:
            raise ValueError(f"replica {k} differs from replica 0: dims {m.dims} / activation {m.activation_name!r} against "
                             f"{first.dims} / {first.activation_name!r}")
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
    D = first.dims["input_dim"]
    for k, x in enumerate(xs):
        if x.dim() != 3 or x.shape[2] != D:
            raise ValueError(f"replica {k}: expected input [B, T, {D}], got {tuple(x.shape)}")
        if x.shape[0] * (x.shape[1] // 2) <= 1:
            raise ValueError(f"replica {k}: Expected more than 1 value per channel when training")
    for k, x in enumerate(xs):
        if not x.is_cuda:
            raise _lib.RsafError(f"{who} needs HIP (cuda) tensors (replica {k}): there is no CPU fallback")
    xs = [x.detach().to(torch.float32).contiguous() for x in xs]
    mks = []
    for k, (m, x) in enumerate(zip(models, xs)):
        mk = masks[k] if masks is not None else None
        if mk is None:
            mk = m.forced_masks if m.forced_masks is not None else draw_masks(m, x.shape[0], x.shape[1], x.device)
        mks.append(mk)
    return models, xs, mks


def cnnlstm_train_group(models, xs, masks=None):
    """One training-mode forward of K independent ``CNNLSTM`` replicas (same ``dims`` and activation; own weights, own
    batch ``xs[k]`` of own shape [B_k, T_k, D]) -> list of K logits tensors.  Sum the K losses and call ``backward()``
    once: the replicas share nothing, so each model's ``.grad`` is the gradient of its own loss, and an output that
    stays out of the loss leaves its model without gradients.  Logits, gradients and BatchNorm buffers are those of K
    separate ``model(x)`` steps, bit for bit; the LSTM recurrences of all replicas run in one launch per layer and pass.

    ``masks[k]``: dropout keep masks in the format of ``draw_masks``; ``None`` (for the list or an entry) uses the
    model's ``forced_masks`` if set and draws them from torch's device RNG otherwise, replica by replica."""
    models, xs, mks = _check_train_group(models, xs, masks, "cnnlstm_train_group")
    params = [p for m in models for _, _, _, outs in _train_segments(m)[0] for p, _ in outs]
    return list(_TrainGroupStep.apply(models, xs, mks, *params))


# ---- fused training step: cross-entropy, Adam and the running statistics in HIP ------------------------------------------
# Around the model the reference's loop runs ``nn.CrossEntropyLoss()``, ``loss.backward()`` and ``Adam.step()``
# (``src/dl_cv_strategies.py:122-125,236-248``).  Through autograd that costs, per replica and step, the packing of the
# parameter blob, the unpacking of the gradient blob, the BatchNorm buffer updates and the loss and optimizer kernels of
# torch: elementwise work on a few hundred thousand floats spread over 100+ small ops.  Here the blob is written from the
# parameters where they live (``rsaf_cnnlstm_pack_params_group``), ``rsaf_cnnlstm_adam_group`` reads the gradient blob and
# updates the parameters in their torch layouts, the loss and its gradient come from ``rsaf_ce_loss_group`` and the running
# statistics from ``rsaf_bn_running_stats_group``: one launch each per group step.

def _adam_order(model):
    """The parameters in the numbering of ``rsaf_cnnlstm_adam_group`` (blob order; include/rsaf.h)."""
    order = [p for _, _, _, outs in _train_segments(model)[0] for p, _ in outs]
    d = model.dims
    n = int(_lib.load().rsaf_cnnlstm_adam_param_count(d["input_dim"], d["channels"], d["hidden"], d["num_classes"], d["layers"]))
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
    versions of everything written are bumped: ``packed_weights()`` and every other version-keyed cache see the change."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
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
        params = list(model.parameters())
        if any(not p.is_cuda for p in params):
            raise ValueError("FusedAdam: the CNNLSTM must be on a HIP device (model.to('cuda') first): there is no CPU fallback")
        if any(p.dtype != torch.float32 for p in params):
            raise ValueError("FusedAdam: the parameters must be float32")
        # the keys of torch.optim.Adam's own param_groups, so that state dicts load in both directions
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps).defaults)
        super().__init__(params, defaults)
        self.model = model
        self._order = _adam_order(model)
        self._steps = None                  # step count per parameter of _order (host mirror of state[p]['step']), None = unknown
        self._state_gen = 0                 # bumped whenever a moment tensor is created or replaced
        self._table = self._table_key = None
        self._blob = None                   # blob buffer of the fused step, rewritten from the parameters every step

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
        for i, p in enumerate(self._order):
            if not (skip >> i) & 1 and "exp_avg" not in self.state[p]:
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
        live = [i for i in range(len(self._order)) if not (skip >> i) & 1]
        torch._foreach_add_([self.state[self._order[i]]["step"] for i in live], 1)
        for i in live:
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
        ``rsaf_cnnlstm_train_backward_group`` writes); parameters with ``requires_grad = False`` are left alone."""
        total = train_param_offsets(self.model.dims)[1]
        if not grads.is_cuda or grads.dtype != torch.float32 or grads.shape != (total,) or not grads.is_contiguous():
            raise ValueError(f"expected a contiguous float32 HIP (cuda) gradient blob of {total} floats")
        skip = self._frozen()
        if skip == (1 << len(self._order)) - 1:
            return
        self._ensure_state(skip)
        _adam_group([(self, grads, self._cached_table(), skip)])
        self._written([p for i, p in enumerate(self._order) if not (skip >> i) & 1])

    @torch.no_grad()
    def step(self, closure=None):
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
        if skip == (1 << len(self._order)) - 1:
            return loss
        self._ensure_state(skip)
        rows = self._rows() + [[g.data_ptr() if g is not None else 0 for g in grads]]
        table = _pointer_table(rows, self._order[0].device)
        _adam_group([(self, None, table, skip)])
        self._written([p for i, p in enumerate(self._order) if not (skip >> i) & 1])
        return loss


def _adam_group(entries):
    """``entries``: [(optimizer, gradient blob or None, pointer table, skip mask)] of one architecture ->
    ``rsaf_cnnlstm_adam_group`` in chunks of ``train_group_max()``; a replica whose parameters stand at different step
    counts takes one launch per count."""
    lib = _lib.load()
    gmax = train_group_max()
    d = entries[0][0].model.dims
    plans = [opt._launches(skip) for opt, _, _, skip in entries]
    for j in range(max(len(pl) for pl in plans)):
        live = [(e, pl[j]) for e, pl in zip(entries, plans) if j < len(pl)]
        for c0 in range(0, len(live), gmax):
            chunk = live[c0:c0 + gmax]
            items = (_lib.AdamItem * len(chunk))()
            for it, ((opt, grads, table, _), (t, mask)) in zip(items, chunk):
                it.grads = grads.data_ptr() if grads is not None else None
                it.table, it.skip, it.step = table.data_ptr(), mask, t
                it.lr, it.beta1, it.beta2, it.eps = opt._hyper()
            _lib.check(lib.rsaf_cnnlstm_adam_group(items, len(chunk), d["input_dim"], d["channels"], d["hidden"],
                                                   d["num_classes"], d["layers"], _lib.stream_ptr(None)), "rsaf_cnnlstm_adam_group")
    for opt, _, _, skip in entries:
        opt._stepped(skip)


def _pack_group(optimizers):
    """The parameter blobs of the optimizers' models, written on the device from the parameters where they live: one
    launch of ``rsaf_cnnlstm_pack_params_group`` per chunk of ``train_group_max()``."""
    lib = _lib.load()
    gmax = train_group_max()
    d = optimizers[0].model.dims
    blobs = [opt._blob_buffer() for opt in optimizers]
    tables = [opt._cached_table() for opt in optimizers]
    for c0 in range(0, len(optimizers), gmax):
        n = min(gmax, len(optimizers) - c0)
        items = (_lib.PackItem * n)()
        for j, it in enumerate(items):
            it.table, it.params = tables[c0 + j].data_ptr(), blobs[c0 + j].data_ptr()
        _lib.check(lib.rsaf_cnnlstm_pack_params_group(items, n, d["input_dim"], d["channels"], d["hidden"], d["num_classes"],
                                                      d["layers"], _lib.stream_ptr(None)), "rsaf_cnnlstm_pack_params_group")
    return blobs


def ce_loss_group(logits, labels, with_grad=True):
    """Mean-reduced cross-entropy of K (logits [B_k, nc], int64 labels [B_k]) pairs in one launch of
    ``rsaf_ce_loss_group`` (``nn.CrossEntropyLoss()`` with its defaults) -> (losses [K] on the device, list of
    d loss_k / d logits_k, or None without ``with_grad``).  Lists longer than ``train_group_max()`` are chunked."""
    lib = _lib.load()
    logits, labels = list(logits), list(labels)
    if len(logits) != len(labels) or not logits:
        raise ValueError(f"{len(logits)} logits but {len(labels)} label tensors")
    nc, device = logits[0].shape[1], logits[0].device
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
    gmax = train_group_max()
    for c0 in range(0, len(logits), gmax):
        n = min(gmax, len(logits) - c0)
        items = (_lib.CeLossItem * n)()
        for j, it in enumerate(items):
            k = c0 + j
            it.logits, it.labels, it.B = logits[k].data_ptr(), labs[k].data_ptr(), logits[k].shape[0]
            it.loss_out = losses.data_ptr() + 4 * k
            it.dlogits_out = dl[k].data_ptr() if with_grad else None
        _lib.check(lib.rsaf_ce_loss_group(items, n, nc, _lib.stream_ptr(None)), "rsaf_ce_loss_group")
    return losses, dl


def _bn_running_group(reps, channels):
    """Running statistics of the replicas ``reps`` (dicts with model, stats, B, T) after a step: one launch of
    ``rsaf_bn_running_stats_group`` per chunk, ``num_batches_tracked`` incremented on the host side in one foreach op.
    A replica with a ``momentum=None`` layer (cumulative average) takes the torch ops of ``_update_running_stats``.
    Returns the buffers written."""
    lib = _lib.load()
    fused, counters, written = [], [], []
    for r in reps:
        bns = [bn for bn in _bn_modules(r["model"]) if bn is not None and bn.track_running_stats and bn.running_mean is not None]
        written += [t for bn in bns for t in (bn.running_mean, bn.running_var)]
        if any(bn.momentum is None for bn in bns):
            _update_running_stats(r["model"], r["stats"], r["B"], r["T"])
        elif bns:
            fused.append(r)
            counters += [bn.num_batches_tracked for bn in bns]
    gmax = train_group_max()
    for c0 in range(0, len(fused), gmax):
        chunk = fused[c0:c0 + gmax]
        items = (_lib.BnRunningItem * len(chunk))()
        for it, r in zip(items, chunk):
            B, T = r["B"], r["T"]
            it.stats = r["stats"].data_ptr()
            for i, (bn, n) in enumerate(zip(_bn_modules(r["model"]), (B * T, B * T, B * T, B * (T // 2), B * (T // 2)))):
                if bn is None or not bn.track_running_stats or bn.running_mean is None:
                    continue
                if not (bn.running_mean.is_contiguous() and bn.running_var.is_contiguous()
                        and bn.running_mean.dtype == bn.running_var.dtype == torch.float32):
                    raise _lib.RsafError("the BatchNorm running statistics must be contiguous float32 tensors")
                it.running_mean[i], it.running_var[i] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
                it.momentum[i], it.unbias[i] = float(bn.momentum), (n / (n - 1.0) if n > 1 else 1.0)
        _lib.check(lib.rsaf_bn_running_stats_group(items, len(chunk), channels, _lib.stream_ptr(None)), "rsaf_bn_running_stats_group")
    if counters:
        torch._foreach_add_(counters, 1)
    return written


def _train_step_chunk(models, optimizers, xs, labels, masks):
    """The fused step of up to ``train_group_max()`` replicas -> (losses [K], [logits_k])."""
    lib = _lib.load()
    d, act, device = models[0].dims, models[0].activation_name, xs[0].device
    K, nc, C = len(models), d["num_classes"], d["channels"]
    rows = [x.shape[0] for x in xs]
    logits_all = torch.empty((sum(rows), nc), dtype=torch.float32, device=device)
    stats_all = torch.empty((K, 5, 3, C), dtype=torch.float32, device=device)
    logits = list(torch.split(logits_all, rows))
    blobs = _pack_group(optimizers)
    reps = []
    for k, (model, opt, x, mk) in enumerate(zip(models, optimizers, xs, masks)):
        B, T, D = x.shape
        blob = blobs[k]
        a = (B, T, D, C, d["hidden"], d["layers"])
        n_saved, n_scr = int(lib.rsaf_cnnlstm_train_saved_floats(*a)), int(lib.rsaf_cnnlstm_train_scratch_floats(*a))
        if n_saved < 0 or n_scr < 0:
            raise ValueError("sequence length must be >= 2")
        if model._train_scratch is None or model._train_scratch.numel() < n_scr or model._train_scratch.device != device:
            model._train_scratch = torch.empty(n_scr, dtype=torch.float32, device=device)
        reps.append({"model": model, "x": x, "B": B, "T": T, "blob": blob, "masks": mk, "lstm_ptrs": _lstm_mask_ptrs(mk),
                     "scratch": model._train_scratch, "saved": torch.empty(n_saved, dtype=torch.float32, device=device),
                     "logits": logits[k], "stats": stats_all[k]})
    _group_call(lib.rsaf_cnnlstm_train_forward_group, "rsaf_cnnlstm_train_forward_group", reps, d, act, False)
    losses, dl = ce_loss_group(logits, labels)
    grads = torch.zeros((K, blob.numel()), dtype=torch.float32, device=device)       # one zero fill for the group
    for k, r in enumerate(reps):
        r["dlogits"], r["grads"] = dl[k], grads[k]
    _group_call(lib.rsaf_cnnlstm_train_backward_group, "rsaf_cnnlstm_train_backward_group", reps, d, act, True)
    entries = []
    for k, opt in enumerate(optimizers):
        skip = opt._frozen()
        opt._ensure_state(skip)
        entries.append((opt, grads[k], opt._cached_table(), skip))
    live = [e for e in entries if e[3] != (1 << len(e[0]._order)) - 1]
    if live:
        _adam_group(live)
    buffers = _bn_running_group(reps, C)
    for opt, _, _, skip in entries:
        own = set(id(t) for t in opt.model.buffers())
        opt._written([p for i, p in enumerate(opt._order) if not (skip >> i) & 1] + [t for t in buffers if id(t) in own])
    return losses, logits


def cnnlstm_train_step_group(models, optimizers, xs, labels, masks=None):
    """One whole training step of K independent ``CNNLSTM`` replicas, ``optimizers[k]`` the ``FusedAdam`` of ``models[k]``:
    group forward in training mode, ``nn.CrossEntropyLoss()`` (defaults) of ``labels[k]``, group backward, Adam and the
    BatchNorm running statistics -> ``(losses [K] on the device, [logits_k])``.  No autograd graph is built and ``.grad``
    is not touched; the packing of the parameter blobs, the loss, the optimizer and the running statistics are one launch
    each for the group.  A parameter with ``requires_grad = False`` keeps its value and its moments.

    Arguments are checked as ``cnnlstm_train_group`` checks them; ``masks`` as there (``forced_masks`` are honoured, and
    masks are drawn replica by replica in the same order, so with equal RNG state both paths see equal masks).  Lists
    longer than ``train_group_max()`` are split into chunks of that size."""
    optimizers, labels = list(optimizers), list(labels)
    models, xs, mks = _check_train_group(models, xs, masks, "cnnlstm_train_step_group")
    if not (len(optimizers) == len(labels) == len(models)):
        raise ValueError(f"{len(models)} models, {len(optimizers)} optimizers and {len(labels)} label tensors")
    for k, (m, opt) in enumerate(zip(models, optimizers)):
        if not isinstance(opt, FusedAdam) or opt.model is not m:
            raise ValueError(f"optimizers[{k}] is not the FusedAdam of models[{k}]")
    for k, (x, lab) in enumerate(zip(xs, labels)):
        if lab.dim() != 1 or lab.shape[0] != x.shape[0] or lab.dtype.is_floating_point:
            raise ValueError(f"replica {k}: expected {x.shape[0]} integer class labels, got {lab.dtype} {tuple(lab.shape)}")
    gmax = train_group_max()
    losses, logits = [], []
    with torch.no_grad():
        for c0 in range(0, len(models), gmax):
            s = slice(c0, c0 + gmax)
            ls, lg = _train_step_chunk(models[s], optimizers[s], xs[s], labels[s], mks[s])
            losses.append(ls)
            logits += lg
    return (losses[0] if len(losses) == 1 else torch.cat(losses)), logits


def _fused_step_applies(optimizers, models, loss_fn):
    """The lockstep loops take the fused step when the loss is ``nn.CrossEntropyLoss`` with its default options and
    every optimizer is the ``FusedAdam`` of its model."""
    if type(loss_fn) is not nn.CrossEntropyLoss or loss_fn.weight is not None or loss_fn.reduction != "mean" \
            or loss_fn.label_smoothing != 0 or loss_fn.ignore_index != -100:
        return False
    return all(isinstance(o, FusedAdam) and o.model is m for o, m in zip(optimizers, models))


# ---- group eval forward: K independent eval-mode forwards of one architecture in one call --------------------------------
# ``rsaf_cnnlstm_forward_group``: the recurrences of all items in one launch per layer, their heads in one launch, the
# fp16 planes of the weights once per distinct model; everything else per item.  The logits are those of ``model(x)``,
# bit for bit.

_group_workspace = {}               # device -> cached workspace tensor of the group calls (grown on demand)
_WS_ALIGN = 256                     # bytes between the items' slices


def _group_forward_chunk(lib, items, dims, act, device):
    """One C call: ``items`` = [(x, blob)] with B >= 1 -> list of logits (views of one tensor)."""
    a = (dims["input_dim"], dims["channels"], dims["hidden"], dims["layers"])
    needs = [int(lib.rsaf_cnnlstm_workspace_bytes(x.shape[0], x.shape[1], *a)) for x, _ in items]
    offs, total = [], 0
    for n in needs:
        offs.append(total)
        total += (n + _WS_ALIGN - 1) // _WS_ALIGN * _WS_ALIGN
    ws = _group_workspace.get(str(device))
    if ws is None or ws.numel() * 4 < total:
        ws = _group_workspace[str(device)] = torch.empty(total // 4, dtype=torch.float32, device=device)
    nc = dims["num_classes"]
    rows = [x.shape[0] for x, _ in items]
    logits = torch.empty((sum(rows), nc), dtype=torch.float32, device=device)
    arr = (_lib.ForwardItem * len(items))()
    r0 = 0
    for it, (x, blob), n, off, B in zip(arr, items, needs, offs, rows):
        it.x, it.B, it.T, it.weights = x.data_ptr(), B, x.shape[1], blob.data_ptr()
        it.workspace, it.workspace_bytes = ws.data_ptr() + off, n
        it.logits = logits.data_ptr() + r0 * nc * 4
        r0 += B
    _lib.check(lib.rsaf_cnnlstm_forward_group(arr, len(items), dims["input_dim"], dims["channels"], dims["hidden"], nc,
                                              dims["layers"], _ACT_CODE[act], _lib.stream_ptr(None)),
               "rsaf_cnnlstm_forward_group")
    return list(torch.split(logits, rows))


def cnnlstm_forward_group(models, xs):
    """Eval-mode forward of the pairs ``(models[i], xs[i])`` (same ``dims`` and activation; ``xs[i]`` of own shape
    [B_i, T_i, D]) under ``no_grad`` -> list of logits tensors, each equal to ``models[i](xs[i])`` bit for bit.  ``models``
    may name the same module several times (the batches of one validation loader): its weights are packed and split
    once.  Lists longer than ``train_group_max()`` are split into chunks of that size."""
    models, xs = list(models), list(xs)
    if not models:
        raise ValueError("cnnlstm_forward_group needs at least one (model, input) pair")
    if len(models) != len(xs):
        raise ValueError(f"{len(models)} models but {len(xs)} inputs")
    first = models[0]
    for k, m in enumerate(models):
        if m.dims != first.dims or m.activation_name != first.activation_name:
            raise ValueError(f"replica {k} differs from replica 0: dims {m.dims} / activation {m.activation_name!r} against "
                             f"{first.dims} / {first.activation_name!r}")
        if m.training:
            raise ValueError(f"replica {k} is in training mode: the group forward is the inference forward (model.eval())")
    D = first.dims["input_dim"]
    for k, x in enumerate(xs):
        if x.dim() != 3 or x.shape[2] != D:
            raise ValueError(f"replica {k}: expected input [B, T, {D}], got {tuple(x.shape)}")
        if x.shape[0] > 0 and x.shape[1] < 2:
            raise ValueError(f"replica {k}: sequence length must be >= 2")
    for k, x in enumerate(xs):
        if not x.is_cuda:
            raise _lib.RsafError(f"cnnlstm_forward_group needs HIP (cuda) tensors (replica {k}): there is no CPU fallback")
    lib = _lib.load()
    gmax = train_group_max()
    device = xs[0].device
    with torch.no_grad():
        blobs = {}
        for m in models:
            if id(m) not in blobs:
                blobs[id(m)] = m.packed_weights(device)
        xs = [x.detach().to(torch.float32).contiguous() for x in xs]
        outs = [None] * len(xs)
        live = [k for k, x in enumerate(xs) if x.shape[0] > 0]
        for k in range(len(xs)):
            if xs[k].shape[0] == 0:
                outs[k] = torch.empty((0, first.dims["num_classes"]), dtype=torch.float32, device=device)
        for c0 in range(0, len(live), gmax):
            chunk = live[c0:c0 + gmax]
            got = _group_forward_chunk(lib, [(xs[k], blobs[id(models[k])]) for k in chunk], first.dims, first.activation_name, device)
            for k, o in zip(chunk, got):
                outs[k] = o
    return outs


class CNNLSTMGroup(nn.Module):
    """K ``CNNLSTM`` replicas of one architecture that train side by side.  ``forward(xs)`` takes one batch per replica
    (``None``: the replica sits out and its output is ``None``): in training mode the group step over the others, in
    eval mode the group inference forward over them (``cnnlstm_forward_group``).  ``state_dict`` keys are ``models.<k>.<reference key>``, so a
    replica's weights load into a plain ``CNNLSTM``."""

    def __init__(self, models):
        super().__init__()
        self.models = nn.ModuleList(models)
        if len(self.models) == 0:
            raise ValueError("CNNLSTMGroup needs at least one replica")
        for k, m in enumerate(self.models):
            if not isinstance(m, CNNLSTM):
                raise TypeError(f"replica {k} is a {type(m).__name__}, not a CNNLSTM")

    def forward(self, xs):
        xs = list(xs)
        if len(xs) != len(self.models):
            raise ValueError(f"{len(self.models)} replicas but {len(xs)} inputs")
        live = [k for k, x in enumerate(xs) if x is not None]
        outs = [None] * len(xs)
        if self.training:
            if live:
                for k, o in zip(live, cnnlstm_train_group([self.models[k] for k in live], [xs[k] for k in live])):
                    outs[k] = o
        elif live:
            for k, o in zip(live, cnnlstm_forward_group([self.models[k] for k in live], [xs[k] for k in live])):
                outs[k] = o
        return outs


def train_replicas_lockstep(models, optimizers, loaders, loss_fn, epochs, device):
    """The reference's inner training loop (``src/dl_cv_strategies.py:244-248``: ``zero_grad / model(seq) / loss /
    backward / step`` per batch, a fixed number of epochs) for K replicas over K loaders in lock step: step i of an
    epoch takes batch i of every loader through one group step.  Loaders may differ in length; a replica whose epoch
    is exhausted sits out until the others finish theirs.  Returns the mean training loss per epoch of every replica
    (``histories[k][epoch]``, accumulated as the reference's ``train_model`` does, ``:120-129``); the K losses of a
    step come to the host in one copy.

    Parameters, buffers and losses equal those of K sequential trainings bit for bit as long as the replicas see the
    same batches and dropout masks.  When ``loss_fn`` is ``nn.CrossEntropyLoss()`` with its default options and every
    optimizer of the call is the ``FusedAdam`` of its model, a step is one ``cnnlstm_train_step_group`` call (loss, Adam and running
    statistics in HIP, no autograd graph); anything else runs the loop above as written.  Note that ``DataLoader(shuffle=True)`` without a ``generator`` of its own draws
    its permutations from torch's global RNG: in lock step the K loaders draw in a different order than K sequential
    trainings would, so give every loader its own ``torch.Generator`` where the batch order matters.  The same holds
    for dropout masks, which come from the device RNG replica by replica within a step."""
    models, optimizers, loaders = list(models), list(optimizers), list(loaders)
    if not (len(models) == len(optimizers) == len(loaders)):
        raise ValueError(f"{len(models)} models, {len(optimizers)} optimizers and {len(loaders)} loaders")
    histories = [[] for _ in models]
    fused = _fused_step_applies(optimizers, models, loss_fn)      # decided once for the call: no replica changes path mid-epoch
    for _ in range(epochs):
        for m in models:
            m.train()
        its = [iter(ld) for ld in loaders]
        total, count = [0.0] * len(models), [0] * len(models)
        while True:
            batches = [next(it, None) for it in its]
            live = [k for k, b in enumerate(batches) if b is not None]
            if not live:
                break
            xs = [batches[k][0].to(device) for k in live]
            labs = [batches[k][1].to(device) for k in live]
            if fused:
                step_losses = cnnlstm_train_step_group([models[k] for k in live], [optimizers[k] for k in live], xs, labs)[0]
            else:
                for k in live:
                    optimizers[k].zero_grad()
                outs = cnnlstm_train_group([models[k] for k in live], xs)
                losses = [loss_fn(o, lab) for o, lab in zip(outs, labs)]
                torch.stack(losses).sum().backward()
                for k in live:
                    optimizers[k].step()
                step_losses = torch.stack([ls.detach() for ls in losses])
            for k, v in zip(live, step_losses.tolist()):
                total[k] += v
                count[k] += 1
        for k in range(len(models)):
            histories[k].append(total[k] / max(count[k], 1))
    return histories


def _grouped_eval_batches(pairs, device):
    """``pairs``: iterable of ``(tag, model, seq, lab)`` in any mix of models -> yields ``(tag, logits, lab on the device)``
    in the same order, the forwards pooled into group calls of up to ``train_group_max()`` batches.  The batches stay as
    collated: zero padding is not masked (``src/dl_cv_strategies.py:81-84``), so regrouping sequences would change the
    results."""
    gmax = train_group_max()
    pend = []

    def flush():
        outs = cnnlstm_forward_group([p[1] for p in pend], [p[2] for p in pend])
        res = [(p[0], o, p[3]) for p, o in zip(pend, outs)]
        pend.clear()
        return res

    for tag, model, seq, lab in pairs:
        pend.append((tag, model, seq.to(device), lab.to(device)))
        if len(pend) == gmax:
            yield from flush()
    if pend:
        yield from flush()


def eval_replicas_lockstep(models, loaders, device):
    """``_eval_model`` (``src/dl_cv_strategies.py:183-194``) for K models over K loaders: all (model, batch) pairs are
    pooled into group calls.  Returns K triples ``(labels, preds, probs)`` of NumPy arrays in loader order, equal to
    what the reference's loop returns model by model; the results of a replica come to the host in one copy each."""
    models, loaders = list(models), list(loaders)
    if len(models) != len(loaders):
        raise ValueError(f"{len(models)} models but {len(loaders)} loaders")
    for m in models:
        m.eval()
    parts = [([], [], []) for _ in models]
    with torch.no_grad():
        pairs = ((k, m, seq, lab) for k, (m, ld) in enumerate(zip(models, loaders)) for seq, lab in ld)
        for k, out, lab in _grouped_eval_batches(pairs, device):
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


def train_eval_replicas_lockstep(models, optimizers, schedulers, train_loaders, val_loaders, loss_fn, epochs, patience, device):
    """``_train_eval_loop`` (``src/dl_cv_strategies.py:112-165``) for K replicas: per epoch the training pass of
    ``train_replicas_lockstep`` over the replicas still running, then the validation pass of all of them in group calls
    (``val_loss`` accumulated batch by batch in loader order; the losses of a pass come to the host in one copy), then per
    replica ``scheduler.step(avg_val_loss)`` (``schedulers[k]`` may be ``None``), best-weights checkpointing and early
    stopping as the reference does them.  A replica that stopped early sits out of the later epochs.  Returns
    ``[(model, train_loss_history, val_loss_history)]``, every model with its best weights loaded."""
    models, optimizers, schedulers = list(models), list(optimizers), list(schedulers)
    train_loaders, val_loaders = list(train_loaders), list(val_loaders)
    K = len(models)
    if not (K == len(optimizers) == len(schedulers) == len(train_loaders) == len(val_loaders)):
        raise ValueError(f"{K} models, {len(optimizers)} optimizers, {len(schedulers)} schedulers, {len(train_loaders)} training "
                         f"loaders and {len(val_loaders)} validation loaders")
    train_hist, val_hist = [[] for _ in models], [[] for _ in models]
    best_val_loss = [float("inf")] * K
    epochs_no_improve = [0] * K
    best_model_weights = [None] * K
    running = list(range(K))
    for _ in range(epochs):
        if not running:
            break
        hist = train_replicas_lockstep([models[k] for k in running], [optimizers[k] for k in running],
                                       [train_loaders[k] for k in running], loss_fn, 1, device)
        for k, h in zip(running, hist):
            train_hist[k].append(h[0])
        for k in running:
            models[k].eval()
        tags, outs, labs = [], [], []
        fused = _fused_step_applies([optimizers[k] for k in running], [models[k] for k in running], loss_fn)
        with torch.no_grad():
            pairs = ((k, models[k], seq, lab) for k in running for seq, lab in val_loaders[k])
            for k, out, lab in _grouped_eval_batches(pairs, device):
                tags.append(k)
                outs.append(out)
                labs.append(lab)
            if not outs:
                losses = []
            elif fused and all(o.shape[0] > 0 for o in outs):           # the losses of the pass in group launches, no gradient
                losses = ce_loss_group(outs, labs, with_grad=False)[0].tolist()
            else:
                losses = torch.stack([loss_fn(o, lab) for o, lab in zip(outs, labs)]).tolist()
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
                epochs_no_improve[k] = 0
            else:
                epochs_no_improve[k] += 1
            if epochs_no_improve[k] < patience:
                still.append(k)
        running = still
    for k in range(K):
        if best_model_weights[k]:
            models[k].load_state_dict(best_model_weights[k])
    return [(models[k], train_hist[k], val_hist[k]) for k in range(K)]
