"""Learned mix of encoder layers on the HIP path: the usual consumer of all hidden states of a speech encoder.

``extract_wav2vec2_sequences(output_layers=[...])`` returns every requested layer's hidden states per file; padded to a batch
they are ``h`` [B, L, T, D].  ``LayerMix(L)`` holds one weight per layer and returns ``x[b, t, :] = sum_l p_l h[b, l, t, :]``
with ``p = softmax(weights)``: the input of the downstream classifier (``CNNLSTM``, whose training step returns the gradient
of its input), learned together with it.

``h`` is L + 1 times the size of ``x``, so forward and backward are one stream over it each (``rsaf_layer_mix_forward`` /
``rsaf_layer_mix_backward``, csrc/layer_mix.hip).  The softmax over the L weights and its Jacobian are two tiny torch ops on
[L]: the kernels take ``p`` and return ``dL/dp``, the latter accumulated in double over a partition that depends on the shape
alone and summed in a fixed order, so a step is reproducible bit for bit.  There is no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib

LAYER_MIX_MAX = 32            # RSAF_LAYER_MIX_MAX (include/rsaf.h)


def _check_h(h, L):
    if not h.is_cuda:
        raise _lib.RsafError("LayerMix needs a HIP (cuda) tensor: there is no CPU fallback")
    if h.dim() != 4 or h.shape[1] != L:
        raise ValueError(f"expected hidden states [B, {L}, T, D], got {tuple(h.shape)}")
    if h.dtype != torch.float32:
        raise ValueError(f"expected float32 hidden states, got {h.dtype}")
    if h.shape[0] < 1 or h.shape[2] < 1 or h.shape[3] < 4 or h.shape[3] % 4:
        raise ValueError(f"expected B >= 1, T >= 1 and D a positive multiple of 4, got {tuple(h.shape)}")


def layer_mix_forward(h, p):
    """``sum_l p[l] h[:, l]`` of float32 ``h`` [B, L, T, D] and ``p`` [L] on the device -> [B, T, D]; no graph."""
    B, L, T, D = h.shape
    x = torch.empty((B, T, D), dtype=torch.float32, device=h.device)
    _lib.check(_lib.load().rsaf_layer_mix_forward(_lib.ptr(h), B, L, T, D, _lib.ptr(p), _lib.ptr(x), _lib.stream_ptr(None)),
               "rsaf_layer_mix_forward")
    return x


def layer_mix_backward(h, dx):
    """``dp[l] = sum_{b,t,d} h[b, l, t, d] dx[b, t, d]`` -> float32 [L]; the same bits on every call."""
    B, L, T, D = h.shape
    lib = _lib.load()
    n = int(lib.rsaf_layer_mix_partials(B, L, T, D))
    if n < 0:
        raise ValueError(f"rsaf_layer_mix_partials refuses the shape {tuple(h.shape)}")
    partials = torch.empty(n, dtype=torch.float64, device=h.device)
    dp = torch.empty(L, dtype=torch.float32, device=h.device)
    _lib.check(lib.rsaf_layer_mix_backward(_lib.ptr(h), _lib.ptr(dx), B, L, T, D, _lib.ptr(partials), n, _lib.ptr(dp),
                                           _lib.stream_ptr(None)), "rsaf_layer_mix_backward")
    return dp


class _Mix(torch.autograd.Function):
    """x = sum_l p_l h_l.  backward: dL/dp from the HIP kernel; dL/dh, when asked for, is the outer product of ``p`` and
    ``dx`` as a torch expression (a cold path: the hidden states of a frozen encoder need none)."""

    @staticmethod
    def forward(ctx, h, p):
        ctx.save_for_backward(h, p)
        return layer_mix_forward(h, p)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dx):
        h, p = ctx.saved_tensors
        dx = dx.to(torch.float32).contiguous()
        dp = layer_mix_backward(h, dx) if ctx.needs_input_grad[1] else None
        dh = p[None, :, None, None] * dx[:, None] if ctx.needs_input_grad[0] else None
        return dh, dp


def layer_mix(h, p):
    """``sum_l p[l] h[:, l]`` on the autograd graph of ``p`` (and of ``h``, where it requires a gradient): float32 ``h``
    [B, L, T, D] on the device, ``p`` [L].  ``LayerMix`` calls it with the softmax of its weights."""
    _check_h(h, p.shape[0] if p.dim() == 1 else -1)
    return _Mix.apply(h.contiguous(), p.to(torch.float32).contiguous())


class LayerMix(nn.Module):
    """Softmax-weighted sum of ``num_layers`` encoder layers (1 <= num_layers <= 32): ``weights`` [L], initialised to zeros
    (the plain mean).  ``forward(h)``: float32 ``h`` [B, L, T, D] on the device, D a multiple of 4 -> [B, T, D]."""

    def __init__(self, num_layers):
        super().__init__()
        if not 1 <= int(num_layers) <= LAYER_MIX_MAX:
            raise ValueError(f"num_layers must be in [1, {LAYER_MIX_MAX}], got {num_layers}")
        self.num_layers = int(num_layers)
        self.weights = nn.Parameter(torch.zeros(self.num_layers))

    def forward(self, h):
        _check_h(h, self.num_layers)
        return layer_mix(h, torch.softmax(self.weights.to(torch.float32), dim=0))
