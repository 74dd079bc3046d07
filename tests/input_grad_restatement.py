"""Float64 restatement of the CNN-LSTM training step with the input as a leaf, and of the learned mix of encoder layers.

TEST INFRASTRUCTURE: only tests/ use it.  ``forward_backward`` is ``oracle.cnnlstm_train_oracle.forward_backward`` with one
difference: ``x`` is a leaf of the graph, so autograd also returns ``dx`` = dLoss/dx [B, T, D] (zero-padded frames and the
odd last frame included: nothing is masked).  The ops and their order are the oracle's (``_bn_train`` and ``lstm_layer`` are
the oracle's own), so logits, loss and parameter gradients are the oracle's to the last bits
(tests/test_cnnlstm_input_grad.py holds them to 1e-12); ``dx`` is pinned by ``x.grad`` of the reference's own module
(tests/golden/cnnlstm_input_grad_*.npz, tests/golden/make_cnnlstm_input_grad_golden.py).

``layer_mix`` / ``layer_mix_dp``: x = sum_l softmax(w)_l h_l and dp_l = sum h_l . dx in float64.
"""
from __future__ import annotations

import numpy as np

from oracle.cnnlstm_train_oracle import _bn_train, _t, lstm_layer, n_lstm_layers


def forward_backward(sd, x, labels, activation_fn="silu", masks=None, grad_logits=None):
    """One training-mode forward + backward in float64 with ``x`` [B, T, D] as a leaf.  Returns what the oracle returns
    (``logits``, ``loss``, ``grads``, ``bn_stats``) plus ``dx`` [B, T, D] and ``stages`` (res1, res2, lstm, pooled)."""
    import torch
    import torch.nn.functional as F
    act = {"silu": F.silu, "gelu": F.gelu}.get(activation_fn)
    if act is None:
        raise ValueError(f"Unsupported activation function: {activation_fn}")
    P = {k: _t(v).requires_grad_(True) for k, v in sd.items()
         if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))}
    masks = masks or {}
    m = lambda k: _t(masks[k]) if k in masks else None                      # noqa: E731
    stats, st = {}, {}

    def block(h, p):
        o = act(_bn_train(F.conv1d(h, P[p + ".conv1.weight"], P[p + ".conv1.bias"], padding=1),
                          P[p + ".bn1.weight"], P[p + ".bn1.bias"], stats, p + ".bn1"))
        mk = m(p)
        if mk is not None:
            o = o * mk.permute(0, 2, 1)
        o = _bn_train(F.conv1d(o, P[p + ".conv2.weight"], P[p + ".conv2.bias"], padding=1),
                      P[p + ".bn2.weight"], P[p + ".bn2.bias"], stats, p + ".bn2")
        if (p + ".shortcut.0.weight") in P:
            s = _bn_train(F.conv1d(h, P[p + ".shortcut.0.weight"], P[p + ".shortcut.0.bias"]),
                          P[p + ".shortcut.1.weight"], P[p + ".shortcut.1.bias"], stats, p + ".shortcut.1")
        else:
            s = h
        return act(o + s)

    x_leaf = _t(x).requires_grad_(True)
    h = x_leaf.permute(0, 2, 1)
    h = block(h, "res_block1")
    st["res1"] = h.permute(0, 2, 1)
    h = F.max_pool1d(h, kernel_size=2)
    h = block(h, "res_block2")
    st["res2"] = h.permute(0, 2, 1)
    seq = h.permute(0, 2, 1)
    nl = n_lstm_layers(sd)
    for l in range(nl):
        outs = [lstm_layer(seq, P[f"lstm.weight_ih_l{l}{s}"], P[f"lstm.weight_hh_l{l}{s}"],
                           P[f"lstm.bias_ih_l{l}{s}"], P[f"lstm.bias_hh_l{l}{s}"], rev)
                for s, rev in (("", False), ("_reverse", True))]
        seq = torch.cat(outs, dim=2)
        if l < nl - 1 and m(f"lstm{l}") is not None:
            seq = seq * m(f"lstm{l}")
    st["lstm"] = seq
    sc = F.linear(seq, P["attention_pooling.attention_weights.weight"], P["attention_pooling.attention_weights.bias"])
    ctx = torch.sum(seq * F.softmax(sc, dim=1), dim=1)
    st["pooled"] = ctx
    if m("fc") is not None:
        ctx = ctx * m("fc")
    logits = F.linear(ctx, P["fc.weight"], P["fc.bias"])
    if grad_logits is not None:
        loss = None
        logits.backward(_t(grad_logits))
    else:
        loss = F.cross_entropy(logits, torch.as_tensor(np.asarray(labels), dtype=torch.long))
        loss.backward()
    return {"logits": logits.detach().numpy(), "loss": None if loss is None else loss.item(),
            "grads": {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in P.items()},
            "bn_stats": stats, "dx": x_leaf.grad.numpy().copy(),
            "stages": {k: v.detach().numpy() for k, v in st.items()}}


def softmax64(w):
    w = np.asarray(w, np.float64)
    e = np.exp(w - w.max())
    return e / e.sum()


def layer_mix(h, p):
    """x [B, T, D] = sum_l p[l] h[:, l] in float64 (``p``: the probabilities, not the weights)."""
    return np.einsum("l,bltd->btd", np.asarray(p, np.float64), np.asarray(h, np.float64))


def layer_mix_dp(h, dx):
    """dp [L] = sum_{b,t,d} h[b, l, t, d] dx[b, t, d] in float64, and sum |h_l dx| [L] for the error bound."""
    h64, d64 = np.asarray(h, np.float64), np.asarray(dx, np.float64)[:, None]
    prod = h64 * d64
    return prod.sum(axis=(0, 2, 3)), np.abs(prod).sum(axis=(0, 2, 3))


def softmax_jacobian_apply(p, dp):
    """dL/dw of w -> softmax(w) = p, given dL/dp: p * (dp - p . dp)."""
    p, dp = np.asarray(p, np.float64), np.asarray(dp, np.float64)
    return p * (dp - (p * dp).sum())
