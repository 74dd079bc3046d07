"""Float64 restatement of what the fused CNN-LSTM step does with class weights and a clipping norm, for the tests:
``nn.CrossEntropyLoss(weight=w)`` (reduction "mean"), ``clip_grad_norm_(parameters, max_norm)`` (2-norm) and the Adam
step of ``oracle.cnnlstm_train_oracle`` on the clipped gradients.  numpy only."""
import numpy as np

from oracle import cnnlstm_train_oracle as to


def weighted_cross_entropy(x, y, w):
    """loss = sum_b w[y_b] nll_b / sum_b w[y_b] and d loss / d x, for logits ``x`` [B, nc], labels ``y`` [B], weights ``w`` [nc]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    rows = np.arange(len(y))
    mx = x.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
    wy = w[y]
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = (wy * (lse - x[rows, y])).sum() / wy.sum()
        sm = np.exp(x - lse[:, None])
        sm[rows, y] -= 1.0
        return loss, wy[:, None] * sm / wy.sum()


def grad_norm(grads):
    """sqrt(sum_p ||g_p||^2) over the gradients of a dict (name -> array): every PARAMETER counts, so the two biases of an
    LSTM direction, which hold the same gradient, count twice."""
    return float(np.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads.values())))


def clip_scale(norm, max_norm):
    """What ``clip_grad_norm_`` multiplies the gradients by."""
    return min(1.0, max_norm / (norm + 1e-6))


def clipped_adam_step(params, grads, state, lr, max_norm):
    """``clip_grad_norm_`` then ``adam_step`` of the oracle, in place on float64 dicts -> (norm, scale)."""
    norm = grad_norm(grads)
    scale = clip_scale(norm, max_norm)
    to.adam_step(params, {k: np.asarray(g, np.float64) * scale for k, g in grads.items()}, state, lr)
    return norm, scale
