"""Cases shared by tests/test_collate_mix_gpu.py, test_layer_mix_adam_gpu.py and test_layer_mix_lockstep_gpu.py: layer stacks
from seeds, and the float64 restatement of one ragged training step with a three-layer mix in front of a geometry row.
Every host-side result is computed once and left unchanged."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cnnlstm_geometry as geo  # noqa: E402
import input_grad_cases as igc  # noqa: E402
import input_grad_restatement as igr  # noqa: E402

# (lengths, L, D): a member of no frames and L = 1; D / 4 = 5; 14 chunks per member, the last ragged, and 7 backward parts;
# L at its cap; 129 backward parts that straddle the members
CASES = [((5, 3, 0, 5), 1, 4), ((7, 2, 6), 2, 20), ((37, 11, 29, 1), 13, 768), ((33,), 32, 20), ((1367, 900), 2, 768)]
GROUP_CASES = [((7, 2, 6), 2, 20), ((9, 4), 13, 20), ((33,), 32, 20)]          # one width, L of 2, 13 and 32: one K = 3 call


def case_id(case):
    lengths, L, D = case
    return "t" + "_".join(map(str, lengths)) + f"_l{L}_d{D}"


@functools.lru_cache(maxsize=None)
def stacks(case):
    """The sequences [L, T_i, D] of a case (float32), p [L] (float32, sums to about 1) and dx [B, T, D] at 1e-3 scale, non-zero on
    the padded frames too; then the zero-padded stack h [B, L, T, D] built on the host."""
    lengths, L, D = case
    rng = np.random.Generator(np.random.PCG64(29000 + 31 * L + D + sum(lengths)))
    seqs = [rng.standard_normal((L, n, D)).astype(np.float32) for n in lengths]
    w = rng.uniform(-1.5, 1.5, L)
    p = (np.exp(w) / np.exp(w).sum()).astype(np.float32)
    T = max(lengths)
    dx = (1e-3 * rng.standard_normal((len(lengths), T, D))).astype(np.float32)
    h = np.zeros((len(lengths), L, T, D), np.float32)
    for b, s in enumerate(seqs):
        h[b, :, :s.shape[1]] = s
    return seqs, p, dx, h


# ---- one ragged step with a three-layer mix in front of a geometry row ---------------------------------------------------------
STEP_ROW = 2                                    # D = 16, C = 48, H = 64, silu, 5 classes, 3 LSTM layers
STEP_L = igc.MIX_L
STEP_WEIGHTS = igc.MIX_WEIGHTS


@functools.lru_cache(maxsize=None)
def step_case():
    """The row's own state dict, labels and masks at its (B, T); ragged lengths, the longest of them T; ``want``: the restatement
    (``input_grad_restatement.forward_backward``) at the float64 mix of the zero-padded stack; ``dp64``, ``dw64`` as in
    ``input_grad_cases.mix_case``."""
    D, C, H, act, NC, L, B, T = geo.CASES[STEP_ROW]
    sd = geo.state_dict(STEP_ROW)
    _, labels, mk = geo.train_inputs(STEP_ROW)
    rng = np.random.Generator(np.random.PCG64(29500))
    lengths = [T] + [int(n) for n in rng.integers(max(2, T // 2), T, B - 1)]
    seqs = [np.stack([geo.synth_input(1, n, D, 29600 + 10 * b + l)[0] for l in range(STEP_L)]) for b, n in enumerate(lengths)]
    h = np.zeros((B, STEP_L, T, D), np.float32)
    for b, s in enumerate(seqs):
        h[b, :, :s.shape[1]] = s
    p = igr.softmax64(STEP_WEIGHTS)
    want = igr.forward_backward(sd, igr.layer_mix(h, p), labels, act, masks=mk)
    dp64, _ = igr.layer_mix_dp(h, want["dx"])
    return {"seqs": seqs, "lengths": lengths, "h": h, "labels": labels, "masks": mk, "sd": sd, "p64": p, "want": want, "dp64": dp64,
            "dw64": igr.softmax_jacobian_apply(p, dp64)}
