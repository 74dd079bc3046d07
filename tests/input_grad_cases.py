"""The cases of the input-gradient tests, shared by tests/test_cnnlstm_input_grad.py (no GPU: every input keeps the max-pool
gap on the float64 restatement alone) and tests/test_cnnlstm_input_grad_gpu.py (the HIP step against that restatement).

``DX_CASES``: the 12 rows of ``cnnlstm_geometry.CASES`` at their own B x T (N = D of 4 .. 192, K = 3C of 12 .. 1 584, the
identity shortcut at D = C = 20 and 64, C > 256, B = 17, T' = 2), rows 0 and 4 (both with the identity shortcut) at
(B, T) = (1, 4) and (3, 2), the smallest the step takes, and one case at the shipped width D = 768 (C = 128, H = 128, B = 2,
T = 9: N = 768 is six column tiles of the data-gradient GEMM).  Every float64 result is computed once and shared.

A max-pool near-tie reroutes a whole row of ``dx``, so the seeds of the inputs that are new here were checked, on the CPU and
on the restatement alone, and keep the closest pair of res1 at ``POOL_GAP`` = 1e-5 or more (the rows at their own B x T keep
1.2e-5 as they are); tests/test_cnnlstm_input_grad.py asserts it for every case."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cnnlstm_geometry as geo  # noqa: E402
import input_grad_restatement as igr  # noqa: E402

POOL_GAP = 1e-5
WIDE = (768, 128, 128, "silu", 2, 2)                # D, C, H, act, NC, L
# (row of geo.CASES or None for WIDE, B, T, seed or None for the row's own)
DX_CASES = [(i, geo.CASES[i][6], geo.CASES[i][7], None) for i in range(len(geo.CASES))] + [
    (0, 1, 4, 9701), (0, 3, 2, 9702), (4, 1, 4, 9703), (4, 3, 2, 9704), (None, 2, 9, 9705)]
# BatchNorm over exactly two rows in block 2 (B T' = 2) beyond the two (1, 4) cases above: the convolution shortcut with three
# layers, gelu with C > 256 (a second 256-channel block of the two-row kernel), an odd T
PAIR_CASES = [(2, 1, 5, 9711), (6, 1, 4, 9712), (10, 1, 5, 9713)]
MIX_ROWS = (2, 4)
MIX_L = 3
MIX_WEIGHTS = (0.3, -0.2, 0.1)
MIX_SEEDS = {2: 9800, 4: 9810}


def dx_case_id(case):
    i, B, T, seed = case
    return (geo.case_id(i) if i is not None else "wide_d768_c128_h128") + (f"_b{B}_t{T}" if seed is not None else "")


def dims_of(case):
    return geo.CASES[case[0]][:6] if case[0] is not None else WIDE


@functools.lru_cache(maxsize=None)
def setup(case):
    """(state dict, x, labels, masks) of a case."""
    from oracle import cnnlstm_train_oracle as to
    i, B, T, seed = case
    if i is not None:
        return (geo.state_dict(i),) + tuple(geo.train_inputs(i, B, T, seed))
    D, C, H, _, NC, L = WIDE
    x = geo.synth_input(B, T, D, seed + 1)
    labels = np.random.Generator(np.random.PCG64(seed + 2)).integers(0, NC, B)
    return (geo.synth_state_dict(D, C, H, seed, num_classes=NC, layers=L), x, labels,
            to.make_masks(B, T, C, H, geo.P_BLOCK, geo.P_RATE, seed + 3, layers=L))


@functools.lru_cache(maxsize=None)
def restated_case(case):
    sd, x, labels, mk = setup(case)
    return igr.forward_backward(sd, x, labels, dims_of(case)[3], masks=mk)


def restated(i):
    return restated_case(DX_CASES[i])


def model_of(case, train=True):
    """The drop-in module of a case on the device, holding the case's state dict."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM
    if case[0] is not None:
        return geo.model_of(case[0], setup(case)[0], train=train)
    D, C, H, act, NC, L = WIDE
    m = CNNLSTM(input_dim=D, num_classes=NC, cnn_out_channels=C, lstm_hidden_dim=H, lstm_layers=L, dropout_rate=geo.P_RATE,
                activation_fn=act)
    full = m.state_dict()
    for k, v in setup(case)[0].items():
        full[k] = torch.from_numpy(v)
    m.load_state_dict(full)
    m.res_block1.dropout.p = geo.P_BLOCK
    m.res_block2.dropout.p = geo.P_BLOCK
    m = m.to("cuda")
    return m.train() if train else m.eval()


@functools.lru_cache(maxsize=None)
def mix_case(i):
    """One step of a three-layer mix in front of geometry row i: h [B, 3, T, D] float32 from seeds, the row's own state dict,
    labels and masks; ``want``: the restatement at the float64 mix, ``dp64`` = dLoss/dp, ``dw64`` = dLoss/dweights."""
    D, C, H, act, NC, L, B, T = geo.CASES[i]
    sd = geo.state_dict(i)
    _, labels, mk = geo.train_inputs(i)
    h = np.stack([geo.synth_input(B, T, D, MIX_SEEDS[i] + l) for l in range(MIX_L)], axis=1)
    p = igr.softmax64(MIX_WEIGHTS)
    want = igr.forward_backward(sd, igr.layer_mix(h, p), labels, act, masks=mk)
    dp64, _ = igr.layer_mix_dp(h, want["dx"])
    return {"h": h, "labels": labels, "masks": mk, "sd": sd, "p64": p, "want": want, "dp64": dp64,
            "dw64": igr.softmax_jacobian_apply(p, dp64)}
