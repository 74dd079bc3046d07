"""Geometry table of the CNN-LSTM entry points and the builders of its cases, shared by tests/test_cnnlstm_geometry.py
(no GPU) and tests/test_cnnlstm_geometry_gpu.py.

``check_dims`` (csrc/cnnlstm_host.h over ``dims_problem`` of csrc/cnnlstm_layout.h) accepts every input_dim and cnn_out_channels that is a multiple
of 4, lstm_hidden_dim 64 or 128, 1 to 16 classes and 1 to 4 LSTM layers; the code branches on exactly these dimensions
(fp16-split or exact-fp32 convolutions, panel image of the input, the tile configuration of the GEMM, the 32 / 64 / 256
channel blocks of the training helpers, the ``max(...)`` sizes of the training scratch).  Each row is the smallest shape
that reaches one of those branches.  Everything is drawn from numpy PCG64 streams keyed by the case number."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from weights import synth_input, synth_state_dict  # noqa: E402

P_BLOCK, P_RATE = 0.2, 0.5
GUARD_FLOATS = 4096
GUARD_PATTERN = 0x5A5A5A5A

CASES = [
    # D, C, H, act, NC, L, B, T           what only this case reaches
    (4, 4, 64, "silu", 3, 1, 3, 9),       # smallest widths; fp32 path; identity shortcut; one partial 32 / 64 / 256-channel block
    (20, 20, 64, "gelu", 2, 3, 2, 10),    # width no multiple of 8 or 16; identity shortcut on the fp32 path; three layers
    (16, 48, 64, "silu", 5, 3, 5, 13),    # f16x3 path, ragged 256 x 64 tile (N = 48); C / 8 = 6; K = 144; odd T; B above a 4-row tile
    (64, 16, 128, "gelu", 16, 4, 2, 8),   # panel image at its smallest D (4 tap panels); N = 16; largest NC and L; H = 128
    (64, 64, 64, "silu", 2, 2, 3, 12),    # panel image with the identity shortcut
    (48, 100, 128, "silu", 3, 1, 4, 7),   # D % 16 == 0, C % 16 != 0: fp32 path; C straddles a 64-channel block and a 32-wide tile
    (36, 272, 64, "gelu", 4, 2, 2, 6),    # fp32 path with C > 256 (second 256-channel block, guarded) and C > 2H
    (16, 272, 64, "silu", 2, 2, 3, 7),    # f16x3 convolutions on the 256 x 256 configuration with a 16-column edge tile
    (32, 96, 128, "gelu", 3, 2, 4, 11),   # 512 x 128 configuration with N = 96
    (192, 144, 64, "silu", 2, 2, 2, 9),   # 12 tap panels; 256 x 256 configuration with N = 144
    (100, 20, 128, "silu", 7, 4, 17, 5),  # D >> C on the fp32 path; B above one 16-row tile; T' = 2; four layers
    (16, 528, 64, "silu", 2, 1, 2, 6),    # C > 8H: the C side of every max(...) of the training scratch; three column tiles
]
INFER_SHAPES = [(1, 2), (3, 3), (2, 9), (5, 12)]
NC1 = len(CASES)                          # inference only: geometry 9 with one class
NC1_GEOMETRY, NC1_SEED = 9, 9300


def case_id(i):
    if i == NC1:
        return f"{NC1}_geometry{NC1_GEOMETRY}_nc1"
    D, C, H, act, NC, L, _, _ = CASES[i]
    return f"{i}_d{D}_c{C}_h{H}_{act}_nc{NC}_l{L}"


def geometry(i):
    """(D, C, H, act, NC, L) of case i (``NC1``: the one-class case)."""
    if i == NC1:
        D, C, H, act, _, L = CASES[NC1_GEOMETRY][:6]
        return D, C, H, act, 1, L
    return CASES[i][:6]


def seed_of(i):
    return NC1_SEED if i == NC1 else 9100 + 10 * i


def state_dict(i, seed=None):
    D, C, H, _, NC, L = geometry(i)
    return synth_state_dict(D, C, H, seed_of(i) if seed is None else seed, num_classes=NC, layers=L)


def model_of(i, sd, train=False):
    """The drop-in module of case i on the device, holding ``sd``."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM
    D, C, H, act, NC, L = geometry(i)
    m = CNNLSTM(input_dim=D, num_classes=NC, cnn_out_channels=C, lstm_hidden_dim=H, lstm_layers=L, dropout_rate=P_RATE,
                activation_fn=act)
    full = m.state_dict()
    assert set(sd) <= set(full)
    for k, v in sd.items():
        full[k] = torch.from_numpy(v)
    m.load_state_dict(full)
    m.res_block1.dropout.p = P_BLOCK
    m.res_block2.dropout.p = P_BLOCK
    m = m.to("cuda")
    return m.train() if train else m.eval()


def infer_shapes(i):
    return INFER_SHAPES + ([(17, 6)] if i == 10 else [])


def infer_input(i, k):
    B, T = infer_shapes(i)[k]
    return synth_input(B, T, geometry(i)[0], seed_of(i) + 100 + k)


def train_inputs(i, B=None, T=None, seed=None):
    """(x, labels, masks) of the training step of case i (other B, T, seed: the replicas of the group tests)."""
    from oracle import cnnlstm_train_oracle as to
    D, C, H, _, NC, L, B0, T0 = CASES[i]
    B, T, seed = B0 if B is None else B, T0 if T is None else T, seed_of(i) if seed is None else seed
    x = synth_input(B, T, D, seed + 1)
    labels = np.random.Generator(np.random.PCG64(seed + 2)).integers(0, NC, B)
    return x, labels, to.make_masks(B, T, C, H, P_BLOCK, P_RATE, seed + 3, layers=L)


def train_oracle(i):
    """float64 forward and backward of the training step of case i, with the stage tensors."""
    from oracle import cnnlstm_train_oracle as to
    x, labels, mk = train_inputs(i)
    return to.forward_backward(state_dict(i), x, labels, CASES[i][3], masks=mk, return_stages=True)


def pool_gap(res1):
    """Closest pair of max_pool1d(2) in the oracle's res1 [B, T, C], relative as tests/sweeps/train_fuzz.py measures it."""
    Tp = res1.shape[1] // 2
    pa, pb = res1[:, 0:2 * Tp:2], res1[:, 1:2 * Tp:2]
    return float((np.abs(pa - pb) / np.maximum(np.abs(pa), 1e-3)).min())


def guarded(n_floats, device="cuda"):
    """A float32 buffer of ``n_floats`` + GUARD_FLOATS, every word the pattern."""
    import torch
    return torch.full((int(n_floats) + GUARD_FLOATS,), GUARD_PATTERN, dtype=torch.int32, device=device).view(torch.float32)


def guard_buffers(model, B, T):
    """Replaces the model's cached inference workspace and training scratch by buffers of the size the ABI asks for
    followed by a guard tail (both caches are kept when they are large enough); returns ``check()``, which asserts that
    nothing wrote behind the requested size.  The callee is told the whole length, tail included: what is checked is
    that every write stays inside the layout computed from the dimensions, not the entry's own size check (that one is
    in tests/test_cnnlstm_geometry.py).  ``check.workspace``: the same kind of buffer for a call that takes its own."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    d = model.dims
    sizes = (B, T, d["input_dim"], d["channels"], d["hidden"], d["layers"])
    n_ws, n_scr = int(lib.rsaf_cnnlstm_workspace_bytes(*sizes)), int(lib.rsaf_cnnlstm_train_scratch_floats(*sizes))
    assert n_ws > 0 and n_ws % 4 == 0 and n_scr > 0
    ws, scr, ws2 = guarded(n_ws // 4), guarded(n_scr), guarded(n_ws // 4)
    model._workspace, model._train_scratch = ws, scr

    def check():
        torch.cuda.synchronize()
        assert model._workspace is ws and model._train_scratch is scr, "a cache that was large enough has been replaced"
        for name, buf in (("workspace", ws), ("training scratch", scr), ("workspace of the stages call", ws2)):
            tail = buf.view(torch.int32)[-GUARD_FLOATS:].cpu().numpy()
            bad = np.flatnonzero(tail != GUARD_PATTERN)
            assert bad.size == 0, f"{name}: {bad.size} words written behind the buffer, the first {bad[0]} floats past its end"
    check.workspace = ws2
    return check
