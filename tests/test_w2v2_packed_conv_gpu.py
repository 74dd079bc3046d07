"""Feature-encoder convolutions with the windows of a group packed along M (csrc/w2v2.hip: packed_in_rows; the row table of
csrc/gemm_f16x3.hip): window boundaries inside a GEMM tile, the junk row between two windows, more windows than one group."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import w2v2_oracle as wo
from robust_speech_analysis_framework_amd import synth
from robust_speech_analysis_framework_amd.w2v2_config import W2V2Config, random_state_dict

TOL = 1e-4      # the bound of tests/test_w2v2_gpu.py for these geometries

KERN = (10, 3, 3, 3, 3, 2, 2)
STRD = (5, 2, 2, 2, 2, 2, 2)

# One ragged call, non-increasing lengths.  Frames per layer (chunk_lengths' recurrence, checked in _check_lengths):
#   20520 -> 4103 2051 1025 512 255 127 63    first window: its 512 rows of conv3 end on a 256-row tile boundary (the junk row
#                                             opens the next tile) and its 255 + 1 rows of conv4 fill one tile exactly
#    9000 -> 1799  899  449 224 111  55 27
#    5123 -> 1023  511  255 127  63  31 15
#    1234 ->  245  122   60  29  14   7  3
#     801 ->  159   79   39  19   9   4  2
#     400 ->   79   39   19   9   4   2  1    five of them: a tile of every layer holds rows of three and more windows, and
#                                             the last window of the call is one frame long
LENS = (20520, 9000, 5123, 1234, 801, 400, 400, 400, 400, 400)
STARTS = (11, 3000, 12000, 700, 25000, 0, 401, 9999, 31000, 31600)


def _frames(n):
    T = []
    for k, s in zip(KERN, STRD):
        n = (n - k) // s + 1 if n >= k else 0
        T.append(n)
    return T


def _check_lengths():
    Ts = [_frames(n) for n in LENS]
    assert all(a >= b for a, b in zip(LENS, LENS[1:])) and Ts[-1][6] == 1 and all(T[6] >= 1 for T in Ts)
    seen = {(KERN[i], T[i - 1] - 2 * T[i]) for T in Ts for i in range(1, 7)}
    assert seen == {(3, 1), (3, 2), (2, 0), (2, 1)}, seen            # every way a window fills its 2 (T_i + 1) input rows
    assert Ts[0][3] % 256 == 0 and (Ts[0][4] + 1) % 256 == 0         # rows / rows + junk row ending on a tile boundary
    for i in range(1, 7):                                            # a 256-row tile with rows of >= 3 windows, every layer
        off = np.concatenate([[0], np.cumsum([T[i] + 1 for T in Ts])])
        tiles = {o // 256 for o in off[:-1]}
        assert max(sum(1 for o in off[:-1] if o // 256 == t) for t in tiles) >= 3


def _cfg(conv_dim):
    return W2V2Config(conv_dim=(conv_dim,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                      num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)


@functools.lru_cache(maxsize=None)
def _case(conv_dim):
    """(cfg, weights, clip, oracle frames per window): computed once per geometry, read-only afterwards."""
    cfg = _cfg(conv_dim)
    sd = random_state_dict(cfg, seed=5)
    clip = synth.synth_clip(310, 2.1)
    assert len(clip) >= max(s + l for s, l in zip(STARTS, LENS))
    refs = tuple(wo.forward(sd, cfg, wo.hf_normalize(clip[s:s + l])[None])[0] for s, l in zip(STARTS, LENS))
    return cfg, sd, clip, refs


def _rows(cfg, lens):
    return np.concatenate([[0], np.cumsum([cfg.frames(l) for l in lens])])


def _run(eng, wav, starts, lens, rows):
    import torch
    out = torch.full((int(rows[-1]), eng.cfg.hidden_size), float("nan"), dtype=torch.float32, device="cuda")
    eng.forward_windows(wav, list(starts), list(lens), out, rows[:-1])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("conv_dim", [32, 512])      # 512: the 256 x 256 tile of the GEMM; 32: its 256 x 64 tile
def test_boundary_lengths_in_one_ragged_call_match_the_oracle_and_the_per_length_bits(rsaf_lib, conv_dim):
    import torch
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    _check_lengths()
    cfg, sd, clip, refs = _case(conv_dim)
    eng = W2V2Engine(cfg, sd)
    wav = torch.from_numpy(clip).cuda()
    rows = _rows(cfg, LENS)
    together = _run(eng, wav, STARTS, LENS, rows)
    host = together.cpu().numpy()
    for w, ref in enumerate(refs):
        got = host[rows[w]:rows[w + 1]]
        assert got.shape == ref.shape
        rel = np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)
        print(f"C = {conv_dim}, window {w} ({LENS[w]} samples): {rel:.3e}")
        assert rel < TOL, (w, rel)
    alone = torch.full_like(together, float("nan"))
    for w, (s0, l) in enumerate(zip(STARTS, LENS)):
        eng.forward_windows(wav, [s0], [l], alone, [int(rows[w])])
    torch.cuda.synchronize()
    assert torch.equal(together, alone)


def test_more_windows_than_one_group_return_the_bits_of_every_window_alone(rsaf_lib):
    """513 windows, one above the 512 of a feature-encoder group, of two short lengths."""
    import torch
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = _cfg(32)
    eng = W2V2Engine(cfg, random_state_dict(cfg, seed=5), max_chunks_per_call=1024)
    clip = synth.synth_clip(311, 2.0)
    wav = torch.from_numpy(clip).cuda()
    n = 513
    lens = [800] * 200 + [400] * (n - 200)
    starts = [(97 * k) % (len(clip) - 800) for k in range(n)]
    rows = _rows(cfg, lens)
    together = _run(eng, wav, starts, lens, rows)
    assert torch.isfinite(together).all()
    alone = torch.full_like(together, float("nan"))
    for w in range(n):
        eng.forward_windows(wav, [starts[w]], [lens[w]], alone, [int(rows[w])])
    torch.cuda.synchronize()
    assert torch.equal(together, alone)


@pytest.mark.parametrize("conv_dim", [32, 512])
def test_junk_rows_and_gap_rows_never_reach_the_output(rsaf_lib, conv_dim):
    """The same call over a workspace of 0xFF bytes (every fp16 pattern a NaN) and over a zeroed one."""
    import torch
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = _cfg(conv_dim)
    eng = W2V2Engine(cfg, random_state_dict(cfg, seed=5))
    clip = synth.synth_clip(310, 2.1)
    wav = torch.from_numpy(clip).cuda()
    rows = _rows(cfg, LENS)
    _run(eng, wav, STARTS, LENS, rows)                   # sizes the workspace
    ws = eng._ws
    ws.view(torch.uint8).fill_(0xFF)
    over_nan = _run(eng, wav, STARTS, LENS, rows)
    assert eng._ws is ws
    ws.zero_()
    over_zero = _run(eng, wav, STARTS, LENS, rows)
    assert eng._ws is ws
    assert torch.isfinite(over_nan).all()
    assert torch.equal(over_nan, over_zero)
