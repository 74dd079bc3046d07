"""Wav2Vec2 windows over 256 frames (chunk_seconds = 10, 20, 30 of the drop-ins; forward_windows) against float64, and the
promise of include/rsaf.h that a ragged call returns the values of the per-window calls, across every regime.

The forward picks its kernels from a window's frame count T (csrc/w2v2_layout.h: window_regime), at head width 64 and a
positional group width of 16:
    T <= 256        posconv_f16x3_kernel<NT, 2>, attn_f16x3_kernel (fused)
    257 .. 512      posconv_f16x3_kernel<NT, 1>, three launches: fp32 GEMM, softmax_kernel<false>, fp32 GEMM
    T > 512         posconv_batched_gemm() on the f16x3 GEMM, three launches

Main geometry (that of tests/test_w2v2_attention_gpu.py): conv_dim 32 x 7, hidden 128, 2 heads of width 64, 1 layer,
intermediate 128, 16 positional taps in 8 groups (width 16: the f16x3 positional path), seeded weights.  A window of
400 + 320 (T - 1) samples gives exactly T frames; the windows are cut from synth.synth_clip(328, 22.0)[8000:].
Frames: 255, 256 | 257, 258, 259, 260, 511, 512 | 513, 1023, 1024, 1025: the two regime edges, all four values of T mod 4 on
softmax_kernel<false> (its pad columns T .. Tp - 1 are written by a loop of their own) and the edges of PC_ROWS.  Each regime
runs as ONE ragged call with hidden=[0, L]: hidden state 0 isolates the positional convolution, the last one adds attention
and the feed forward.

(a) per window and state: err = max |got - ref64| / max |ref64| <= max(FACTOR e32, FLOOR), FACTOR and FLOOR those of
    tests/test_w2v2_conditioning_gpu.py (8 and 2e-6, derived there).  e32 is the larger of the two float32 runs of the
    restatement (tests/w2v2_reference64.py): torch's own, and chain=True, the index-order sums an fp32 FMA chain may take.
    The bar comes from the reference alone.  The same figure is asserted as a maximum over the rows, and a failure names
    the row and the channel of the maximum.
(b) widths with no regimes: hidden 64, 4 heads of 16, 8 positional groups of 8, 2 layers (the geometry of
    test_group_width_not_multiple_of_16_matches_oracle), T = 255, 256, 257, 513 in one call under the bar of (a): the
    exact-fp32 grouped convolution per run of equal windows, softmax_kernel<true> at Tp = 256 against <false> at Tp = 260.
(c) position bias: WavLM at the main geometry (num_buckets 32, max_bucket_distance 40), T = 257, 513, 1025 in one call
    against transformers' WavLMModel in float64 under the bar of (a), e32 being the same model in float32.  T = 1025 is the
    smallest window whose distances reach +-1024 = RSAF_W2V2_REL_SPAN, where the kernels clamp the table index.
(d) the batched-GEMM positional convolution alone (RSAF_W2V2_POSCONV_GEMM=1): hidden state 0 at T = 257 and 512 under the
    bar of (a), so that the > 512 path is not the only place that form is held to float64.
(e) the contract of rsaf.h: one forward_windows call over T = 1025, 513, 512, 499, 257, 256, 249, 120, 33, 2 in shuffled
    order with hidden=[0, L] returns the bits of ten calls of one window each, for `out` and both planes; the same for the
    WavLM engine of (c) (1025, 513, 257, 120) and a stable-layer-norm engine (d-layer-bias-stable: 513, 257, 120).  Before
    the ragged entry points ran a call as one sub-call per regime run, every window whose regime differed from the longest
    one's took the longest one's kernels and returned other bits.  A last case repeats a call across three regimes with
    the C ABI's packed output (out_row_start NULL), which forward_windows never asks for.

`python tests/test_w2v2_long_windows_gpu.py` prints the table of every cell of (a) - (d)
(profiles/r28/w2v2_long_windows.txt is one run)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import w2v2_reference64 as R                                                                 # noqa: E402
from robust_speech_analysis_framework_amd import synth                                       # noqa: E402
from robust_speech_analysis_framework_amd.w2v2_config import REL_SPAN, W2V2Config, random_state_dict   # noqa: E402
from test_w2v2_conditioning_gpu import FACTOR, FLOOR                                         # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 28
REGIME_CALLS = ((256, 255), (512, 511, 260, 259, 258, 257), (1025, 1024, 1023, 513))       # one ragged call each
NARROW = dict(conv_dim=(32,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
              num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=8)
NARROW_FRAMES = (513, 257, 256, 255)
WAVLM_FRAMES = (1025, 513, 257)
GEMM_FRAMES = (512, 257)
MIXED = {"main": (1025, 513, 512, 499, 257, 256, 249, 120, 33, 2), "wavlm": (1025, 513, 257, 120), "stable": (513, 257, 120)}

_clip = []


def _speech():
    if not _clip:
        _clip.append(np.ascontiguousarray(synth.synth_clip(328, 22.0)[8000:], dtype=np.float32))
    return _clip[0]


def _spec(frames):
    return [(37 * i, 400 + 320 * (T - 1)) for i, T in enumerate(frames)]


def _config(kind):
    """(config, state dict, whether the restatement's chain=True run is a second float32 baseline)"""
    if kind == "main":
        cfg = W2V2Config(**R.GEOM)
        assert cfg.head_dim == 64 and cfg.hidden_size // cfg.num_conv_pos_embedding_groups == 16
        return cfg, random_state_dict(cfg, SEED), True
    if kind == "narrow":
        cfg = W2V2Config(**NARROW)
        assert cfg.head_dim == 16 and cfg.hidden_size // cfg.num_conv_pos_embedding_groups == 8
        return cfg, random_state_dict(cfg, SEED + 1), True
    if kind == "wavlm":
        cfg = W2V2Config(**R.GEOM, model_type="wavlm", num_buckets=32, max_bucket_distance=40)
        assert cfg.head_dim == 64
        return cfg, random_state_dict(cfg, SEED + 2), False
    assert kind == "stable"
    cfg, sd = R.conditioned_weights("d-layer-bias-stable")
    assert cfg.do_stable_layer_norm and cfg.head_dim == 64
    return cfg, sd, False


_engines = {}


def _engine(kind):
    if kind not in _engines:
        from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
        cfg, sd, chain = _config(kind)
        _engines[kind] = (cfg, sd, chain, W2V2Engine(cfg, sd))
    return _engines[kind]


def _forward(eng, spec, order=None):
    """one forward_windows call with hidden=[0, L] over the windows of `spec`, given in `order` -> (out, planes [2, rows, hidden]);
    window k of `spec` owns rows rows[k] .. rows[k + 1] whatever the order"""
    import torch
    cfg = eng.cfg
    T = [cfg.frames(l) for _, l in spec]
    rows = np.concatenate([[0], np.cumsum(T)])
    order = list(range(len(spec))) if order is None else list(order)
    wav = torch.from_numpy(_speech()).cuda()
    out = torch.full((int(rows[-1]), cfg.hidden_size), float("nan"), dtype=torch.float32, device="cuda")
    _, planes = eng.forward_windows(wav, [spec[k][0] for k in order], [spec[k][1] for k in order], out, [int(rows[k]) for k in order],
                                    hidden=[0, cfg.num_hidden_layers])
    torch.cuda.synchronize()
    return out.cpu().numpy(), planes.cpu().numpy(), rows


def _references(kind, cfg, sd, chain, wav):
    """(ref64, [float32 baselines]) of one window, each the pair of hidden states (0, L)"""
    import torch
    L = cfg.num_hidden_layers
    if kind == "wavlm":
        runs = [R.wavlm64(sd, cfg, wav), R.wavlm64(sd, cfg, wav, dtype=torch.float32)]
    else:
        runs = [R.forward64(sd, cfg, wav), R.forward64(sd, cfg, wav, dtype=torch.float32)]
        if chain:
            runs.append(R.forward64(sd, cfg, wav, dtype=torch.float32, chain=True))
    pairs = [[h[0], h[L]] for h in runs]
    for pair in pairs:
        for a in pair:
            a.setflags(write=False)
    assert pairs[0][0].dtype == np.float64 and all(p[0].dtype == np.float32 for p in pairs[1:])
    return pairs[0], pairs[1:]


class Call:
    """One ragged call of an engine over the windows of `frames` (longest first), its two hidden states, and per window
    the float64 reference and the float32 baselines (computed once, never changed)."""

    def __init__(self, kind, frames, refs=None):
        self.kind, self.frames = kind, tuple(frames)
        self.cfg, self.sd, self.chain, self.eng = _engine(kind)
        self.spec = _spec(frames)
        clip = _speech()
        assert [self.cfg.frames(l) for _, l in self.spec] == list(frames) and max(s + l for s, l in self.spec) <= len(clip)
        self.refs = refs or [_references(kind, self.cfg, self.sd, self.chain, clip[s:s + l]) for s, l in self.spec]
        self.out, self.got, self.rows = _forward(self.eng, self.spec)

    def cells(self, states=(0, 1)):
        """[(T, state, err, row, channel, row figure, [e32 per baseline], bar)] of the call's windows"""
        out = []
        L = self.cfg.num_hidden_layers
        for k, T in enumerate(self.frames):
            ref64, base = self.refs[k]
            for j in states:
                got, ref = self.got[j, self.rows[k]:self.rows[k + 1]], ref64[j]
                assert got.shape == ref.shape == (T, self.cfg.hidden_size)
                assert np.isfinite(got).all(), (self.kind, T, j)
                den = np.abs(ref).max()
                d = np.abs(got - ref)
                per_row = d.max(axis=1) / den
                row = int(per_row.argmax())
                e32 = [float(np.abs(b[j] - ref).max() / den) for b in base]
                out.append((T, (0, L)[j], float(d.max() / den), row, int(d[row].argmax()), float(per_row[row]), e32,
                            max(FACTOR * max(e32), FLOOR)))
        return out


_calls = {}


def _call(kind, frames):
    key = (kind, tuple(frames))
    if key not in _calls:
        _calls[key] = Call(kind, frames)
    return _calls[key]


def _print(label, cells):
    for T, state, err, row, ch, _, e32, bar in cells:
        print(f"{label:8s} T {T:4d} hidden[{state}]  err {err:.3e} (row {row:4d}, channel {ch:3d})  e32 torch {e32[0]:.3e}  "
              f"chain {(f'{e32[1]:.3e}' if len(e32) > 1 else '-'):>9s}  bar {bar:.3e}  {'ok' if err <= bar else 'ABOVE'}")


def _assert_under_the_bar(label, cells, only=None):
    cells = [c for c in cells if only is None or c[0] == only]
    _print(label, cells)
    seen = 0
    for T, state, err, row, ch, row_err, e32, bar in cells:
        seen += 1
        assert row_err == err, (label, T, state, row_err, err)           # the per-row maximum is the same number
        assert err <= bar, (f"{label} T = {T} hidden_states[{state}]: err {err:.3e} above the bar {bar:.3e} (e32 {e32}); the maximum "
                            f"sits at row {row} of {T}, channel {ch}")
    assert seen


def _regime_call_of(T):
    return next(f for f in REGIME_CALLS if T in f)


# ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [T for f in REGIME_CALLS for T in sorted(f)])
def test_every_regime_stays_within_8x_float32_of_float64(rsaf_lib, T):
    c = _call("main", _regime_call_of(T))
    assert np.array_equal(c.out, c.got[1])                                # the call's output is its last hidden state
    _assert_under_the_bar("main", c.cells(), only=T)


# ---- (b) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", sorted(NARROW_FRAMES))
def test_widths_with_no_regimes_stay_under_the_same_bar(rsaf_lib, T):
    c = _call("narrow", NARROW_FRAMES)
    assert np.array_equal(c.out, c.got[1])
    _assert_under_the_bar("narrow", c.cells(), only=T)


# ---- (c) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", sorted(WAVLM_FRAMES))
def test_position_bias_stays_under_the_bar_up_to_the_clamped_distances(rsaf_lib, T):
    cfg = _config("wavlm")[0]
    assert cfg.max_bucket_distance < REL_SPAN <= max(WAVLM_FRAMES) - 1    # the clamp executes, and is exact (rsaf.h)
    c = _call("wavlm", WAVLM_FRAMES)
    assert np.array_equal(c.out, c.got[1])
    _assert_under_the_bar("wavlm", c.cells(), only=T)


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def test_batched_gemm_positional_convolution_alone(rsaf_lib, monkeypatch):
    ref = _call("main", GEMM_FRAMES)                                      # its references; its launch took the LDS kernel
    monkeypatch.setenv("RSAF_W2V2_POSCONV_GEMM", "1")
    c = Call("main", GEMM_FRAMES, refs=ref.refs)
    monkeypatch.delenv("RSAF_W2V2_POSCONV_GEMM", raising=False)
    assert not np.array_equal(c.got[0], ref.got[0])                       # another summation order: the switch was read
    _assert_under_the_bar("gemm", c.cells(states=(0,)))


# ---- (e) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(MIXED))
def test_call_across_regimes_returns_the_bits_of_one_call_per_window(rsaf_lib, kind):
    cfg, _, _, eng = _engine(kind)
    frames = MIXED[kind]
    spec = _spec(frames)
    assert [cfg.frames(l) for _, l in spec] == list(frames)
    order = np.random.Generator(np.random.PCG64(SEED)).permutation(len(spec))
    assert list(order) != sorted(order)
    out, planes, rows = _forward(eng, spec, order)
    assert np.isfinite(out).all() and np.isfinite(planes).all() and np.array_equal(out, planes[1])
    differ = []
    for k, T in enumerate(frames):
        o1, p1, _ = _forward(eng, [spec[k]])
        assert o1.shape == (T, cfg.hidden_size) and np.isfinite(p1).all()
        sl = slice(int(rows[k]), int(rows[k + 1]))
        for name, a, b in (("out", out[sl], o1), ("hidden[0]", planes[0, sl], p1[0]), ("hidden[L]", planes[1, sl], p1[1])):
            if not np.array_equal(a, b):
                differ.append((T, name, float(np.abs(a - b).max() / np.abs(b).max())))
    assert not differ, f"{kind}: windows whose bits depend on the call they share (T, tensor, max |d| / max |alone|): {differ}"


def test_packed_output_across_regimes_lands_window_after_window(rsaf_lib):
    """out_row_start NULL (the C ABI's packed layout, which forward_windows never asks for): the sub-calls of a call that spans
    regimes advance `out` and the hidden-state planes by the rows already written.  Same bits as the call with row starts."""
    import ctypes as C
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.w2v2 import _cfg_args
    cfg, _, _, eng = _engine("main")
    frames = (513, 257, 256, 33)                                          # three regimes, longest first
    spec = _spec(frames)
    want_out, want_planes, rows = _forward(eng, spec)
    n, L = len(spec), cfg.num_hidden_layers
    wav = torch.from_numpy(_speech()).cuda()
    starts = torch.tensor([s for s, _ in spec], dtype=torch.int64, device="cuda")
    lens = torch.tensor([l for _, l in spec], dtype=torch.int32, device="cuda")
    lens_c = (C.c_int * n)(*[l for _, l in spec])
    hidden_c = (C.c_int * 2)(0, L)
    ws = eng._workspace(lens_c, n)
    out = torch.full((int(rows[-1]), cfg.hidden_size), float("nan"), dtype=torch.float32, device="cuda")
    planes = torch.full((2,) + tuple(out.shape), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(rsaf_lib.rsaf_w2v2_forward_ragged_hidden(
        _lib.ptr(wav), _lib.ptr(starts), _lib.ptr(lens), lens_c, n, *_cfg_args(cfg), float(cfg.layer_norm_eps), cfg.flags,
        _lib.ptr(eng.blob), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(out), None, hidden_c, 2, _lib.ptr(planes),
        out.shape[0] * cfg.hidden_size, _lib.stream_ptr(None)), "rsaf_w2v2_forward_ragged_hidden")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(planes.cpu().numpy(), want_planes)


if __name__ == "__main__":          # the table of every cell of (a) - (d), as the library in the tree gives it
    print("err = max |got - ref64| / max |ref64| per window and hidden state; e32: the float32 baselines' (torch's own products, "
          f"index-order chain); bar = max({FACTOR:g} max e32, {FLOOR:g})")
    tables = [("main", _call("main", f).cells()) for f in REGIME_CALLS]
    tables.append(("narrow", _call("narrow", NARROW_FRAMES).cells()))
    tables.append(("wavlm", _call("wavlm", WAVLM_FRAMES).cells()))
    os.environ["RSAF_W2V2_POSCONV_GEMM"] = "1"
    tables.append(("gemm", Call("main", GEMM_FRAMES).cells(states=(0,))))
    del os.environ["RSAF_W2V2_POSCONV_GEMM"]
    above = 0
    for label, cells in tables:
        _print(label, cells)
        above += sum(c[2] > c[-1] for c in cells)
    print(f"cells above the bar: {above}")
    # the outlier that tests/test_w2v2_attention_gpu.py carries in PARENT_ERR at T = 255: its own window, on this library
    import test_w2v2_attention_gpu as A
    t255 = next(c for c in tables[0][1] if c[0] == 255 and c[1] == 1)
    print(f"T = 255, last hidden state, fused kernel: err {t255[2]:.3e} here (seed {SEED}, bar {t255[-1]:.3e}); on the window of "
          f"tests/test_w2v2_attention_gpu.py (seed {A.SEED}) this library gives {A._case(1.0).errors()[255]:.3e}, where PARENT_ERR "
          f"records {A.PARENT_ERR[1.0][255]:.3e} for the kernel before the base-2 softmax")
