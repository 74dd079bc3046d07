"""tests/w2v2_reference64.py held to transformers: for the four configurations of the conditioning matrix
(tests/test_w2v2_conditioning_gpu.py) the float64 restatement returns every hidden state of transformers' Wav2Vec2Model, built
from the same config and state dict and cast to float64, to 1e-10 of the state's maximum, on a control waveform and on one with
a DC offset.  That makes the restatement a reference, not a second opinion.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import w2v2_reference64 as R                                                                 # noqa: E402

N = R.LENGTHS[1]                      # 33 frames


def _hf_double(cfg, sd):
    """transformers' Wav2Vec2Model of the config with the weights ``sd`` (as _hf_hidden of tests/test_w2v2_families_gpu.py
    builds its models), cast to float64"""
    import torch
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    m = Wav2Vec2Model(Wav2Vec2Config(
        conv_dim=cfg.conv_dim, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
        num_conv_pos_embeddings=cfg.num_conv_pos_embeddings, num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups,
        layer_norm_eps=cfg.layer_norm_eps, feat_extract_norm=cfg.feat_extract_norm, conv_bias=cfg.conv_bias,
        do_stable_layer_norm=cfg.do_stable_layer_norm))
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"masked_spec_embed"}, res
    return m.eval().double()


@pytest.mark.parametrize("kind", ["control", "dc-strong"])
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_float64_restatement_is_transformers_model_in_float64(name, kind):
    import torch
    from transformers import Wav2Vec2FeatureExtractor
    cfg, sd = R.conditioned_weights(name)
    wav = R.waveform(kind, N)
    # the preprocessor's arithmetic is float32; the restatement's window is that formula in float64
    x64 = R.window_input(cfg, wav, torch.float64)
    fe = Wav2Vec2FeatureExtractor(do_normalize=cfg.do_normalize)(wav, sampling_rate=16000, return_tensors="pt").input_values[0]
    assert float((fe.double() - x64).abs().max()) <= 1e-5 * float(x64.abs().max())
    with torch.no_grad():
        want = _hf_double(cfg, sd)(x64[None], output_hidden_states=True)
    got = R.forward64(sd, cfg, wav)
    assert len(got) == len(want.hidden_states) == cfg.num_hidden_layers + 1
    for k, (g, w) in enumerate(zip(got, want.hidden_states)):
        w = w[0].numpy()
        assert g.dtype == w.dtype == np.float64 and g.shape == w.shape == (R.FRAMES[1], cfg.hidden_size)
        e = np.abs(g - w).max() / np.abs(w).max()
        print(f"{name} {kind} hidden_states[{k}]: rel {e:.3e}")
        assert e <= 1e-10, (name, kind, k, e)
    assert torch.equal(want.hidden_states[-1], want.last_hidden_state)


def test_float32_baseline_is_the_same_code_in_float32():
    """dtype = float32 runs the same operations on float32 tensors: float32 results, within float32's reach of the reference
    on the control waveform (a wrong branch taken in one precision only would show as an error of order one)."""
    import torch
    for name in R.CONFIGS:
        cfg, sd = R.conditioned_weights(name)
        wav = R.waveform("control", N)
        h64, h32 = R.forward64(sd, cfg, wav), R.forward64(sd, cfg, wav, dtype=torch.float32)
        assert len(h32) == len(h64)
        for a, b in zip(h32, h64):
            assert a.dtype == np.float32 and a.shape == b.shape
            assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max()


def test_index_order_attention_products_change_nothing_in_float64():
    """chain=True (tests/test_w2v2_long_windows_gpu.py takes its second float32 baseline from it) at T = 257, the first
    window of the three-launch attention: in float64 the index-order products equal torch's own to 1e-12 of each state's
    maximum, and in float32 they stay within float32's reach of the reference."""
    import torch
    T = 257
    cfg, sd = R.conditioned_weights("a-group")
    wav = R.waveform("control", 400 + 320 * (T - 1))
    h64, c64 = R.forward64(sd, cfg, wav), R.forward64(sd, cfg, wav, chain=True)
    c32 = R.forward64(sd, cfg, wav, dtype=torch.float32, chain=True)
    assert len(h64) == len(c64) == len(c32) == cfg.num_hidden_layers + 1
    for a, b, c in zip(h64, c64, c32):
        assert a.shape == b.shape == c.shape == (T, cfg.hidden_size) and b.dtype == np.float64 and c.dtype == np.float32
        assert np.abs(b - a).max() <= 1e-12 * np.abs(a).max()
        assert np.abs(c - a).max() <= 1e-4 * np.abs(a).max()
    assert np.array_equal(h64[0], c64[0])                         # hidden state 0 lies before any attention


def test_hard_kinds_are_hard_and_the_control_is_not():
    """The conditions the GPU matrix asserts before its first launch, here without a GPU: mean^2 / var of conv0's float64
    output, worst channel."""
    cfg_b, sd_b = R.conditioned_weights("b-group-raw")
    cfg_c, sd_c = R.conditioned_weights("c-group-bias")
    for n in R.LENGTHS:
        # 8e2, not 1e3: see DC_STRONG_MIN in tests/test_w2v2_conditioning_gpu.py (slow speech on an offset cannot exceed 900)
        assert R.mean2_over_var(R.conv0_output(sd_b, cfg_b, R.waveform("dc-strong", n))) >= 8e2
        assert R.mean2_over_var(R.conv0_output(sd_b, cfg_b, R.waveform("dc-extreme", n))) >= 1e4
        assert R.mean2_over_var(R.conv0_output(sd_c, cfg_c, R.waveform("control", n))) >= 30
        for name in ("a-group", "b-group-raw"):
            cfg, sd = R.conditioned_weights(name)
            assert R.mean2_over_var(R.conv0_output(sd, cfg, R.waveform("control", n))) <= 1e-2
