"""WavLM and HuBERT checkpoints on the HIP Wav2Vec2 path against transformers: committed goldens at the small geometry (every
hidden state; a forward that ignores WavLM's position bias cannot pass), WavLMModel / HubertModel run on the CPU at test time
at the base and the large stable-layer-norm geometries, the ragged-call bit identity, and the drop-ins on a local WavLM
directory."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

from robust_speech_analysis_framework_amd import synth
from robust_speech_analysis_framework_amd.w2v2_config import (LAYER_FEAT_NORM, NO_FEAT_PROJ_LN, PRE_LN, REL_POS_BIAS, W2V2Config,
                                                               random_state_dict, save_local_model)

TOL = 1e-4      # north_star: <= 1e-4 relative for float outputs
BASE = dict(conv_dim=(512,) * 7, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
            intermediate_size=3072, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)
LARGE = dict(conv_dim=(512,) * 7, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
             intermediate_size=4096, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _run(eng, wav_np, spec, layers=None):
    """spec [(start, length)] -> (packed last_hidden_state, hidden-state planes or None, window row offsets), host arrays."""
    import torch
    T = [eng.cfg.frames(l) for _, l in spec]
    rows = np.concatenate([[0], np.cumsum(T)])
    wav = torch.from_numpy(np.ascontiguousarray(wav_np, dtype=np.float32)).cuda()
    out = torch.full((int(rows[-1]), eng.cfg.hidden_size), float("nan"), dtype=torch.float32, device="cuda")
    r = eng.forward_windows(wav, [s for s, _ in spec], [l for _, l in spec], out, rows[:-1], hidden=layers)
    torch.cuda.synchronize()
    planes = None if layers is None else r[1].cpu().numpy()
    return out.cpu().numpy(), planes, rows


def _hf_model(cfg, sd):
    """transformers' WavLMModel / HubertModel of the config with the weights ``sd``, on the CPU."""
    import torch
    from transformers import HubertConfig, HubertModel, WavLMConfig, WavLMModel
    torch.set_num_threads(16)
    common = dict(conv_dim=cfg.conv_dim, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                  num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                  num_conv_pos_embeddings=cfg.num_conv_pos_embeddings,
                  num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups, layer_norm_eps=cfg.layer_norm_eps,
                  feat_extract_norm=cfg.feat_extract_norm, conv_bias=cfg.conv_bias, do_stable_layer_norm=cfg.do_stable_layer_norm)
    if cfg.model_type == "wavlm":
        m = WavLMModel(WavLMConfig(**common, num_buckets=cfg.num_buckets, max_bucket_distance=cfg.max_bucket_distance))
    else:
        assert cfg.model_type == "hubert"
        m = HubertModel(HubertConfig(**common, feat_proj_layer_norm=cfg.feat_proj_layer_norm))
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"masked_spec_embed"}, res
    return m.eval()


def _hf_hidden(cfg, sd, windows, layers=None):
    """One window at a time (the reference loop runs batch 1): per window [len(layers), T, H]; layers None = all."""
    import torch
    from transformers import Wav2Vec2FeatureExtractor
    m = _hf_model(cfg, sd)
    fe = Wav2Vec2FeatureExtractor(do_normalize=cfg.do_normalize)
    outs = []
    for x in windows:
        iv = fe(x, sampling_rate=16000, return_tensors="pt").input_values
        with torch.no_grad():
            hs = m(iv, output_hidden_states=True).hidden_states
        outs.append(np.stack([hs[k].numpy()[0] for k in (range(len(hs)) if layers is None else layers)]))
    return outs


def _check_states(got, rows, refs, layers):
    worst = 0.0
    for k, ref in enumerate(refs):
        w = got[:, rows[k]:rows[k + 1]]
        assert w.shape == ref.shape and np.isfinite(w).all()
        for j, layer in enumerate(layers):
            e = _rel(w[j], ref[j])
            worst = max(worst, e)
            print(f"window {k} hidden_states[{layer}] rel {e:.3e}")
            assert e < TOL, (k, layer, e)
    return worst


# ---- committed goldens at the small geometry ---------------------------------------------------------------------------
GOLDEN_FLAGS = {"wavlm": REL_POS_BIAS, "wavlm_stable": REL_POS_BIAS | LAYER_FEAT_NORM | PRE_LN,
                "hubert": LAYER_FEAT_NORM | 2 | PRE_LN, "hubert_noln": NO_FEAT_PROJ_LN}


@pytest.mark.parametrize("n", [8000, 20000])
@pytest.mark.parametrize("name", list(GOLDEN_FLAGS))
def test_small_families_match_transformers_goldens(rsaf_lib, name, n):
    """Every hidden state of WavLMModel / HubertModel (tests/golden/make_w2v2_families_golden.py).  head_dim 16: the
    three-launch attention with the bias added in the softmax launch."""
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    z = np.load(os.path.join(HERE, "golden", "w2v2_families_small.npz"))
    geom = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(z["cfg"])).items()}
    cfg = W2V2Config(**geom, **json.loads(str(z["cases"]))[name])
    assert cfg.flags == GOLDEN_FLAGS[name]
    eng = W2V2Engine(cfg, random_state_dict(cfg, seed=int(z["seed"])))
    layers = list(range(cfg.num_hidden_layers + 1))
    out, planes, rows = _run(eng, synth.synth_clip(50, 2.0)[:n], [(0, n)], layers)
    want = z[f"hidden_states_{name}_{n}"]
    _check_states(planes, rows, [want], layers)
    assert np.array_equal(out, planes[-1])
    if cfg.model_type == "wavlm":
        # what a forward without the position bias returns is far from the reference, so the check above sees the bias
        blind = z[f"no_bias_last_hidden_state_{name}_{n}"]
        print(f"reference without the bias: rel {_rel(blind, want[-1]):.3e}; this forward against it: {_rel(out, blind):.3e}")
        assert _rel(blind, want[-1]) > 100 * TOL
        assert _rel(out, blind) > 100 * TOL


# ---- transformers on the CPU at test time ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wavlm_base():
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = W2V2Config(**BASE, model_type="wavlm")
    assert cfg.flags == REL_POS_BIAS and cfg.head_dim == 64
    sd = random_state_dict(cfg, seed=31)
    return cfg, sd, W2V2Engine(cfg, sd)


def test_wavlm_base_geometry_matches_transformers(rsaf_lib, wavlm_base):
    """768 / 12 / 12, head_dim 64: a 5 s window and a 2 s tail in one call (the fused attention kernel's bias instance), then
    a 10 s window (T = 499 > 256: the three-launch attention).  num_buckets 320, max_bucket_distance 800."""
    cfg, sd, eng = wavlm_base
    clip = synth.synth_clip(310, 12.0)
    spec = [(0, 80000), (64000, 32000)]
    layers = [0, 1, 6, 12]
    _, planes, rows = _run(eng, clip, spec, layers)
    _check_states(planes, rows, _hf_hidden(cfg, sd, [clip[s:s + l] for s, l in spec], layers), layers)
    out10, _, _ = _run(eng, clip, [(16000, 160000)])
    ref10 = _hf_hidden(cfg, sd, [clip[16000:176000]], [12])[0][0]
    assert out10.shape == ref10.shape == (499, 768)
    print(f"T = 499 rel {_rel(out10, ref10):.3e}")
    assert _rel(out10, ref10) < TOL
    # the bias is not a rounding matter at this geometry either
    blind = _hf_hidden(cfg, {**sd, "encoder.layers.0.attention.rel_attn_embed.weight":
                             np.zeros_like(sd["encoder.layers.0.attention.rel_attn_embed.weight"])},
                       [clip[16000:176000]], [12])[0][0]
    assert _rel(blind, ref10) > 100 * TOL


def test_wavlm_large_stable_geometry_matches_transformers(rsaf_lib):
    """1024 / 24 / 16 with stable layer norm and the layer-norm feature encoder (wavlm-large's switches): the gates come from
    LN1(h).  A 5 s window and a 2 s tail in one call, then a 10 s window."""
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = W2V2Config(**LARGE, model_type="wavlm", feat_extract_norm="layer", do_stable_layer_norm=True)
    assert cfg.flags == REL_POS_BIAS | LAYER_FEAT_NORM | PRE_LN
    sd = random_state_dict(cfg, seed=32)
    eng = W2V2Engine(cfg, sd)
    clip = synth.synth_clip(311, 12.0)
    spec = [(0, 80000), (64000, 32000)]
    layers = [0, 12, 24]
    _, planes, rows = _run(eng, clip, spec, layers)
    _check_states(planes, rows, _hf_hidden(cfg, sd, [clip[s:s + l] for s, l in spec], layers), layers)
    out10, _, _ = _run(eng, clip, [(16000, 160000)])
    ref10 = _hf_hidden(cfg, sd, [clip[16000:176000]], [24])[0][0]
    assert out10.shape == ref10.shape == (499, 1024)
    print(f"T = 499 rel {_rel(out10, ref10):.3e}")
    assert _rel(out10, ref10) < TOL


def test_hubert_base_geometry_matches_transformers(rsaf_lib):
    """768 / 12 / 12 without the feature-projection LayerNorm (hubert-base's switches)."""
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = W2V2Config(**BASE, model_type="hubert", feat_proj_layer_norm=False)
    assert cfg.flags == NO_FEAT_PROJ_LN
    sd = random_state_dict(cfg, seed=33)
    eng = W2V2Engine(cfg, sd)
    clip = synth.synth_clip(312, 7.0)
    spec = [(0, 80000), (64000, 32000)]
    layers = [0, 6, 12]
    _, planes, rows = _run(eng, clip, spec, layers)
    _check_states(planes, rows, _hf_hidden(cfg, sd, [clip[s:s + l] for s, l in spec], layers), layers)


def test_wavlm_ragged_call_returns_the_bits_of_the_per_length_calls(rsaf_lib, wavlm_base):
    """Windows of at most 249 frames at the base geometry; tests/test_w2v2_long_windows_gpu.py mixes windows either side of
    256 and 512 frames, where the forward changes kernels."""
    import torch
    cfg, sd, eng = wavlm_base
    clip = synth.synth_clip(313, 7.0)
    spec = [(0, 80000), (1000, 52000), (64000, 48000), (5, 80000), (30000, 9000), (200, 400)]    # at most 249 frames
    together, _, rows = _run(eng, clip, spec)
    wav = torch.from_numpy(clip).cuda()
    alone = torch.zeros((int(rows[-1]), cfg.hidden_size), device="cuda")
    for k, (s0, l) in enumerate(spec):
        eng.forward_windows(wav, [s0], [l], alone, [int(rows[k])])
    torch.cuda.synchronize()
    assert np.isfinite(together).all() and np.array_equal(together, alone.cpu().numpy())


def test_bad_flag_combinations_are_refused_before_any_launch(rsaf_lib):
    import ctypes as C
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.w2v2 import _cfg_args
    cfg = W2V2Config(conv_dim=(32,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
                     intermediate_size=128, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
    buf = torch.zeros(1 << 20, device="cuda")
    lens = (C.c_int * 1)(8000)
    dev = torch.zeros(8, dtype=torch.int64, device="cuda")
    for flags in (NO_FEAT_PROJ_LN | LAYER_FEAT_NORM, 16, 128):
        rc = rsaf_lib.rsaf_w2v2_forward_ragged_ex(_lib.ptr(buf), _lib.ptr(dev), _lib.ptr(dev), lens, 1, *_cfg_args(cfg), 1e-5, flags,
                                                  _lib.ptr(buf), _lib.ptr(buf), buf.numel() * 4, _lib.ptr(buf), None, None)
        assert rc != 0, flags
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                                         # nothing ran


# ---- the drop-ins on a local WavLM directory ---------------------------------------------------------------------------
def test_dropins_on_a_local_wavlm_directory(rsaf_lib, tmp_path):
    import pandas as pd
    from robust_speech_analysis_framework_amd import w2v2
    from robust_speech_analysis_framework_amd.w2v2_config import chunk_plan
    cfg = W2V2Config(conv_dim=(32,) * 7, hidden_size=128, num_hidden_layers=8, num_attention_heads=2,
                     intermediate_size=256, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, model_type="wavlm")
    assert cfg.head_dim == 64                                                    # the fused attention kernel
    sd = random_state_dict(cfg, seed=9)
    mdir = tmp_path / "wavlm"
    save_local_model(str(mdir), cfg, sd)
    assert json.loads((mdir / "config.json").read_text())["model_type"] == "wavlm"
    paths = synth.write_synth_corpus(str(tmp_path / "wav"), 1, 11.0, first=71)
    df = pd.DataFrame({"filepath": [paths[0]]})
    clip = synth.synth_clip(71, 11.0)
    plan = chunk_plan(len(clip))
    sel = [0, 6, -1]
    refs = _hf_hidden(cfg, sd, [clip[s:s + l] for s, l in plan], [0, 6, 8])
    want = np.concatenate(refs, axis=1)                                          # [3, sum T, H]
    seq = w2v2.extract_wav2vec2_sequences(df, model_name=str(mdir), verbose=False)["synth_00071.wav"]
    assert seq.dtype == np.float32 and seq.shape == want.shape[1:]
    lay = w2v2.extract_wav2vec2_sequences(df, model_name=str(mdir), verbose=False, output_layers=sel)["synth_00071.wav"]
    assert lay.shape == want.shape and np.array_equal(lay[2], seq)
    r0 = 0
    for ref in refs:                                                             # every window on its own
        T = ref.shape[1]
        assert _rel(seq[r0:r0 + T], ref[2]) < TOL
        for j in range(3):
            assert _rel(lay[j, r0:r0 + T], ref[j]) < TOL, j
        r0 += T
    emb = w2v2.extract_wav2vec2_embeddings(df, model_name=str(mdir), verbose=False)
    assert np.allclose(emb.iloc[0, :-1].to_numpy(dtype=np.float64), want[2].mean(axis=0), atol=1e-4)
    pooled = w2v2.extract_wav2vec2_embeddings(df, model_name=str(mdir), verbose=False, output_layers=sel)
    assert list(pooled.columns[[0, 128, 256]]) == ["l0_dim_0", "l6_dim_0", "l8_dim_0"] and pooled.shape == (1, 3 * 128 + 1)
    got = pooled.iloc[0, :-1].to_numpy(dtype=np.float64).reshape(3, 128)
    assert np.allclose(got, want.mean(axis=1), atol=1e-4)
