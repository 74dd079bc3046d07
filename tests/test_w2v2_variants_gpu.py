"""HIP Wav2Vec2 forward variants of the large checkpoints (layer-norm feature encoder, conv bias, stable layer norm,
do_normalize=False) against transformers: committed goldens at the small geometry, and Wav2Vec2Model run on the CPU at
test time at the large stable-layer-norm geometry."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

from robust_speech_analysis_framework_amd import synth
from robust_speech_analysis_framework_amd.w2v2_config import (CONV_BIAS, LAYER_FEAT_NORM, NO_INPUT_NORM, PRE_LN, W2V2Config,
                                                               random_state_dict, save_local_model)

TOL = 1e-4      # north_star: <= 1e-4 relative for float outputs
LARGE = dict(conv_dim=(512,) * 7, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
             intermediate_size=4096, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)
STABLE = LAYER_FEAT_NORM | CONV_BIAS | PRE_LN          # wav2vec2-large-lv60 / XLSR-53 / XLS-R 300M


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _variant(flags, geom, do_normalize=True):
    return W2V2Config(**geom, feat_extract_norm="layer" if flags & LAYER_FEAT_NORM else "group",
                      conv_bias=bool(flags & CONV_BIAS), do_stable_layer_norm=bool(flags & PRE_LN),
                      do_normalize=do_normalize)


def _run(eng, wav_np, spec):
    """spec [(start, length)] -> packed frames of every window (one call), host array."""
    import torch
    T = [eng.cfg.frames(l) for _, l in spec]
    rows = np.concatenate([[0], np.cumsum(T)])
    wav = torch.from_numpy(np.ascontiguousarray(wav_np, dtype=np.float32)).cuda()
    out = torch.full((int(rows[-1]), eng.cfg.hidden_size), float("nan"), dtype=torch.float32, device="cuda")
    eng.forward_windows(wav, [s for s, _ in spec], [l for _, l in spec], out, rows[:-1])
    torch.cuda.synchronize()
    return out.cpu().numpy(), rows


def _hf_reference(cfg, sd, windows):
    """transformers' Wav2Vec2Model on the CPU, one window at a time (the reference loop runs batch 1)."""
    import torch
    from transformers import Wav2Vec2Config, Wav2Vec2FeatureExtractor, Wav2Vec2Model
    torch.set_num_threads(16)
    hc = Wav2Vec2Config(conv_dim=cfg.conv_dim, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        num_conv_pos_embeddings=cfg.num_conv_pos_embeddings,
                        num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups, layer_norm_eps=cfg.layer_norm_eps,
                        feat_extract_norm=cfg.feat_extract_norm, conv_bias=cfg.conv_bias,
                        do_stable_layer_norm=cfg.do_stable_layer_norm)
    m = Wav2Vec2Model(hc)
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"masked_spec_embed"}, res
    m.eval()
    fe = Wav2Vec2FeatureExtractor(do_normalize=cfg.do_normalize)
    outs = []
    for x in windows:
        iv = fe(x, sampling_rate=16000, return_tensors="pt").input_values
        with torch.no_grad():
            outs.append(m(iv).last_hidden_state.numpy()[0])
    return outs


GOLDEN_CASES = [(f, n, True) for f in range(8) for n in (8000, 20000)] + [(STABLE, 20000, False)]


@pytest.mark.parametrize("flags, n, norm", GOLDEN_CASES, ids=[f"f{f}_{n}{'' if m else '_nonorm'}" for f, n, m in GOLDEN_CASES])
def test_small_variants_match_transformers_goldens(rsaf_lib, flags, n, norm):
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    z = np.load(os.path.join(HERE, "golden", "w2v2_variants_small.npz"))
    geom = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(z["cfg"])).items()}
    cfg = _variant(flags, geom, norm)
    assert cfg.flags == flags | (0 if norm else NO_INPUT_NORM)
    eng = W2V2Engine(cfg, random_state_dict(cfg, seed=int(z["seed"])))
    got, _ = _run(eng, synth.synth_clip(50, 2.0)[:n], [(0, n)])
    want = z[f"last_hidden_state_f{cfg.flags}_{n}"]
    assert got.shape == want.shape
    assert _rel(got, want) < TOL


@pytest.fixture(scope="module")
def large_stable():
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = _variant(STABLE, LARGE)
    sd = random_state_dict(cfg, seed=21)
    return cfg, sd, W2V2Engine(cfg, sd)


def test_large_stable_geometry_matches_transformers(rsaf_lib, large_stable):
    """The large stable-layer-norm geometry (512 / 1024 / 24 / 16 / 4096 / 128 / 16): a 5 s window and a 2 s tail in one
    call (fused attention), and a 10 s window (T = 499 > 256: the three-launch attention)."""
    cfg, sd, eng = large_stable
    clip = synth.synth_clip(300, 12.0)
    spec = [(0, 80000), (64000, 32000)]
    got, rows = _run(eng, clip, spec)
    refs = _hf_reference(cfg, sd, [clip[s:s + l] for s, l in spec])
    for k, ref in enumerate(refs):
        w = got[rows[k]:rows[k + 1]]
        assert w.shape == ref.shape and np.isfinite(w).all()
        assert _rel(w, ref) < TOL, (k, _rel(w, ref))
    got10, _ = _run(eng, clip, [(16000, 160000)])
    ref10 = _hf_reference(cfg, sd, [clip[16000:176000]])[0]
    assert got10.shape == ref10.shape == (499, 1024)
    assert _rel(got10, ref10) < TOL


def test_large_stable_ragged_call_returns_the_bits_of_the_per_length_calls(rsaf_lib, large_stable):
    import torch
    cfg, sd, eng = large_stable
    clip = synth.synth_clip(301, 7.0)
    spec = [(0, 80000), (1000, 52000), (64000, 48000), (5, 80000), (30000, 9000), (200, 400)]
    together, rows = _run(eng, clip, spec)
    wav = torch.from_numpy(clip).cuda()
    alone = torch.zeros((int(rows[-1]), cfg.hidden_size), device="cuda")
    for k, (s0, l) in enumerate(spec):
        eng.forward_windows(wav, [s0], [l], alone, [int(rows[k])])
    torch.cuda.synchronize()
    assert np.array_equal(together, alone.cpu().numpy())


def test_ex_with_flags_zero_returns_the_bits_of_the_base_entry_point(rsaf_lib, monkeypatch):
    """rsaf_w2v2_forward_ragged_ex(..., flags = 0, ...) is rsaf_w2v2_forward_ragged at the base geometry."""
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = W2V2Config()
    eng = W2V2Engine(cfg, random_state_dict(cfg, seed=4))
    clip = synth.synth_clip(302, 9.0)
    spec = [(0, 80000), (64000, 80000), (20000, 30000)]
    base, _ = _run(eng, clip, spec)
    lib = _lib.load()
    ex = lib.rsaf_w2v2_forward_ragged_ex
    used = []

    def via_ex(*a):                       # the base signature with flags = 0 inserted after layer_norm_eps
        used.append(1)
        return ex(*a[:13], 0, *a[13:])
    monkeypatch.setattr(lib, "rsaf_w2v2_forward_ragged", via_ex)
    got, _ = _run(eng, clip, spec)
    assert used and np.array_equal(got, base)


def test_dropin_on_a_local_stable_layer_norm_directory(rsaf_lib, tmp_path):
    import pandas as pd
    from robust_speech_analysis_framework_amd import w2v2
    from robust_speech_analysis_framework_amd.w2v2_config import chunk_plan
    geom = dict(conv_dim=(32,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
                intermediate_size=128, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
    cfg = _variant(STABLE, geom)
    sd = random_state_dict(cfg, seed=8)
    mdir = tmp_path / "model"
    save_local_model(str(mdir), cfg, sd)
    (mdir / "preprocessor_config.json").write_text(json.dumps(
        {"do_normalize": True, "feature_size": 1, "padding_value": 0.0, "return_attention_mask": True,
         "sampling_rate": 16000, "feature_extractor_type": "Wav2Vec2FeatureExtractor"}))
    paths = synth.write_synth_corpus(str(tmp_path / "wav"), 1, 11.0, first=70)
    short = tmp_path / "wav" / "short.wav"
    synth.write_wav(str(short), synth.synth_clip_int16(98, 0.3))
    df = pd.DataFrame({"filepath": [str(short), paths[0]]})
    seqs = w2v2.extract_wav2vec2_sequences(df, model_name=str(mdir), verbose=False)
    assert list(seqs) == ["synth_00070.wav"]                                    # the 0.3 s file is absent
    clip = synth.synth_clip(70, 11.0)
    plan = chunk_plan(len(clip))
    refs = _hf_reference(cfg, sd, [clip[s:s + l] for s, l in plan])
    seq = seqs["synth_00070.wav"]
    assert seq.dtype == np.float32 and seq.shape == (sum(r.shape[0] for r in refs), cfg.hidden_size)
    r0 = 0
    for ref in refs:                                                            # every window on its own
        assert _rel(seq[r0:r0 + ref.shape[0]], ref) < TOL
        r0 += ref.shape[0]
    emb = w2v2.extract_wav2vec2_embeddings(df, model_name=str(mdir), verbose=False)
    assert list(emb["filename"]) == ["synth_00070.wav"]
    assert np.allclose(emb.iloc[0, :-1].to_numpy(dtype=np.float64), np.concatenate(refs).mean(axis=0), atol=1e-4)
