"""Wav2Vec2 hidden states on the HIP path (transformers' ``output_hidden_states=True``) against transformers: committed
goldens at the small geometry for all 8 switch combinations, Wav2Vec2Model run on the CPU at test time at the base and
the large stable-layer-norm geometries, bit identities of the taps, the drop-ins' ``output_layers`` and the device
segment mean."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

from robust_speech_analysis_framework_amd import synth
from robust_speech_analysis_framework_amd.w2v2_config import (CONV_BIAS, LAYER_FEAT_NORM, PRE_LN, W2V2Config, random_state_dict,
                                                               save_local_model)

TOL = 1e-4      # north_star: <= 1e-4 relative for float outputs
SMALL = dict(conv_dim=(32,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
             intermediate_size=128, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
LARGE = dict(conv_dim=(512,) * 7, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
             intermediate_size=4096, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)
STABLE = LAYER_FEAT_NORM | CONV_BIAS | PRE_LN


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _variant(flags, geom):
    return W2V2Config(**geom, feat_extract_norm="layer" if flags & LAYER_FEAT_NORM else "group",
                      conv_bias=bool(flags & CONV_BIAS), do_stable_layer_norm=bool(flags & PRE_LN))


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


def _hf_hidden(cfg, sd, windows, layers):
    """transformers' Wav2Vec2Model on the CPU, one window at a time: per window [len(layers), T, H]."""
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
            hs = m(iv, output_hidden_states=True).hidden_states
        outs.append(np.stack([hs[k].numpy()[0] for k in layers]))
    return outs


def _check_states(got, rows, refs, layers):
    for k, ref in enumerate(refs):
        w = got[:, rows[k]:rows[k + 1]]
        assert w.shape == ref.shape and np.isfinite(w).all()
        for j, layer in enumerate(layers):
            assert _rel(w[j], ref[j]) < TOL, (k, layer, _rel(w[j], ref[j]))


GOLDEN_CASES = [(f, n) for f in range(8) for n in (8000, 20000)]


@pytest.mark.parametrize("flags, n", GOLDEN_CASES, ids=[f"f{f}_{n}" for f, n in GOLDEN_CASES])
def test_small_hidden_states_match_transformers_goldens(rsaf_lib, flags, n):
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    z = np.load(os.path.join(HERE, "golden", "w2v2_hidden_states_small.npz"))
    geom = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(z["cfg"])).items()}
    cfg = _variant(flags, geom)
    eng = W2V2Engine(cfg, random_state_dict(cfg, seed=int(z["seed"])))
    layers = list(range(cfg.num_hidden_layers + 1))
    out, got, rows = _run(eng, synth.synth_clip(50, 2.0)[:n], [(0, n)], layers)
    want = z[f"hidden_states_f{flags}_{n}"]
    assert got.shape == want.shape
    for k in layers:
        assert _rel(got[k], want[k]) < TOL, (k, _rel(got[k], want[k]))
    assert np.array_equal(got[-1], out)                                    # hidden_states[L] is `out`, bit for bit


def test_base_geometry_all_hidden_states_match_transformers(rsaf_lib):
    """All 13 states of the base geometry: a 5 s window and a 2 s tail in one call (fused attention), and a 10 s window
    (T = 499: the three-launch attention)."""
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = W2V2Config()
    sd = random_state_dict(cfg, seed=5)
    eng = W2V2Engine(cfg, sd)
    layers = list(range(13))
    clip = synth.synth_clip(310, 12.0)
    spec = [(0, 80000), (64000, 32000)]
    out, got, rows = _run(eng, clip, spec, layers)
    _check_states(got, rows, _hf_hidden(cfg, sd, [clip[s:s + l] for s, l in spec], layers), layers)
    assert np.array_equal(got[12], out)
    out10, got10, rows10 = _run(eng, clip, [(16000, 160000)], layers)
    assert got10.shape == (13, 499, 768)
    _check_states(got10, rows10, _hf_hidden(cfg, sd, [clip[16000:176000]], layers), layers)
    assert np.array_equal(got10[12], out10)


@pytest.fixture(scope="module")
def large_stable():
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = _variant(STABLE, LARGE)
    sd = random_state_dict(cfg, seed=21)
    return cfg, sd, W2V2Engine(cfg, sd)


def test_large_stable_hidden_states_match_transformers(rsaf_lib, large_stable):
    cfg, sd, eng = large_stable
    layers = [0, 1, 12, 23, 24]
    clip = synth.synth_clip(311, 12.0)
    spec = [(0, 80000), (64000, 32000)]
    out, got, rows = _run(eng, clip, spec, layers)
    _check_states(got, rows, _hf_hidden(cfg, sd, [clip[s:s + l] for s, l in spec], layers), layers)
    assert np.array_equal(got[-1], out)
    _, got10, rows10 = _run(eng, clip, [(16000, 160000)], layers)
    _check_states(got10, rows10, _hf_hidden(cfg, sd, [clip[16000:176000]], layers), layers)


@pytest.mark.parametrize("which", ["base", "large_stable"])
def test_ragged_taps_return_the_bits_of_the_per_window_taps(rsaf_lib, large_stable, which):
    import torch
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    if which == "base":
        cfg = W2V2Config()
        eng = W2V2Engine(cfg, random_state_dict(cfg, seed=6))
        layers = [0, 3, 11, 12]
    else:
        cfg, _, eng = large_stable
        layers = [0, 5, 23, 24]
    clip = synth.synth_clip(312, 7.0)
    spec = [(0, 80000), (1000, 52000), (64000, 48000), (30000, 9000), (200, 400)]
    _, together, rows = _run(eng, clip, spec, layers)
    wav = torch.from_numpy(clip).cuda()
    out = torch.zeros((int(rows[-1]), cfg.hidden_size), device="cuda")
    alone = np.zeros_like(together)
    for k, (s0, l) in enumerate(spec):
        _, planes = eng.forward_windows(wav, [s0], [l], out, [int(rows[k])], hidden=layers)
        alone[:, rows[k]:rows[k + 1]] = planes[:, rows[k]:rows[k + 1]].cpu().numpy()
    assert np.array_equal(together, alone)


def test_n_hidden_zero_returns_the_bits_of_the_ex_entry_point(rsaf_lib, monkeypatch):
    """rsaf_w2v2_forward_ragged_hidden(..., n_hidden = 0, ...) is rsaf_w2v2_forward_ragged_ex (here at the base geometry)."""
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = W2V2Config()
    eng = W2V2Engine(cfg, random_state_dict(cfg, seed=4))
    clip = synth.synth_clip(302, 9.0)
    spec = [(0, 80000), (64000, 80000), (20000, 30000)]
    base, _, _ = _run(eng, clip, spec)
    lib = _lib.load()
    hid = lib.rsaf_w2v2_forward_ragged_hidden
    used = []

    def via_hidden(*a):                   # the base signature with flags = 0 and an empty tap list
        used.append(1)
        return hid(*a[:13], 0, *a[13:18], None, 0, None, 0, a[18])
    monkeypatch.setattr(lib, "rsaf_w2v2_forward_ragged", via_hidden)
    got, _, _ = _run(eng, clip, spec)
    assert used and np.array_equal(got, base)


def test_segment_mean_matches_float64_numpy(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    rng = np.random.default_rng(3)
    planes, rows, width = 3, 1000, 300
    x = (rng.standard_normal((planes, rows, width)) * 3 + 1).astype(np.float32)
    seg = np.array([0, 1, 9, 9, 517, 1000], dtype=np.int64)                 # includes an empty segment
    xd, sd = torch.from_numpy(x).cuda(), torch.from_numpy(seg).cuda()
    out = torch.empty((planes, len(seg) - 1, width), device="cuda")
    _lib.check(_lib.load().rsaf_rows_segment_mean_f32(_lib.ptr(xd), width, rows * width, planes, _lib.ptr(sd), len(seg) - 1,
                                                      width, _lib.ptr(out), _lib.stream_ptr()))
    got = out.cpu().numpy()
    for p in range(planes):
        for s in range(len(seg) - 1):
            a, b = seg[s], seg[s + 1]
            if a == b:
                assert np.isnan(got[p, s]).all()
            else:
                want = x[p, a:b].astype(np.float64).mean(axis=0)
                assert np.abs(got[p, s] - want).max() <= 1e-6 * np.abs(want).max()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("hs")
    cfg = _variant(STABLE, SMALL)
    sd = random_state_dict(cfg, seed=8)
    mdir = d / "model"
    save_local_model(str(mdir), cfg, sd)
    paths = synth.write_synth_corpus(str(d / "wav"), 2, 11.0, first=70)
    short = d / "wav" / "short.wav"
    synth.write_wav(str(short), synth.synth_clip_int16(98, 0.3))
    return cfg, sd, str(mdir), [str(short)] + list(paths)


def test_dropin_sequences_of_layers_on_a_local_stable_layer_norm_directory(rsaf_lib, corpus):
    import pandas as pd
    from robust_speech_analysis_framework_amd import w2v2
    from robust_speech_analysis_framework_amd.w2v2_config import chunk_plan
    cfg, sd, mdir, paths = corpus
    df = pd.DataFrame({"filepath": paths})
    seqs = w2v2.extract_wav2vec2_sequences(df, model_name=mdir, verbose=False, output_layers=[2, 0, 1])
    assert list(seqs) == ["synth_00070.wav", "synth_00071.wav"]               # the 0.3 s file is absent
    for i, fn in enumerate(seqs):
        clip = synth.synth_clip(70 + i, 11.0)
        plan = chunk_plan(len(clip))
        refs = _hf_hidden(cfg, sd, [clip[s:s + l] for s, l in plan], [2, 0, 1])
        seq = seqs[fn]
        assert seq.dtype == np.float32 and seq.shape == (3, sum(r.shape[1] for r in refs), cfg.hidden_size)
        r0 = 0
        for ref in refs:                                                        # every window on its own
            for j in range(3):
                assert _rel(seq[j, r0:r0 + ref.shape[1]], ref[j]) < TOL
            r0 += ref.shape[1]
    # an int gives [T, H]; -1 is last_hidden_state, bit for bit
    last = w2v2.extract_wav2vec2_sequences(df, model_name=mdir, verbose=False, output_layers=-1)
    default = w2v2.extract_wav2vec2_sequences(df, model_name=mdir, verbose=False)
    assert list(last) == list(default)
    for fn in default:
        assert last[fn].shape == default[fn].shape and np.array_equal(last[fn], default[fn])
    one = w2v2.extract_wav2vec2_sequences(df, model_name=mdir, verbose=False, output_layers=1)
    for fn in default:
        assert np.array_equal(one[fn], seqs[fn][2])
    with pytest.raises(ValueError):
        w2v2.extract_wav2vec2_sequences(df, model_name=mdir, verbose=False, output_layers=[0, 3])


def test_dropin_pooled_layers_on_a_local_stable_layer_norm_directory(rsaf_lib, corpus):
    import pandas as pd
    from robust_speech_analysis_framework_amd import w2v2
    from robust_speech_analysis_framework_amd.w2v2_config import chunk_plan
    cfg, sd, mdir, paths = corpus
    df = pd.DataFrame({"filepath": paths})
    emb = w2v2.extract_wav2vec2_embeddings(df, model_name=mdir, verbose=False, output_layers=[0, 1, 2])
    H = cfg.hidden_size
    assert list(emb.columns) == [f"l{l}_dim_{k}" for l in range(3) for k in range(H)] + ["filename"]
    assert list(emb["filename"]) == ["synth_00070.wav", "synth_00071.wav"]
    seqs = w2v2.extract_wav2vec2_sequences(df, model_name=mdir, verbose=False, output_layers=[0, 1, 2])
    for i, fn in enumerate(emb["filename"]):
        got = emb.iloc[i, :-1].to_numpy(dtype=np.float64).reshape(3, H)
        clip = synth.synth_clip(70 + i, 11.0)
        refs = _hf_hidden(cfg, sd, [clip[s:s + l] for s, l in chunk_plan(len(clip))], [0, 1, 2])
        want = np.concatenate(refs, axis=1).mean(axis=1)
        for j in range(3):
            assert _rel(got[j], want[j]) < TOL
        exact = seqs[fn].astype(np.float64).mean(axis=1)                       # the device pool vs float64 numpy
        assert np.abs(got - exact).max() <= 1e-6 * np.abs(exact).max()
    single = w2v2.extract_wav2vec2_embeddings(df, model_name=mdir, verbose=False, output_layers=-2)
    assert list(single.columns) == [f"dim_{k}" for k in range(H)] + ["filename"]
    assert np.array_equal(single.iloc[:, :-1].to_numpy(), emb.iloc[:, H:2 * H].to_numpy())


def test_dropin_splits_a_batch_under_the_tap_budget(rsaf_lib, corpus, monkeypatch):
    """A budget below one file's planes runs every file alone: the same values as the whole batch."""
    import pandas as pd
    from robust_speech_analysis_framework_amd import w2v2
    cfg, sd, mdir, paths = corpus
    df = pd.DataFrame({"filepath": paths})
    whole = w2v2.extract_wav2vec2_sequences(df, model_name=mdir, verbose=False, output_layers=[0, 2])
    pooled = w2v2.extract_wav2vec2_embeddings(df, model_name=mdir, verbose=False, output_layers=[0, 2])
    monkeypatch.setattr(w2v2, "HIDDEN_TAP_BUDGET_BYTES", 1)
    split = w2v2.extract_wav2vec2_sequences(df, model_name=mdir, verbose=False, output_layers=[0, 2])
    assert list(split) == list(whole)
    for fn in whole:
        assert np.array_equal(split[fn], whole[fn])
    p2 = w2v2.extract_wav2vec2_embeddings(df, model_name=mdir, verbose=False, output_layers=[0, 2])
    assert np.array_equal(p2.iloc[:, :-1].to_numpy(), pooled.iloc[:, :-1].to_numpy())
