"""data2vec-audio checkpoints on the HIP Wav2Vec2 path against transformers' Data2VecAudioModel: committed goldens at the small
geometry (every hidden state, windows of 1 to 62 frames, odd and even kernels; a forward that stops one stack layer early
cannot pass), the model run on the CPU at test time at the base and the large widths and on the exact-fp32 route, the
ragged-call bit identity, the refusals of the C entry point, and the drop-ins on a local data2vec-audio directory."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

from robust_speech_analysis_framework_amd import synth
from robust_speech_analysis_framework_amd.w2v2_config import (LAYER_FEAT_NORM, POS_CONV_STACK, POS_DEPTH_SHIFT, PRE_LN, REL_POS_BIAS,
                                                               W2V2Config, random_state_dict, save_local_model)

TOL = 1e-4      # north_star: <= 1e-4 relative for float outputs
D2V = dict(model_type="data2vec-audio", feat_extract_norm="layer")
# two encoder layers: the stack sits in front of the encoder, and the CPU reference stays at seconds
BASE2 = dict(conv_dim=(512,) * 7, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072,
             num_conv_pos_embeddings=5, conv_pos_kernel_size=19, num_conv_pos_embedding_groups=16)
LARGE2 = dict(conv_dim=(512,) * 7, hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096,
              num_conv_pos_embeddings=5, conv_pos_kernel_size=19, num_conv_pos_embedding_groups=16)


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
    """transformers' Data2VecAudioModel of the config with the weights ``sd``, on the CPU."""
    import torch
    from transformers import Data2VecAudioConfig, Data2VecAudioModel
    torch.set_num_threads(16)
    m = Data2VecAudioModel(Data2VecAudioConfig(
        conv_dim=cfg.conv_dim, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
        num_conv_pos_embeddings=cfg.num_conv_pos_embeddings, conv_pos_kernel_size=cfg.conv_pos_kernel_size,
        num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups, layer_norm_eps=cfg.layer_norm_eps,
        conv_bias=cfg.conv_bias))
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"masked_spec_embed"}, res
    return m.eval()


def _hf_hidden(m, cfg, windows, layers=None):
    """One window at a time (the reference loop runs batch 1): per window [len(layers), T, H]; layers None = all."""
    import torch
    from transformers import Wav2Vec2FeatureExtractor
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
GOLDEN_CASES = ("d2v", "d2v_bias", "d2v_even", "d2v_one")
GOLDEN_LENGTHS = (400, 1000, 3000, 8000, 20000)                                  # T = 1, 2, 9, 24, 62


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "w2v2_data2vec_small.npz"))
    geom = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(z["cfg"])).items()}
    return z, geom, json.loads(str(z["cases"])), {}


@pytest.mark.parametrize("n", GOLDEN_LENGTHS)
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_small_data2vec_matches_transformers_goldens(rsaf_lib, golden, name, n):
    """Every hidden state of Data2VecAudioModel (tests/golden/make_w2v2_data2vec_golden.py).  Group width 16: the MFMA kernel
    of the positional stack, its one partly filled row tile, windows shorter than the half kernel."""
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    z, geom, cases, engines = golden
    cfg = W2V2Config(**geom, **cases[name], **D2V)
    assert cfg.flags & POS_CONV_STACK and cfg.flags >> POS_DEPTH_SHIFT == cases[name]["num_conv_pos_embeddings"]
    if name not in engines:
        engines[name] = W2V2Engine(cfg, random_state_dict(cfg, seed=int(z["seed"])))
    layers = list(range(cfg.num_hidden_layers + 1))
    out, planes, rows = _run(engines[name], synth.synth_clip(50, 2.0)[:n], [(0, n)], layers)
    want = z[f"hidden_states_{name}_{n}"]
    _check_states(planes, rows, [want], layers)
    assert np.array_equal(out, planes[-1])
    # what a forward that stops one stack layer early returns is far from the reference, so the check above sees every layer
    blind = z[f"short_stack_last_hidden_state_{name}_{n}"]
    print(f"reference one stack layer short: rel {_rel(blind, want[-1]):.3e}; this forward against it: {_rel(out, blind):.3e}")
    assert _rel(blind, want[-1]) > 100 * TOL
    assert _rel(out, blind) > 100 * TOL


# ---- transformers on the CPU at test time ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def d2v_base():
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = W2V2Config(**BASE2, **D2V)
    assert cfg.flags == LAYER_FEAT_NORM | POS_CONV_STACK | 5 << POS_DEPTH_SHIFT
    sd = random_state_dict(cfg, seed=41)
    return cfg, sd, W2V2Engine(cfg, sd)


def test_data2vec_base_widths_match_transformers(rsaf_lib, d2v_base):
    """768 / 16 groups (48 channels per group, 57 k16 units: an odd count), D = 5, K = 19: a 5 s window and a 2 s tail in one
    call, then a 10 s window (T = 499: two row tiles) and a 21 s window (T = 1049: five, the last one partly filled)."""
    cfg, sd, eng = d2v_base
    m = _hf_model(cfg, sd)
    clip = synth.synth_clip(320, 23.0)
    spec = [(0, 80000), (64000, 32000)]
    layers = [0, 1, 2]
    _, planes, rows = _run(eng, clip, spec, layers)
    assert list(np.diff(rows)) == [249, 99]
    _check_states(planes, rows, _hf_hidden(m, cfg, [clip[s:s + l] for s, l in spec], layers), layers)
    for start, length, T in ((16000, 160000, 499), (8000, 336000, 1049)):
        _, planes, rows = _run(eng, clip, [(start, length)], layers)
        assert rows[-1] == T
        _check_states(planes, rows, _hf_hidden(m, cfg, [clip[start:start + length]], layers), layers)


def test_data2vec_large_widths_match_transformers(rsaf_lib):
    """1024 / 16 groups: 64 channels per group."""
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = W2V2Config(**LARGE2, **D2V)
    sd = random_state_dict(cfg, seed=42)
    eng = W2V2Engine(cfg, sd)
    clip = synth.synth_clip(321, 7.0)
    spec = [(0, 80000), (64000, 32000)]
    layers = [0, 1, 2]
    _, planes, rows = _run(eng, clip, spec, layers)
    _check_states(planes, rows, _hf_hidden(_hf_model(cfg, sd), cfg, [clip[s:s + l] for s, l in spec], layers), layers)


def test_data2vec_exact_fp32_route_matches_transformers(rsaf_lib):
    """A group width of 8 (hidden 64, 8 groups): regroup + exact-fp32 GEMM + the row pass per stack layer."""
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    cfg = W2V2Config(conv_dim=(32,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                     num_conv_pos_embeddings=5, conv_pos_kernel_size=19, num_conv_pos_embedding_groups=8, **D2V)
    sd = random_state_dict(cfg, seed=43)
    eng = W2V2Engine(cfg, sd)
    clip = synth.synth_clip(50, 2.0)
    layers = [0, 1, 2]
    _, planes, rows = _run(eng, clip, [(0, 8000)], layers)
    _check_states(planes, rows, _hf_hidden(_hf_model(cfg, sd), cfg, [clip[:8000]], layers), layers)


def test_data2vec_ragged_call_returns_the_bits_of_the_per_length_calls(rsaf_lib, d2v_base):
    """Six windows of mixed lengths packed row after row, a one-frame window last: a halo that reads a neighbour's rows, or a
    plane scale that depends on the other windows of the call, changes bits here."""
    import torch
    cfg, sd, eng = d2v_base
    clip = synth.synth_clip(313, 7.0)
    spec = [(0, 80000), (1000, 52000), (64000, 48000), (5, 80000), (30000, 9000), (200, 400)]
    together, _, rows = _run(eng, clip, spec)
    assert rows[-1] - rows[-2] == 1
    wav = torch.from_numpy(clip).cuda()
    alone = torch.zeros((int(rows[-1]), cfg.hidden_size), device="cuda")
    for k, (s0, l) in enumerate(spec):
        eng.forward_windows(wav, [s0], [l], alone, [int(rows[k])])
    torch.cuda.synchronize()
    assert np.isfinite(together).all() and np.array_equal(together, alone.cpu().numpy())


def test_bad_stack_flags_are_refused_before_any_launch(rsaf_lib):
    import ctypes as C
    import torch
    from robust_speech_analysis_framework_amd import _lib
    geom = (32, 64, 2, 4, 128)                                                   # conv_dim, hidden, layers, heads, intermediate
    buf = torch.zeros(1 << 20, device="cuda")
    lens = (C.c_int * 1)(8000)
    dev = torch.zeros(8, dtype=torch.int64, device="cuda")
    depth = 5 << POS_DEPTH_SHIFT
    ok = POS_CONV_STACK | LAYER_FEAT_NORM | depth
    assert rsaf_lib.rsaf_w2v2_weight_floats_ex(*geom, 19, 4, ok) > 0              # the word the refused ones are variations of
    for flags, kernel in ((POS_CONV_STACK | LAYER_FEAT_NORM, 19), (LAYER_FEAT_NORM | depth, 18), (ok | PRE_LN, 19),
                          (ok | REL_POS_BIAS, 19), (POS_CONV_STACK | depth, 19), (ok, 65)):
        rc = rsaf_lib.rsaf_w2v2_forward_ragged_ex(_lib.ptr(buf), _lib.ptr(dev), _lib.ptr(dev), lens, 1, *geom, kernel, 4, 1e-5, flags,
                                                  _lib.ptr(buf), _lib.ptr(buf), buf.numel() * 4, _lib.ptr(buf), None, None)
        assert rc != 0, (flags, kernel)
        assert rsaf_lib.rsaf_w2v2_weight_floats_ex(*geom, kernel, 4, flags) == -1, (flags, kernel)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                                         # nothing ran


# ---- the drop-ins on a local data2vec-audio directory ------------------------------------------------------------------
def test_dropins_on_a_local_data2vec_directory(rsaf_lib, tmp_path):
    import pandas as pd
    from robust_speech_analysis_framework_amd import w2v2
    from robust_speech_analysis_framework_amd.w2v2_config import chunk_plan
    cfg = W2V2Config(conv_dim=(32,) * 7, hidden_size=128, num_hidden_layers=8, num_attention_heads=2, intermediate_size=256,
                     num_conv_pos_embeddings=5, conv_pos_kernel_size=19, num_conv_pos_embedding_groups=4, **D2V)
    assert cfg.head_dim == 64                                                    # the fused attention kernel
    sd = random_state_dict(cfg, seed=9)
    mdir = tmp_path / "data2vec"
    save_local_model(str(mdir), cfg, sd)
    written = json.loads((mdir / "config.json").read_text())
    assert (written["model_type"], written["conv_pos_kernel_size"], written["num_conv_pos_embeddings"]) == ("data2vec-audio", 19, 5)
    paths = synth.write_synth_corpus(str(tmp_path / "wav"), 1, 11.0, first=71)
    df = pd.DataFrame({"filepath": [paths[0]]})
    clip = synth.synth_clip(71, 11.0)
    plan = chunk_plan(len(clip))
    sel = [0, 6, -1]
    refs = _hf_hidden(_hf_model(cfg, sd), cfg, [clip[s:s + l] for s, l in plan], [0, 6, 8])
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
