"""Wav2Vec2 hidden-state selection on the host side: ``output_layers`` validation, embedding column names, the C ABI's
refusal of bad tap lists (host-only, before any launch) and the committed goldens' shapes.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from robust_speech_analysis_framework_amd.w2v2 import embedding_rows, layer_selection
from robust_speech_analysis_framework_amd.w2v2_config import W2V2Config

HERE = os.path.dirname(os.path.abspath(__file__))
RSAF_ERR_ARG = 1


def test_layer_selection_normalises_negatives_and_keeps_the_requested_order():
    assert layer_selection(-1, 12) == ([12], [12], [0])
    assert layer_selection(0, 12) == ([0], [0], [0])
    assert layer_selection(-13, 12) == ([0], [0], [0])
    assert layer_selection([9, 0, -1], 12) == ([9, 0, 12], [0, 9, 12], [1, 0, 2])
    assert layer_selection((3, 3), 12) == ([3, 3], [3], [0, 0])
    assert layer_selection(np.int64(24), 24) == ([24], [24], [0])
    assert layer_selection([1, 2], None) is None                            # types only


@pytest.mark.parametrize("bad", [13, -14, [0, 13], (5, -20)])
def test_layer_selection_rejects_indices_out_of_range(bad):
    with pytest.raises(ValueError, match="out of range"):
        layer_selection(bad, 12)


@pytest.mark.parametrize("bad", [[], (), "1", 1.0, True, [1, "2"], [1.5], {1: 2}])
def test_layer_selection_rejects_what_is_not_an_int_or_a_list_of_ints(bad):
    with pytest.raises(ValueError, match="output_layers"):
        layer_selection(bad, 12)
    with pytest.raises(ValueError, match="output_layers"):
        layer_selection(bad)


def test_dropins_raise_before_any_device_work(monkeypatch):
    """A bad index is a ValueError raised before the library is even loaded (no GPU here)."""
    import pandas as pd
    from robust_speech_analysis_framework_amd import _lib, w2v2
    monkeypatch.setenv("RSAF_W2V2_RANDOM_SEED", "0")

    def boom(*a, **k):
        raise AssertionError("device work before the index check")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(w2v2, "get_engine", boom)
    df = pd.DataFrame({"filepath": ["/nonexistent.wav"]})
    with pytest.raises(ValueError, match="out of range"):
        w2v2.extract_wav2vec2_sequences(df, output_layers=13, verbose=False)
    with pytest.raises(ValueError, match="out of range"):
        w2v2.extract_wav2vec2_embeddings(df, output_layers=[0, -14], verbose=False)
    with pytest.raises(ValueError, match="output_layers"):
        w2v2.extract_wav2vec2_embeddings(df, output_layers=[], verbose=False)


def test_embedding_columns():
    m1 = {"a.wav": np.arange(4, dtype=np.float32)}
    rows = embedding_rows(m1, None)
    assert list(rows[0]) == ["dim_0", "dim_1", "dim_2", "dim_3", "filename"] and rows[0]["filename"] == "a.wav"
    m2 = {"b.wav": np.arange(6, dtype=np.float32).reshape(2, 3)}
    rows = embedding_rows(m2, [12, 0])
    assert list(rows[0]) == ["l12_dim_0", "l12_dim_1", "l12_dim_2", "l0_dim_0", "l0_dim_1", "l0_dim_2", "filename"]
    assert rows[0]["l0_dim_2"] == 5.0


def _hidden_call(lib, idx, n_hidden=None, layers=12, plane=768 * 4):
    """rsaf_w2v2_forward_ragged_hidden at the base geometry with NULL device pointers: only the host checks can run."""
    cfg = W2V2Config()
    lens = (C.c_int * 1)(80000)
    arr = (C.c_int * max(len(idx), 1))(*idx) if idx is not None else None
    out = C.c_void_p(16)
    return lib.rsaf_w2v2_forward_ragged_hidden(None, None, None, lens, 1, cfg.conv_dim[0], cfg.hidden_size, layers,
                                               cfg.num_attention_heads, cfg.intermediate_size, cfg.num_conv_pos_embeddings,
                                               cfg.num_conv_pos_embedding_groups, 1e-5, 0, None, None, 0, None, None, arr,
                                               len(idx) if n_hidden is None else n_hidden, out, plane, None)


@pytest.mark.parametrize("idx, n_hidden", [([0, 13], None), ([-1], None), ([3, 3], None), ([5, 2], None),
                                           (None, 2), ([0], -1), (list(range(14)), None)],
                         ids=["above_L", "negative", "repeated", "decreasing", "null_list", "negative_count", "too_many"])
def test_bad_tap_lists_return_err_arg_on_the_host(rsaf_lib, idx, n_hidden):
    assert _hidden_call(rsaf_lib, idx, n_hidden) == RSAF_ERR_ARG
    assert b"hidden" in rsaf_lib.rsaf_last_error()


def test_misaligned_tap_planes_return_err_arg_on_the_host(rsaf_lib):
    assert _hidden_call(rsaf_lib, [0, 12], plane=768 * 4 + 2) == RSAF_ERR_ARG


def test_segment_mean_refuses_bad_sizes_on_the_host(rsaf_lib):
    assert rsaf_lib.rsaf_rows_segment_mean_f32(None, 10, 100, 1, None, 1, 20, None, None) == RSAF_ERR_ARG       # ld < width
    assert rsaf_lib.rsaf_rows_segment_mean_f32(None, 10, 100, 1, None, 1, 10, None, None) == RSAF_ERR_ARG       # NULL rows
    assert rsaf_lib.rsaf_rows_segment_mean_f32(None, 10, 100, 0, None, 1, 10, None, None) == 0                  # nothing to do


def test_golden_hidden_states_shapes_match_transformers():
    """Every entry of the golden file has transformers' hidden_states shape: L + 1 states of [T, H]."""
    transformers = pytest.importorskip("transformers")
    import torch
    z = np.load(os.path.join(HERE, "golden", "w2v2_hidden_states_small.npz"))
    geom = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(z["cfg"])).items()}
    cfg = W2V2Config(**geom)
    hc = transformers.Wav2Vec2Config(conv_dim=cfg.conv_dim, hidden_size=cfg.hidden_size,
                                     num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                                     intermediate_size=cfg.intermediate_size,
                                     num_conv_pos_embeddings=cfg.num_conv_pos_embeddings,
                                     num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups)
    m = transformers.Wav2Vec2Model(hc).eval()
    for flags in range(8):
        for n in (8000, 20000):
            h = z[f"hidden_states_f{flags}_{n}"]
            with torch.no_grad():
                hs = m(torch.zeros(1, n), output_hidden_states=True).hidden_states
            assert h.dtype == np.float32 and h.shape == (len(hs),) + tuple(hs[0].shape[1:])
            assert np.isfinite(h).all()
