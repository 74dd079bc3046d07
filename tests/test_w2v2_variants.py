"""Large-checkpoint Wav2Vec2 variants on the host side: config parsing, HF key layout, weight ABI, local directories.

No GPU: the weight-layout calls of the C ABI are host-only."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from robust_speech_analysis_framework_amd.w2v2_config import (CONV_BIAS, LAYER_FEAT_NORM, NO_INPUT_NORM, PRE_LN, W2V2Config,
                                                               hf_shapes, load_local_model, random_state_dict,
                                                               save_local_model)

SMALL = dict(conv_dim=(32,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
             intermediate_size=128, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)


def _variant(flags, do_normalize=True, **geom):
    return W2V2Config(**(geom or SMALL), feat_extract_norm="layer" if flags & 1 else "group", conv_bias=bool(flags & 2),
                      do_stable_layer_norm=bool(flags & 4), do_normalize=do_normalize)


def _hf_large(**over):
    """config.json of wav2vec2-large-960h-lv60-self / XLS-R 300M as published (the keys this build reads)."""
    d = {"architectures": ["Wav2Vec2ForCTC"], "conv_bias": True, "conv_dim": [512] * 7,
         "conv_kernel": [10, 3, 3, 3, 3, 2, 2], "conv_stride": [5, 2, 2, 2, 2, 2, 2], "do_stable_layer_norm": True,
         "feat_extract_activation": "gelu", "feat_extract_norm": "layer", "hidden_act": "gelu", "hidden_size": 1024,
         "intermediate_size": 4096, "layer_norm_eps": 1e-5, "model_type": "wav2vec2", "num_attention_heads": 16,
         "num_conv_pos_embedding_groups": 16, "num_conv_pos_embeddings": 128, "num_hidden_layers": 24,
         "add_adapter": False, "adapter_attn_dim": None}
    d.update(over)
    return d


def test_from_hf_dict_accepts_the_large_checkpoints():
    lv60 = W2V2Config.from_hf_dict(_hf_large())
    assert lv60.flags == LAYER_FEAT_NORM | CONV_BIAS | PRE_LN
    assert (lv60.hidden_size, lv60.num_hidden_layers, lv60.head_dim) == (1024, 24, 64)
    xlsr = W2V2Config.from_hf_dict(_hf_large(architectures=["Wav2Vec2ForPreTraining"]), do_normalize=False)
    assert xlsr.flags == LAYER_FEAT_NORM | CONV_BIAS | PRE_LN | NO_INPUT_NORM
    # HF allows every mix, e.g. a layer-norm feature encoder in front of a post-LN encoder
    mix = W2V2Config.from_hf_dict(_hf_large(do_stable_layer_norm=False, conv_bias=False))
    assert mix.flags == LAYER_FEAT_NORM
    base = W2V2Config.from_hf_dict(_hf_large(feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False))
    assert base.flags == 0


@pytest.mark.parametrize("over, what", [({"hidden_act": "relu"}, "hidden_act"),
                                        ({"feat_extract_activation": "relu"}, "feat_extract_activation"),
                                        ({"add_adapter": True, "adapter_attn_dim": 16}, "adapter"),
                                        ({"hidden_size": 1280, "num_attention_heads": 16}, "1024"),
                                        ({"feat_extract_norm": "batch"}, "feat_extract_norm")])
def test_from_hf_dict_still_rejects_what_it_cannot_run(over, what):
    with pytest.raises(ValueError, match=what):
        W2V2Config.from_hf_dict(_hf_large(**over))


@pytest.mark.parametrize("flags", range(8))
def test_hf_shapes_match_transformers(flags):
    import torch
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    cfg = _variant(flags)
    torch.manual_seed(0)
    hc = Wav2Vec2Config(conv_dim=cfg.conv_dim, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        num_conv_pos_embeddings=cfg.num_conv_pos_embeddings,
                        num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups,
                        feat_extract_norm=cfg.feat_extract_norm, conv_bias=cfg.conv_bias,
                        do_stable_layer_norm=cfg.do_stable_layer_norm)
    want = {k: tuple(v.shape) for k, v in Wav2Vec2Model(hc).state_dict().items() if k != "masked_spec_embed"}
    assert hf_shapes(cfg) == want


def _offsets(lib, cfg, flags=None):
    args = (cfg.conv_dim[0], cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size,
            cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups)
    cap = 128 + 12 * cfg.num_hidden_layers
    buf = (C.c_int64 * cap)()
    n = C.c_int(0)
    if flags is None:
        assert lib.rsaf_w2v2_weight_offsets(*args, buf, cap, C.byref(n)) == 0
        return [buf[i] for i in range(n.value)], lib.rsaf_w2v2_weight_floats(*args)
    assert lib.rsaf_w2v2_weight_offsets_ex(*args, flags, buf, cap, C.byref(n)) == 0
    return [buf[i] for i in range(n.value)], lib.rsaf_w2v2_weight_floats_ex(*args, flags)


@pytest.mark.parametrize("geom", [SMALL, {}])
def test_weight_layout_ex(rsaf_lib, geom):
    cfg = W2V2Config(**geom)
    C_ = cfg.conv_dim[0]
    base, total0 = _offsets(rsaf_lib, cfg)
    assert _offsets(rsaf_lib, cfg, 0) == (base, total0)
    for flags in range(16):
        offs, total = _offsets(rsaf_lib, cfg, flags)
        assert offs[:len(base)] == base                            # the base segments never move
        extra = offs[len(base):]
        want, o = [], total0
        if flags & CONV_BIAS:                                      # conv biases [7][C]
            want += [o + i * C_ for i in range(7)]
            o += 7 * C_
        if flags & LAYER_FEAT_NORM:                                # conv LayerNorms [7][2][C]: gamma_i, beta_i
            want += [o + j * C_ for j in range(14)]
            o += 14 * C_
        assert extra == want and total == o, flags
    assert rsaf_lib.rsaf_w2v2_weight_floats_ex(*[C_, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                                                 cfg.intermediate_size, cfg.num_conv_pos_embeddings,
                                                 cfg.num_conv_pos_embedding_groups], 16) == -1    # unknown flag bit


def test_workspace_ex_with_flags_zero_is_the_base_workspace(rsaf_lib):
    cfg = W2V2Config()
    lens = (C.c_int * 3)(80000, 80000, 32000)
    args = (cfg.conv_dim[0], cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size,
            cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups)
    base = rsaf_lib.rsaf_w2v2_workspace_bytes_ragged(lens, 3, *args)
    assert base > 0 and rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 3, *args, 0) == base
    assert rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 3, *args, 15) >= base


def test_pack_weights_fills_the_appended_segments(rsaf_lib):
    from robust_speech_analysis_framework_amd.w2v2 import pack_weights, weight_offsets
    cfg = _variant(LAYER_FEAT_NORM | CONV_BIAS | PRE_LN)
    sd = random_state_dict(cfg, 3)
    blob = pack_weights(cfg, sd)
    offs, total = weight_offsets(cfg)
    assert blob.size == total
    C_ = cfg.conv_dim[0]
    ext = offs[-21:]
    for i in range(7):
        assert np.array_equal(blob[ext[i]:ext[i] + C_], sd[f"feature_extractor.conv_layers.{i}.conv.bias"])
        assert np.array_equal(blob[ext[7 + 2 * i]:ext[7 + 2 * i] + C_], sd[f"feature_extractor.conv_layers.{i}.layer_norm.weight"])
        assert np.array_equal(blob[ext[8 + 2 * i]:ext[8 + 2 * i] + C_], sd[f"feature_extractor.conv_layers.{i}.layer_norm.bias"])
    assert not blob[offs[1]:offs[1] + C_].any() and not blob[offs[2]:offs[2] + C_].any()   # GroupNorm slots unused
    # flags 0: the blob of the base architecture is what it was
    cfg0 = W2V2Config(**SMALL)
    assert pack_weights(cfg0, random_state_dict(cfg0, 3)).size == weight_offsets(cfg0)[1]


@pytest.mark.parametrize("flags, norm", [(0, True), (LAYER_FEAT_NORM | CONV_BIAS | PRE_LN, True),
                                         (LAYER_FEAT_NORM | CONV_BIAS | PRE_LN, False), (CONV_BIAS, False)])
def test_local_directory_round_trip_keeps_the_variant(tmp_path, flags, norm):
    cfg = _variant(flags, do_normalize=norm)
    sd = random_state_dict(cfg, 5)
    save_local_model(str(tmp_path), cfg, sd)
    assert os.path.exists(tmp_path / "preprocessor_config.json") == (not norm)
    cfg2, sd2 = load_local_model(str(tmp_path))
    assert cfg2.flags == cfg.flags == flags | (0 if norm else NO_INPUT_NORM)
    assert (cfg2.feat_extract_norm, cfg2.conv_bias, cfg2.do_stable_layer_norm, cfg2.do_normalize) == \
        (cfg.feat_extract_norm, cfg.conv_bias, cfg.do_stable_layer_norm, cfg.do_normalize)
    assert sorted(sd2) == sorted(sd)


def test_default_config_json_is_unchanged(tmp_path):
    """The base architecture's config.json is byte for byte what it was before the variants existed."""
    cfg = W2V2Config(**SMALL)
    save_local_model(str(tmp_path), cfg, random_state_dict(cfg, 1))
    want = {"conv_dim": [32] * 7, "conv_kernel": [10, 3, 3, 3, 3, 2, 2], "conv_stride": [5, 2, 2, 2, 2, 2, 2],
            "hidden_size": 64, "num_hidden_layers": 2, "num_attention_heads": 4, "intermediate_size": 128,
            "num_conv_pos_embeddings": 16, "num_conv_pos_embedding_groups": 4, "layer_norm_eps": 1e-5,
            "feat_extract_norm": "group", "feat_extract_activation": "gelu", "hidden_act": "gelu",
            "do_stable_layer_norm": False, "conv_bias": False, "model_type": "wav2vec2"}
    assert (tmp_path / "config.json").read_text() == json.dumps(want)
    assert not (tmp_path / "preprocessor_config.json").exists()


def test_pretraining_checkpoint_keys_and_preprocessor_are_honoured(tmp_path):
    """XLSR-53 / XLS-R ship as Wav2Vec2ForPreTraining: wav2vec2.* keys beside quantizer / project_q / project_hid."""
    from safetensors.numpy import save_file
    cfg = _variant(LAYER_FEAT_NORM | CONV_BIAS | PRE_LN)
    sd = random_state_dict(cfg, 9)
    st = {"wav2vec2." + k: v for k, v in sd.items()}
    st["quantizer.codevectors"] = np.zeros((1, 640, 384), np.float32)
    st["quantizer.weight_proj.weight"] = np.zeros((640, 32), np.float32)
    st["project_q.weight"] = np.zeros((256, 768), np.float32)
    st["project_hid.weight"] = np.zeros((256, 64), np.float32)
    save_local_model(str(tmp_path), cfg, sd)
    save_file(st, str(tmp_path / "model.safetensors"))
    (tmp_path / "preprocessor_config.json").write_text(json.dumps({"do_normalize": False, "sampling_rate": 16000}))
    cfg2, sd2 = load_local_model(str(tmp_path))
    assert cfg2.flags == LAYER_FEAT_NORM | CONV_BIAS | PRE_LN | NO_INPUT_NORM
    assert sorted(sd2) == sorted(sd)
