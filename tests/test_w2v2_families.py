"""HuBERT and WavLM checkpoints on the Wav2Vec2 path, host side: config.json -> W2V2Config, key shapes against transformers'
models, the packed distance table against ``WavLMAttention.compute_bias``, local directories written by ``save_pretrained``,
and the weight layout / workspace with the two new flags clear."""
import ctypes as C

import numpy as np
import pytest

from robust_speech_analysis_framework_amd.w2v2_config import (LAYER_FEAT_NORM, NO_FEAT_PROJ_LN, PRE_LN, REL_POS_BIAS,
                                                               REL_SPAN, W2V2Config, hf_shapes, load_local_model,
                                                               random_state_dict, relative_position_table, save_local_model)

SMALL = dict(conv_dim=(32,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
             intermediate_size=128, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
WAVLM_GEOMS = {                                     # hidden, layers, heads, intermediate, stable layer norm
    "base": (768, 12, 12, 3072, False), "base-plus": (768, 12, 12, 3072, False), "large": (1024, 24, 16, 4096, True)}


def _hf_kwargs(geom, **kw):
    return dict(conv_dim=list(geom["conv_dim"]), hidden_size=geom["hidden_size"], num_hidden_layers=geom["num_hidden_layers"],
                num_attention_heads=geom["num_attention_heads"], intermediate_size=geom["intermediate_size"],
                num_conv_pos_embeddings=geom["num_conv_pos_embeddings"],
                num_conv_pos_embedding_groups=geom["num_conv_pos_embedding_groups"], **kw)


@pytest.mark.parametrize("name", list(WAVLM_GEOMS))
def test_wavlm_config_json_maps_to_the_bias_flag(name):
    from transformers import WavLMConfig
    hidden, layers, heads, inter, stable = WAVLM_GEOMS[name]
    d = WavLMConfig(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=inter,
                    do_stable_layer_norm=stable, feat_extract_norm="layer" if stable else "group").to_dict()
    assert d["model_type"] == "wavlm"
    cfg = W2V2Config.from_hf_dict(d)
    cfg.validate()
    assert cfg.model_type == "wavlm" and cfg.feat_proj_layer_norm
    assert (cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size) == (hidden, layers, heads, inter)
    assert (cfg.num_buckets, cfg.max_bucket_distance) == (320, 800) and cfg.head_dim == 64
    assert cfg.flags == REL_POS_BIAS | ((LAYER_FEAT_NORM | PRE_LN) if stable else 0)


@pytest.mark.parametrize("fpln", [False, True])
def test_hubert_config_json_honours_feat_proj_layer_norm(fpln):
    from transformers import HubertConfig
    d = HubertConfig(feat_proj_layer_norm=fpln).to_dict()
    assert d["model_type"] == "hubert"
    cfg = W2V2Config.from_hf_dict(d)
    cfg.validate()
    assert cfg.model_type == "hubert" and cfg.feat_proj_layer_norm is fpln
    assert (cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads) == (768, 12, 12)
    assert cfg.flags == (0 if fpln else NO_FEAT_PROJ_LN)
    with pytest.raises(ValueError, match="conv_pos_batch_norm"):
        W2V2Config.from_hf_dict({**d, "conv_pos_batch_norm": True})


def test_unknown_model_type_is_refused_by_name():
    from transformers import Wav2Vec2Config
    d = Wav2Vec2Config().to_dict()
    assert W2V2Config.from_hf_dict(d).flags == 0 and W2V2Config.from_hf_dict(d).model_type == "wav2vec2"
    no_type = {k: v for k, v in d.items() if k != "model_type"}
    assert W2V2Config.from_hf_dict(no_type) == W2V2Config.from_hf_dict(d)         # absent = wav2vec2, as before
    for bad in ("data2vec-audio", "unispeech", "sew"):
        with pytest.raises(ValueError, match=bad):
            W2V2Config.from_hf_dict({**d, "model_type": bad})
    with pytest.raises(ValueError, match="max_bucket_distance"):                 # beyond the packed table
        W2V2Config(**SMALL, model_type="wavlm", max_bucket_distance=REL_SPAN).validate()
    with pytest.raises(ValueError, match="feat_proj_layer_norm"):                # not with the layer-norm feature encoder
        W2V2Config(**SMALL, model_type="hubert", feat_proj_layer_norm=False, feat_extract_norm="layer").validate()


@pytest.mark.parametrize("family, stable", [("wavlm", False), ("wavlm", True), ("hubert", False), ("hubert", True),
                                            ("hubert_noln", False)])
def test_hf_shapes_are_the_state_dict_of_transformers(family, stable):
    from transformers import HubertConfig, HubertModel, WavLMConfig, WavLMModel
    norm = dict(do_stable_layer_norm=stable, feat_extract_norm="layer" if stable else "group", conv_bias=stable)
    if family == "wavlm":
        cfg = W2V2Config(**SMALL, model_type="wavlm", num_buckets=32, max_bucket_distance=40, **norm)
        m = WavLMModel(WavLMConfig(**_hf_kwargs(SMALL, num_buckets=32, max_bucket_distance=40, **norm)))
    else:
        fpln = family == "hubert"
        cfg = W2V2Config(**SMALL, model_type="hubert", feat_proj_layer_norm=fpln, **norm)
        m = HubertModel(HubertConfig(**_hf_kwargs(SMALL, feat_proj_layer_norm=fpln, **norm)))
    want = {k: tuple(v.shape) for k, v in m.state_dict().items() if k != "masked_spec_embed"}
    assert hf_shapes(cfg) == want
    sd = random_state_dict(cfg, 3)
    base = random_state_dict(W2V2Config(**SMALL, **norm), 3)                     # the shared keys keep their draws
    if family != "hubert_noln":                                                  # (two keys fewer: the later draws move)
        assert all(np.array_equal(sd[k], v) for k, v in base.items())
    if family == "wavlm":
        assert sd["encoder.layers.1.attention.gru_rel_pos_linear.bias"].std() > 0.3   # O(1), so that the bias matters


@pytest.mark.parametrize("num_buckets, max_distance", [(320, 800), (32, 40)])
def test_packed_distance_table_is_compute_bias_through_the_clamped_index(num_buckets, max_distance):
    import torch
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    heads = 4
    att = WavLMAttention(embed_dim=64, num_heads=heads, num_buckets=num_buckets, max_distance=max_distance)
    torch.manual_seed(5)
    with torch.no_grad():
        att.rel_attn_embed.weight.normal_()
    cfg = W2V2Config(**SMALL, model_type="wavlm", num_buckets=num_buckets, max_bucket_distance=max_distance)
    tab = relative_position_table(cfg, att.rel_attn_embed.weight.detach().numpy())
    assert tab.shape == (heads, 2 * REL_SPAN - 1) and tab.dtype == np.float32
    for T in (249, 499, 1500):
        with torch.no_grad():
            want = att.compute_bias(T, T).numpy()                                  # [heads, q, k]
        d = np.arange(T)[None, :] - np.arange(T)[:, None]                          # k - q
        got = tab[:, np.clip(d, -(REL_SPAN - 1), REL_SPAN - 1) + REL_SPAN - 1]
        assert np.array_equal(got, want), T


def _offsets(lib, cfg, flags):
    from robust_speech_analysis_framework_amd.w2v2 import _cfg_args
    buf, n = (C.c_int64 * 512)(), C.c_int(0)
    assert lib.rsaf_w2v2_weight_offsets_ex(*_cfg_args(cfg), flags, buf, 512, C.byref(n)) == 0
    return [int(buf[i]) for i in range(n.value)], int(lib.rsaf_w2v2_weight_floats_ex(*_cfg_args(cfg), flags))


def test_local_wavlm_directory_loads_with_the_bias_flag_and_every_key_packed(rsaf_lib, tmp_path):
    """A directory written by WavLMModel.save_pretrained.  Before the families were told apart it loaded with flags == 0."""
    import torch
    from transformers import WavLMConfig, WavLMModel
    from robust_speech_analysis_framework_amd.w2v2 import pack_weights
    torch.manual_seed(0)
    m = WavLMModel(WavLMConfig(**_hf_kwargs(SMALL, num_buckets=32, max_bucket_distance=40)))
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "gru_rel_pos" in k or "rel_attn_embed" in k:
                p.normal_()
    m.save_pretrained(str(tmp_path / "wavlm"))
    cfg, sd = load_local_model(str(tmp_path / "wavlm"))
    assert cfg.model_type == "wavlm" and cfg.flags == REL_POS_BIAS and (cfg.num_buckets, cfg.max_bucket_distance) == (32, 40)
    blob = pack_weights(cfg, sd)
    offs, total = _offsets(rsaf_lib, cfg, cfg.flags)
    assert blob.size == total
    hd, NH, L = cfg.head_dim, cfg.num_attention_heads, cfg.num_hidden_layers
    tail = offs[-(4 * L + 1):]
    for l in range(L):
        p = f"encoder.layers.{l}.attention."
        w, b = sd[p + "gru_rel_pos_linear.weight"].astype(np.float64), sd[p + "gru_rel_pos_linear.bias"].astype(np.float64)
        ga, gb, gbias, gconst = tail[4 * l:4 * l + 4]
        assert np.array_equal(blob[ga:ga + hd], w[:4].sum(0).astype(np.float32))
        assert np.array_equal(blob[gb:gb + hd], w[4:].sum(0).astype(np.float32))
        assert np.array_equal(blob[gbias:gbias + 2], np.array([b[:4].sum(), b[4:].sum()]).astype(np.float32))
        assert np.array_equal(blob[gconst:gconst + NH], sd[p + "gru_rel_pos_const"].reshape(-1))
    tab = blob[tail[-1]:tail[-1] + NH * (2 * REL_SPAN - 1)].reshape(NH, -1)
    assert np.array_equal(tab, relative_position_table(cfg, sd["encoder.layers.0.attention.rel_attn_embed.weight"]))
    assert np.abs(tab).min() > 0                                                  # no entry left unfilled
    # the family's head checkpoints carry a prefix
    from robust_speech_analysis_framework_amd.w2v2_config import _strip_prefix
    assert set(_strip_prefix({"wavlm." + k: v for k, v in sd.items()})) == set(sd)


def test_local_hubert_directory_without_the_projection_layernorm_loads(rsaf_lib, tmp_path):
    """A directory written by HubertModel(feat_proj_layer_norm=False).save_pretrained.  It used to raise KeyError."""
    from transformers import HubertConfig, HubertModel
    from robust_speech_analysis_framework_amd.w2v2 import pack_weights
    HubertModel(HubertConfig(**_hf_kwargs(SMALL, feat_proj_layer_norm=False))).save_pretrained(str(tmp_path / "hubert"))
    cfg, sd = load_local_model(str(tmp_path / "hubert"))
    assert cfg.model_type == "hubert" and cfg.flags == NO_FEAT_PROJ_LN
    assert "feature_projection.layer_norm.weight" not in sd
    blob = pack_weights(cfg, sd)
    assert blob.size == _offsets(rsaf_lib, cfg, cfg.flags)[1] == _offsets(rsaf_lib, cfg, 0)[1]   # same layout, two slots unused
    # a round trip through the build's own writer keeps the family
    save_local_model(str(tmp_path / "again"), cfg, sd)
    cfg2, sd2 = load_local_model(str(tmp_path / "again"))
    assert cfg2 == cfg and set(sd2) == set(sd)
    wl = W2V2Config(**SMALL, model_type="wavlm", num_buckets=32, max_bucket_distance=40)
    save_local_model(str(tmp_path / "wl"), wl, random_state_dict(wl, 1))
    assert load_local_model(str(tmp_path / "wl"))[0] == wl


@pytest.mark.parametrize("geom", [SMALL, {}], ids=["small", "base"])
def test_new_flags_clear_leave_layout_and_workspace_as_they_were(rsaf_lib, geom):
    from robust_speech_analysis_framework_amd.w2v2 import _cfg_args, pack_weights
    cfg = W2V2Config(**geom)
    lens = (C.c_int * 3)(80000, 52000, 9000)
    for flags in range(16):
        offs, total = _offsets(rsaf_lib, cfg, flags)
        ws = rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 3, *_cfg_args(cfg), flags)
        assert ws > 0
        if flags == 0:
            buf, n = (C.c_int64 * 512)(), C.c_int(0)
            assert rsaf_lib.rsaf_w2v2_weight_offsets(*_cfg_args(cfg), buf, 512, C.byref(n)) == 0
            assert offs == [int(buf[i]) for i in range(n.value)] and total == rsaf_lib.rsaf_w2v2_weight_floats(*_cfg_args(cfg))
            assert ws == rsaf_lib.rsaf_w2v2_workspace_bytes_ragged(lens, 3, *_cfg_args(cfg))
        # the new segments only ever follow the old ones, and the gates are the only new workspace
        rel, rtotal = _offsets(rsaf_lib, cfg, flags | REL_POS_BIAS)
        L, NH, hd = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.head_dim
        assert rel[:len(offs)] == offs and len(rel) == len(offs) + 4 * L + 1 and rel[len(offs)] == total
        pad4 = lambda k: (k + 3) & ~3                                              # noqa: E731
        assert rtotal == total + L * (2 * pad4(hd) + 4 + pad4(NH)) + pad4(NH * (2 * REL_SPAN - 1))
        rows = sum(cfg.frames(l) for l in lens)
        assert rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 3, *_cfg_args(cfg), flags | REL_POS_BIAS) == ws + 4 * pad4(rows * NH)
        if not flags & LAYER_FEAT_NORM:
            assert _offsets(rsaf_lib, cfg, flags | NO_FEAT_PROJ_LN) == (offs, total)
            assert rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 3, *_cfg_args(cfg), flags | NO_FEAT_PROJ_LN) == ws
    # bad combinations and unknown bits are refused on the host
    assert rsaf_lib.rsaf_w2v2_weight_floats_ex(*_cfg_args(cfg), NO_FEAT_PROJ_LN | LAYER_FEAT_NORM) == -1
    assert rsaf_lib.rsaf_w2v2_weight_floats_ex(*_cfg_args(cfg), 128) == -1
    # pack_weights fills every segment of every family (it asserts that none is left over)
    if geom:
        for kw in (dict(model_type="wavlm", num_buckets=32, max_bucket_distance=40),
                   dict(model_type="wavlm", do_stable_layer_norm=True, feat_extract_norm="layer", conv_bias=True),
                   dict(model_type="hubert", feat_proj_layer_norm=False, conv_bias=True)):
            fam = W2V2Config(**geom, **kw)
            assert pack_weights(fam, random_state_dict(fam, 2)).size == _offsets(rsaf_lib, fam, fam.flags)[1]
