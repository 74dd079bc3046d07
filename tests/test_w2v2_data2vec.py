"""data2vec-audio on the Wav2Vec2 path, host side: config.json -> W2V2Config (flags, the arguments of the C entry points, the
refusals by name), key shapes against transformers' Data2VecAudioModel, the weight blob with the stack's segments, local
directories, and the layout / draws / workspace of the other families pinned to what they were before the family existed."""
import ctypes as C
import zlib

import numpy as np
import pytest

from robust_speech_analysis_framework_amd.w2v2_config import (CONV_BIAS, LAYER_FEAT_NORM, POS_CONV_STACK, POS_DEPTH_SHIFT, W2V2Config,
                                                               hf_shapes, load_local_model, random_state_dict, save_local_model)

SMALL = dict(conv_dim=(32,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
             intermediate_size=128, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
D2V_SMALL = {**SMALL, "num_conv_pos_embeddings": 5, "conv_pos_kernel_size": 19, "model_type": "data2vec-audio",
             "feat_extract_norm": "layer"}


def _hf_config(cfg, **kw):
    from transformers import Data2VecAudioConfig
    return Data2VecAudioConfig(conv_dim=list(cfg.conv_dim), hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                               num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                               num_conv_pos_embeddings=cfg.num_conv_pos_embeddings, conv_pos_kernel_size=cfg.conv_pos_kernel_size,
                               num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups, conv_bias=cfg.conv_bias, **kw)


@pytest.mark.parametrize("conv_bias", [False, True])
def test_data2vec_config_json_maps_to_the_stack_flag_and_depth(conv_bias):
    from transformers import Data2VecAudioConfig
    from robust_speech_analysis_framework_amd.w2v2 import _cfg_args
    # the two switches transformers' Data2VecAudioModel ignores are ignored here too
    d = Data2VecAudioConfig(conv_bias=conv_bias, layer_norm_eps=1e-6, feat_extract_norm="group", do_stable_layer_norm=True).to_dict()
    assert d["model_type"] == "data2vec-audio" and d["num_conv_pos_embeddings"] == 5 and d["conv_pos_kernel_size"] == 19
    cfg = W2V2Config.from_hf_dict(d)
    cfg.validate()
    assert cfg.model_type == "data2vec-audio" and cfg.feat_extract_norm == "layer" and not cfg.do_stable_layer_norm
    assert cfg.feat_proj_layer_norm and cfg.conv_bias is conv_bias and cfg.layer_norm_eps == 1e-6
    assert (cfg.num_conv_pos_embeddings, cfg.conv_pos_kernel_size, cfg.num_conv_pos_embedding_groups) == (5, 19, 16)
    assert cfg.flags == LAYER_FEAT_NORM | (CONV_BIAS if conv_bias else 0) | POS_CONV_STACK | 5 << POS_DEPTH_SHIFT
    assert _cfg_args(cfg) == (512, 768, 12, 12, 3072, 19, 16)                     # pos_kernel = the stack's taps, not its depth
    even = W2V2Config.from_hf_dict({**d, "conv_pos_kernel_size": 4, "num_conv_pos_embeddings": 3})
    even.validate()                                                              # the "kernel even" rule is the other families'
    assert even.flags >> POS_DEPTH_SHIFT == 3 and _cfg_args(even)[5] == 4
    # the other families keep their meaning of num_conv_pos_embeddings and their flags
    from transformers import Wav2Vec2Config
    w = W2V2Config.from_hf_dict(Wav2Vec2Config().to_dict())
    assert w.flags == 0 and _cfg_args(w)[5] == 128
    with pytest.raises(ValueError, match="even"):
        W2V2Config(**{**SMALL, "num_conv_pos_embeddings": 19}).validate()


def test_data2vec_configs_this_build_cannot_run_are_refused_by_name():
    from transformers import Data2VecAudioConfig, Wav2Vec2Config
    d = Data2VecAudioConfig().to_dict()
    relabelled = {**Wav2Vec2Config().to_dict(), "model_type": "data2vec-audio"}  # depth 128, no conv_pos_kernel_size
    no_kernel = {k: v for k, v in d.items() if k != "conv_pos_kernel_size"}
    for bad in (relabelled, {**d, "num_conv_pos_embeddings": 0}, {**d, "num_conv_pos_embeddings": 16}, no_kernel,
                {**d, "conv_pos_kernel_size": 65}, {**d, "add_adapter": True}, {**d, "hidden_act": "relu"},
                {**d, "hidden_size": 1280}):
        with pytest.raises(ValueError, match="data2vec-audio"):
            W2V2Config.from_hf_dict(bad)
    for kw in (dict(num_conv_pos_embeddings=0), dict(num_conv_pos_embeddings=16), dict(conv_pos_kernel_size=65),
               dict(feat_extract_norm="group"), dict(do_stable_layer_norm=True)):
        with pytest.raises(ValueError, match="data2vec-audio"):
            W2V2Config(**{**D2V_SMALL, **kw}).validate()
    for other in ("unispeech", "sew"):
        with pytest.raises(ValueError, match=other):
            W2V2Config.from_hf_dict({**d, "model_type": other})


@pytest.mark.parametrize("conv_bias", [False, True])
def test_hf_shapes_are_the_state_dict_of_data2vec_audio_model(conv_bias):
    from transformers import Data2VecAudioModel
    cfg = W2V2Config(**D2V_SMALL, conv_bias=conv_bias)
    m = Data2VecAudioModel(_hf_config(cfg))
    want = {k: tuple(v.shape) for k, v in m.state_dict().items() if k != "masked_spec_embed"}
    assert hf_shapes(cfg) == want
    keys = list(hf_shapes(cfg))
    assert all("pos_conv_embed" in k for k in keys[-10:]) and not any("pos_conv_embed" in k for k in keys[:-10])   # last
    sd = random_state_dict(cfg, 3)
    w = sd["encoder.pos_conv_embed.layers.4.conv.weight"]
    assert abs(w.std() * np.sqrt(16 * 19) - 1.0) < 0.05                          # N(0, 1 / fan_in)
    assert abs(sd["encoder.pos_conv_embed.layers.4.conv.bias"].std() / 0.05 - 1.0) < 0.3


# (key -> CRC32 of the float32 bytes, keys), taken with seed 7 at the commit before data2vec-audio was added
PARENT_DRAWS = {
    (): ({"feature_extractor.conv_layers.0.conv.weight": 278742948, "feature_projection.projection.bias": 3352873186,
          "encoder.pos_conv_embed.conv.parametrizations.weight.original1": 723978153,
          "encoder.layers.1.final_layer_norm.bias": 1832509655}, 50),
    (("conv_bias", True), ("feat_extract_norm", "layer")): (
        {"feature_extractor.conv_layers.0.conv.weight": 278742948, "feature_projection.projection.bias": 1469709923,
         "encoder.pos_conv_embed.conv.parametrizations.weight.original1": 1340166730,
         "encoder.layers.1.final_layer_norm.bias": 4086486271}, 69),
}
# the same two configs: (CRC32 of the int64 offsets, number of offsets, weight floats, CRC32 of the packed blob, workspace
# bytes of windows of 80 000, 32 000 and 400 samples) at that commit
PARENT_LAYOUT = {(): (1878173020, 41, 102464, 475351063, 15205040),
                 (("conv_bias", True), ("feat_extract_norm", "layer")): (2822706679, 62, 103136, 1834066862, 15205072)}


@pytest.mark.parametrize("kw", list(PARENT_DRAWS))
def test_wav2vec2_draws_are_the_bits_they_were(kw):
    sd = random_state_dict(W2V2Config(**SMALL, **dict(kw)), 7)
    crcs, n = PARENT_DRAWS[kw]
    assert len(sd) == n
    assert {k: zlib.crc32(sd[k].tobytes()) for k in crcs} == crcs


@pytest.mark.parametrize("kw", list(PARENT_LAYOUT))
def test_wav2vec2_layout_blob_and_workspace_are_what_they_were(rsaf_lib, kw):
    from robust_speech_analysis_framework_amd.w2v2 import _cfg_args, pack_weights, weight_offsets
    cfg = W2V2Config(**SMALL, **dict(kw))
    offs, total = weight_offsets(cfg)
    lens = (C.c_int * 3)(80000, 32000, 400)
    ws = rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 3, *_cfg_args(cfg), cfg.flags)
    blob = pack_weights(cfg, random_state_dict(cfg, 7))
    got = (zlib.crc32(np.asarray(offs, dtype=np.int64).tobytes()), len(offs), total, zlib.crc32(blob.tobytes()), ws)
    assert got == PARENT_LAYOUT[kw]


def _offsets(lib, cfg, flags):
    from robust_speech_analysis_framework_amd.w2v2 import _cfg_args
    buf, n = (C.c_int64 * 512)(), C.c_int(0)
    assert lib.rsaf_w2v2_weight_offsets_ex(*_cfg_args(cfg), flags, buf, 512, C.byref(n)) == 0
    return [int(buf[i]) for i in range(n.value)], int(lib.rsaf_w2v2_weight_floats_ex(*_cfg_args(cfg), flags))


@pytest.mark.parametrize("conv_bias", [False, True])
def test_pack_weights_puts_the_stack_tap_major_at_the_listed_offsets(rsaf_lib, conv_bias):
    from robust_speech_analysis_framework_amd.w2v2 import _cfg_args, pack_weights, weight_offsets
    cfg = W2V2Config(**D2V_SMALL, conv_bias=conv_bias)
    sd = random_state_dict(cfg, 11)
    blob = pack_weights(cfg, sd)                                                 # its closing assert: every segment filled
    offs, total = weight_offsets(cfg)
    assert blob.shape == (total,) == (rsaf_lib.rsaf_w2v2_weight_floats_ex(*_cfg_args(cfg), cfg.flags),)
    # the same switches without the stack (a 20-tap single convolution in the slots layer 0 takes): the stack's layers
    # 1..4 are the only offsets more, {weight, bias} each, after every other segment
    plain = W2V2Config(**{**SMALL, "num_conv_pos_embeddings": 20}, feat_extract_norm="layer", conv_bias=conv_bias)
    p_offs, _ = _offsets(rsaf_lib, plain, plain.flags)
    assert len(offs) == len(p_offs) + 2 * 4 and offs[len(p_offs)] > max(offs[:len(p_offs)])
    assert offs[len(p_offs):] == sorted(offs[len(p_offs):])
    H, cg, K = 64, 16, 19
    slots = [(offs[13], offs[14])] + [(offs[len(p_offs) + 2 * (i - 1)], offs[len(p_offs) + 2 * (i - 1) + 1]) for i in range(1, 5)]
    for i, (ow, ob) in enumerate(slots):
        w = sd[f"encoder.pos_conv_embed.layers.{i}.conv.weight"]                 # [H, cg, K]
        got = blob[ow:ow + H * K * cg].reshape(H, K, cg)                         # [H][tap * cg + ci]
        assert np.array_equal(got, w.transpose(0, 2, 1)), i
        assert np.array_equal(blob[ob:ob + H], sd[f"encoder.pos_conv_embed.layers.{i}.conv.bias"]), i
    assert slots[-1][1] + H == total
    # the workspace grows by the planes and row scales of layers 1..4 only
    lens = (C.c_int * 2)(20000, 400)
    ws = rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 2, *_cfg_args(cfg), cfg.flags)
    one = W2V2Config(**{**D2V_SMALL, "num_conv_pos_embeddings": 1}, conv_bias=conv_bias)
    ws1 = rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 2, *_cfg_args(one), one.flags)
    assert ws - ws1 == 4 * 4 * (H * K * cg + H)


def test_entry_points_refuse_bad_stack_words_on_the_host(rsaf_lib):
    geom = (32, 64, 2, 4, 128)
    depth = 5 << POS_DEPTH_SHIFT
    ok = POS_CONV_STACK | LAYER_FEAT_NORM | depth
    lens = (C.c_int * 1)(8000)
    for kernel in (1, 4, 19, 64):
        assert rsaf_lib.rsaf_w2v2_weight_floats_ex(*geom, kernel, 4, ok) > 0
        assert rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 1, *geom, kernel, 4, ok) > 0
    for flags, kernel in ((POS_CONV_STACK | LAYER_FEAT_NORM, 19), (LAYER_FEAT_NORM | depth, 18), (ok | 4, 19), (ok | 64, 19),
                          (ok | 32, 19), (POS_CONV_STACK | depth, 19), (ok, 65), (ok, 0), (ok | 16, 19), (ok | 128, 19)):
        assert rsaf_lib.rsaf_w2v2_weight_floats_ex(*geom, kernel, 4, flags) == -1, (flags, kernel)
        assert rsaf_lib.rsaf_w2v2_workspace_bytes_ragged_ex(lens, 1, *geom, kernel, 4, flags) == -1, (flags, kernel)


@pytest.mark.parametrize("prefix", ["", "data2vec_audio."])
def test_local_data2vec_directory_round_trip(rsaf_lib, tmp_path, prefix):
    """save_local_model -> load_local_model, also with the prefix of the CTC / classification checkpoints; and a directory
    written by Data2VecAudioModel.save_pretrained."""
    import json
    from robust_speech_analysis_framework_amd.w2v2 import pack_weights
    cfg = W2V2Config(**D2V_SMALL, conv_bias=True, layer_norm_eps=1e-6)
    sd = random_state_dict(cfg, 5)
    mdir = tmp_path / "d2v"
    save_local_model(str(mdir), cfg, {prefix + k: v for k, v in sd.items()})
    written = json.loads((mdir / "config.json").read_text())
    assert (written["model_type"], written["conv_pos_kernel_size"], written["num_conv_pos_embeddings"]) == ("data2vec-audio", 19, 5)
    cfg2, sd2 = load_local_model(str(mdir))
    assert cfg2 == cfg and set(sd2) == set(sd) and all(np.array_equal(sd2[k], sd[k]) for k in sd)
    assert np.array_equal(pack_weights(cfg2, sd2), pack_weights(cfg, sd))
    if not prefix:
        import torch
        from transformers import Data2VecAudioModel
        m = Data2VecAudioModel(_hf_config(cfg, layer_norm_eps=1e-6))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        m.save_pretrained(str(tmp_path / "hf"))
        cfg3, sd3 = load_local_model(str(tmp_path / "hf"))
        assert cfg3 == cfg and all(np.array_equal(sd3[k], sd[k]) for k in sd)
