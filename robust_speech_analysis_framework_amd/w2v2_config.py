"""Wav2Vec2 geometry + weights for the HIP frame-embedding extractor.

The reference loads ``facebook/wav2vec2-base-960h`` by NAME through ``transformers``
(``src/foundation_model_extractor.py:70-72``).  This build never fetches: ``model_name`` must be a
local directory holding ``config.json`` and ``model.safetensors`` (HF layout), or the caller asks
for seeded random weights of the base geometry (benchmarks / parity tests).

Besides base-960h's architecture (GroupNorm feature encoder, no conv bias, post-LN encoder) the
large checkpoints' variants run too: ``feat_extract_norm="layer"``, ``conv_bias=True``,
``do_stable_layer_norm=True`` and a preprocessor with ``do_normalize=False`` (``flags``).

Two sibling families run on the same forward (``model_type`` in config.json): HuBERT, which is Wav2Vec2's arithmetic with
an optional feature-projection LayerNorm (``feat_proj_layer_norm``), and WavLM, whose attention adds a gated relative
position bias to the scores (``num_buckets``, ``max_bucket_distance``).  A third, ``data2vec-audio``, is Wav2Vec2 with the
layer-norm feature encoder, the post-LN encoder and another positional embedding: a stack of ``num_conv_pos_embeddings``
(the DEPTH, HF's naming) grouped convolutions of ``conv_pos_kernel_size`` taps, each followed by a parameter-free LayerNorm
and a GELU (``POS_CONV_STACK``).  Any other ``model_type`` is refused by name: a checkpoint whose keys merely contain
Wav2Vec2's would otherwise run without the terms it adds.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field

import numpy as np

# forward variants of rsaf_w2v2_forward_ragged_ex (include/rsaf.h)
LAYER_FEAT_NORM, CONV_BIAS, PRE_LN, NO_INPUT_NORM, NO_FEAT_PROJ_LN, REL_POS_BIAS = 1, 2, 4, 8, 32, 64
POS_CONV_STACK, POS_DEPTH_SHIFT = 256, 12         # data2vec-audio: the stack's depth (1..15) travels in flags bits 12..15
MAX_HIDDEN = 1024                  # LayerNorm runs one wave per row
REL_SPAN = 1024                    # RSAF_W2V2_REL_SPAN: the packed distance table covers |k - q| < REL_SPAN, clamped beyond
MODEL_TYPES = ("wav2vec2", "hubert", "wavlm", "data2vec-audio")
D2V = "data2vec-audio"


@dataclass
class W2V2Config:
    conv_dim: tuple = (512,) * 7
    conv_kernel: tuple = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: tuple = (5, 2, 2, 2, 2, 2, 2)
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    layer_norm_eps: float = 1e-5
    feat_extract_norm: str = "group"           # "group" (base) or "layer" (large-lv60, XLSR)
    conv_bias: bool = False
    do_stable_layer_norm: bool = False         # pre-LN encoder
    do_normalize: bool = True                  # preprocessor_config.json: zero-mean / unit-variance windows
    model_type: str = "wav2vec2"               # "wav2vec2", "hubert", "wavlm" or "data2vec-audio"
    feat_proj_layer_norm: bool = True          # hubert: False = no LayerNorm before the feature projection
    num_buckets: int = 320                     # wavlm: rows of rel_attn_embed
    max_bucket_distance: int = 800             # wavlm: bucket() is constant from this distance on
    conv_pos_kernel_size: int = 19             # data2vec-audio: taps of every convolution of the positional stack, whose
                                               # depth is num_conv_pos_embeddings (other families: the taps of their one conv)
    extras: dict = field(default_factory=dict)

    @property
    def head_dim(self):
        return self.hidden_size // self.num_attention_heads

    @property
    def flags(self) -> int:
        """The RSAF_W2V2_* bits of this architecture (0 for base-960h's)."""
        return ((LAYER_FEAT_NORM if self.feat_extract_norm == "layer" else 0) | (CONV_BIAS if self.conv_bias else 0)
                | (PRE_LN if self.do_stable_layer_norm else 0) | (0 if self.do_normalize else NO_INPUT_NORM)
                | (0 if self.feat_proj_layer_norm else NO_FEAT_PROJ_LN) | (REL_POS_BIAS if self.model_type == "wavlm" else 0)
                | ((POS_CONV_STACK | self.num_conv_pos_embeddings << POS_DEPTH_SHIFT) if self.model_type == D2V else 0))

    @property
    def pos_kernel(self) -> int:
        """Taps of a positional convolution (the ``pos_kernel`` argument of the C entry points)."""
        return self.conv_pos_kernel_size if self.model_type == D2V else self.num_conv_pos_embeddings

    def frames(self, n_samples: int) -> int:
        """Feature-encoder output length (transformers ``_get_feat_extract_output_lengths``)."""
        n = int(n_samples)
        for k, s in zip(self.conv_kernel, self.conv_stride):
            n = (n - k) // s + 1
            if n <= 0:
                return 0
        return n

    def validate(self):
        c = self.conv_dim
        if len(c) != 7 or len(set(c)) != 1 or tuple(self.conv_kernel) != (10, 3, 3, 3, 3, 2, 2) \
                or tuple(self.conv_stride) != (5, 2, 2, 2, 2, 2, 2):
            raise ValueError("only the wav2vec2 7-layer feature encoder (k 10,3,3,3,3,2,2 / s 5,2,2,2,2,2,2, "
                             "uniform width) is implemented")
        if c[0] % 32 or self.hidden_size % 4 or self.intermediate_size % 4:
            raise ValueError("conv_dim must be a multiple of 32; hidden/intermediate multiples of 4")
        if self.hidden_size > MAX_HIDDEN or c[0] > MAX_HIDDEN:
            raise ValueError(f"hidden_size / conv_dim above {MAX_HIDDEN} are not supported (LayerNorm runs one wave per row; "
                             "XLS-R 1B / 2B are out of scope)")
        if self.feat_extract_norm not in ("group", "layer"):
            raise ValueError(f"feat_extract_norm={self.feat_extract_norm!r} is not supported (need 'group' or 'layer')")
        if self.hidden_size % self.num_attention_heads or self.head_dim % 4:
            raise ValueError("head_dim must be a multiple of 4")
        if self.model_type not in MODEL_TYPES:
            raise ValueError(f"model_type={self.model_type!r} is not supported (need one of {MODEL_TYPES})")
        if not self.feat_proj_layer_norm and (self.model_type != "hubert" or self.feat_extract_norm == "layer"):
            raise ValueError("feat_proj_layer_norm=False is built for hubert with feat_extract_norm='group' only")
        if self.model_type == "wavlm":
            if self.num_buckets < 4 or self.num_buckets % 4:
                raise ValueError(f"num_buckets={self.num_buckets} must be a positive multiple of 4")
            if not self.num_buckets // 4 < self.max_bucket_distance < REL_SPAN:
                raise ValueError(f"max_bucket_distance={self.max_bucket_distance} must lie in (num_buckets / 4, {REL_SPAN}): "
                                 f"the packed distance table covers |k - q| < {REL_SPAN}")
        g = self.num_conv_pos_embedding_groups
        if self.hidden_size % g or (self.hidden_size // g) % 4:
            raise ValueError("pos-conv: channels per group must be a multiple of 4")
        if self.model_type == D2V:
            if not 1 <= self.num_conv_pos_embeddings <= 15 or not 1 <= self.conv_pos_kernel_size <= 64:
                raise ValueError(f"{D2V}: num_conv_pos_embeddings (the stack's depth) must lie in 1..15 and "
                                 "conv_pos_kernel_size in 1..64")
            if self.feat_extract_norm != "layer" or self.do_stable_layer_norm or not self.feat_proj_layer_norm:
                raise ValueError(f"{D2V} is the layer-norm feature encoder with the post-LN encoder and the feature-projection "
                                 "LayerNorm (feat_extract_norm='layer', do_stable_layer_norm=False, feat_proj_layer_norm=True)")
        elif self.num_conv_pos_embeddings % 2:
            raise ValueError("pos-conv: kernel even")

    @staticmethod
    def from_hf_dict(d: dict, do_normalize: bool = True) -> "W2V2Config":
        """``config.json`` of a Wav2Vec2, HuBERT or WavLM checkpoint -> config; raises for anything this build cannot run
        (any other ``model_type`` by name).  ``do_normalize``: the preprocessor's switch (``preprocessor_config.json``), not
        part of config.json."""
        model_type = d.get("model_type", "wav2vec2")
        if model_type not in MODEL_TYPES:
            raise ValueError(f"config.json: model_type={model_type!r} is not supported (need one of {MODEL_TYPES}); its "
                             "weights may load as Wav2Vec2's, its forward is another one")
        family = {}
        if model_type == "hubert":
            if d.get("conv_pos_batch_norm", False):
                raise ValueError("config.json: conv_pos_batch_norm=true is not supported")
            family["feat_proj_layer_norm"] = bool(d.get("feat_proj_layer_norm", True))
        elif model_type == "wavlm":
            family["num_buckets"] = int(d.get("num_buckets", 320))
            family["max_bucket_distance"] = int(d.get("max_bucket_distance", 800))
        elif model_type == D2V:
            # its positional embedding is a stack: num_conv_pos_embeddings convolutions of conv_pos_kernel_size taps.  A
            # Wav2Vec2 config relabelled data2vec-audio has neither the key nor a depth this build runs
            if "conv_pos_kernel_size" not in d:
                raise ValueError(f"config.json: model_type={D2V!r} needs conv_pos_kernel_size (the taps of its positional stack)")
            if not 1 <= int(d["num_conv_pos_embeddings"]) <= 15:
                raise ValueError(f"config.json: model_type={D2V!r}: num_conv_pos_embeddings={d['num_conv_pos_embeddings']!r} is "
                                 "the depth of the positional stack and must lie in 1..15")
            if not 1 <= int(d["conv_pos_kernel_size"]) <= 64:
                raise ValueError(f"config.json: model_type={D2V!r}: conv_pos_kernel_size={d['conv_pos_kernel_size']!r} must lie "
                                 "in 1..64")
            family["conv_pos_kernel_size"] = int(d["conv_pos_kernel_size"])
        tag = f"model_type={D2V!r}: " if model_type == D2V else ""
        for key, want in (("feat_extract_activation", "gelu"), ("hidden_act", "gelu")):
            if d.get(key, want) != want:
                raise ValueError(f"config.json: {tag}{key}={d.get(key)!r} is not supported (need {want!r})")
        if model_type != D2V and d.get("feat_extract_norm", "group") not in ("group", "layer"):
            raise ValueError(f"config.json: feat_extract_norm={d.get('feat_extract_norm')!r} is not supported "
                             "(need 'group' or 'layer')")
        if d.get("add_adapter") or d.get("adapter_attn_dim"):
            raise ValueError(f"config.json: {tag}adapters (add_adapter / adapter_attn_dim) are not supported")
        for key in ("hidden_size", "conv_dim"):
            v = max(d[key]) if isinstance(d.get(key), list) else d.get(key, 0)
            if v > MAX_HIDDEN:
                raise ValueError(f"config.json: {tag}{key}={d[key]!r} is above {MAX_HIDDEN}, which this build does not support "
                                 "(LayerNorm runs one wave per row; XLS-R 1B / 2B are out of scope)")
        return W2V2Config(conv_dim=tuple(d["conv_dim"]), conv_kernel=tuple(d["conv_kernel"]),
                          conv_stride=tuple(d["conv_stride"]), hidden_size=d["hidden_size"],
                          num_hidden_layers=d["num_hidden_layers"], num_attention_heads=d["num_attention_heads"],
                          intermediate_size=d["intermediate_size"],
                          num_conv_pos_embeddings=d["num_conv_pos_embeddings"],
                          num_conv_pos_embedding_groups=d["num_conv_pos_embedding_groups"],
                          layer_norm_eps=d.get("layer_norm_eps", 1e-5),
                          # transformers' Data2VecAudioModel ignores both switches: always layer norm + post-LN
                          feat_extract_norm="layer" if model_type == D2V else d.get("feat_extract_norm", "group"),
                          conv_bias=bool(d.get("conv_bias", False)),
                          do_stable_layer_norm=model_type != D2V and bool(d.get("do_stable_layer_norm", False)),
                          do_normalize=bool(do_normalize), model_type=model_type, **family)


def hf_shapes(cfg: W2V2Config) -> dict:
    """state_dict keys/shapes of ``transformers.Wav2Vec2Model`` (``HubertModel``, ``WavLMModel``, ``Data2VecAudioModel``) for
    this geometry."""
    sh = {}
    cin = 1
    for i, (c, k) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel)):
        sh[f"feature_extractor.conv_layers.{i}.conv.weight"] = (c, cin, k)
        cin = c
    sh["feature_extractor.conv_layers.0.layer_norm.weight"] = (cfg.conv_dim[0],)
    sh["feature_extractor.conv_layers.0.layer_norm.bias"] = (cfg.conv_dim[0],)
    # the variants' keys come after layer 0's norm: the key order (and so the draws of random_state_dict) of the base
    # architecture stays what it was
    if cfg.feat_extract_norm == "layer":                     # layer 0's key is its LayerNorm; layers 1..6 have one too
        for i in range(1, 7):
            sh[f"feature_extractor.conv_layers.{i}.layer_norm.weight"] = (cfg.conv_dim[i],)
            sh[f"feature_extractor.conv_layers.{i}.layer_norm.bias"] = (cfg.conv_dim[i],)
    if cfg.conv_bias:
        for i in range(7):
            sh[f"feature_extractor.conv_layers.{i}.conv.bias"] = (cfg.conv_dim[i],)
    Hd, Cc = cfg.hidden_size, cfg.conv_dim[-1]
    if cfg.feat_proj_layer_norm:
        sh["feature_projection.layer_norm.weight"] = (Cc,)
        sh["feature_projection.layer_norm.bias"] = (Cc,)
    sh["feature_projection.projection.weight"] = (Hd, Cc)
    sh["feature_projection.projection.bias"] = (Hd,)
    K, G = cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups
    if cfg.model_type != D2V:
        sh["encoder.pos_conv_embed.conv.bias"] = (Hd,)
        sh["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = (1, 1, K)
        sh["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = (Hd, Hd // G, K)
    sh["encoder.layer_norm.weight"] = (Hd,)
    sh["encoder.layer_norm.bias"] = (Hd,)
    for l in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sh[p + f"attention.{n}.weight"] = (Hd, Hd)
            sh[p + f"attention.{n}.bias"] = (Hd,)
        sh[p + "layer_norm.weight"] = (Hd,)
        sh[p + "layer_norm.bias"] = (Hd,)
        sh[p + "feed_forward.intermediate_dense.weight"] = (cfg.intermediate_size, Hd)
        sh[p + "feed_forward.intermediate_dense.bias"] = (cfg.intermediate_size,)
        sh[p + "feed_forward.output_dense.weight"] = (Hd, cfg.intermediate_size)
        sh[p + "feed_forward.output_dense.bias"] = (Hd,)
        sh[p + "final_layer_norm.weight"] = (Hd,)
        sh[p + "final_layer_norm.bias"] = (Hd,)
    # WavLM's keys come last: the draws of random_state_dict for the keys above stay what they were
    if cfg.model_type == "wavlm":
        for l in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{l}.attention."
            sh[p + "gru_rel_pos_const"] = (1, cfg.num_attention_heads, 1, 1)
            sh[p + "gru_rel_pos_linear.weight"] = (8, cfg.head_dim)
            sh[p + "gru_rel_pos_linear.bias"] = (8,)
        sh["encoder.layers.0.attention.rel_attn_embed.weight"] = (cfg.num_buckets, cfg.num_attention_heads)
    # data2vec-audio's positional stack comes last too (K = the depth here)
    if cfg.model_type == D2V:
        for i in range(K):
            sh[f"encoder.pos_conv_embed.layers.{i}.conv.weight"] = (Hd, Hd // G, cfg.conv_pos_kernel_size)
            sh[f"encoder.pos_conv_embed.layers.{i}.conv.bias"] = (Hd,)
    return sh


def relative_position_table(cfg: W2V2Config, rel_attn_embed) -> np.ndarray:
    """[heads, 2 REL_SPAN - 1] float32: entry [h, d + REL_SPAN - 1] = rel_attn_embed[bucket(d), h], d = key - query.  The
    buckets come from the torch operations of ``WavLMAttention._relative_positions_bucket`` in their order (a float32
    ``log``, two float32 scalings, a truncation): one ulp at a bucket edge would swap a whole embedding row."""
    import math

    import torch
    d = torch.arange(-(REL_SPAN - 1), REL_SPAN, dtype=torch.long)
    num_buckets = cfg.num_buckets // 2
    buckets = (d > 0).to(torch.long) * num_buckets
    d = torch.abs(d)
    max_exact = num_buckets // 2
    is_small = d < max_exact
    large = torch.log(d.float() / max_exact)
    large = large / math.log(cfg.max_bucket_distance / max_exact)
    large = large * (num_buckets - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    buckets += torch.where(is_small, d, large)
    emb = np.asarray(rel_attn_embed, dtype=np.float32)
    return np.ascontiguousarray(emb[buckets.numpy()].T)


def random_state_dict(cfg: W2V2Config, seed: int = 0) -> dict:
    """Seeded random weights (numpy PCG64; no torch RNG) in the HF key layout.  Scales keep every
    stage O(1) so parity errors are not hidden by vanishing activations."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for k, shape in hf_shapes(cfg).items():
        if k.endswith("layer_norm.weight"):
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif "gru_rel_pos" in k or "rel_attn_embed" in k:       # O(1): the gated bias moves the scores
            v = rng.standard_normal(shape)
        elif k.endswith("bias"):
            v = 0.05 * rng.standard_normal(shape)
        elif k.endswith("original0"):
            v = 1.0 + 0.2 * rng.random(shape)
        elif k.endswith("original1"):
            v = rng.standard_normal(shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = np.sqrt(2.0) if "conv_layers" in k else 1.0
            v = gain * rng.standard_normal(shape) / np.sqrt(fan_in)
        sd[k] = v.astype(np.float32)
    return sd


def _strip_prefix(sd: dict) -> dict:
    """base-960h is a Wav2Vec2ForCTC checkpoint: keys carry a ``wav2vec2.`` prefix (``hubert.`` / ``wavlm.`` / ``data2vec_audio.`` in those
    families' CTC and classification checkpoints); ``lm_head`` is unused.  The heads of Wav2Vec2ForPreTraining checkpoints
    (XLSR-53, XLS-R: ``quantizer``, ``project_q``, ``project_hid``) are unused too."""
    out = {}
    for k, v in sd.items():
        for prefix in ("wav2vec2.", "hubert.", "wavlm.", "data2vec_audio."):
            if k.startswith(prefix):
                k = k[len(prefix):]
                break
        if k.startswith(("lm_head", "quantizer.", "project_q.", "project_hid.")) or k == "masked_spec_embed":
            continue
        k = k.replace("pos_conv_embed.conv.weight_g", "pos_conv_embed.conv.parametrizations.weight.original0")
        k = k.replace("pos_conv_embed.conv.weight_v", "pos_conv_embed.conv.parametrizations.weight.original1")
        out[k] = np.asarray(v, dtype=np.float32)
    return out


def load_local_model(model_dir: str):
    """(config, state_dict) from a LOCAL HF directory.  Raises for anything that is not a local path.
    ``do_normalize`` comes from ``preprocessor_config.json`` when the directory has one (default True)."""
    if not os.path.isdir(model_dir):
        raise FileNotFoundError(
            f"'{model_dir}' is not a local directory; this build never downloads models "
            "(pass a directory with config.json + model.safetensors)")
    do_normalize = True
    pp = os.path.join(model_dir, "preprocessor_config.json")
    if os.path.exists(pp):
        with open(pp) as f:
            do_normalize = bool(json.load(f).get("do_normalize", True))
    with open(os.path.join(model_dir, "config.json")) as f:
        cfg = W2V2Config.from_hf_dict(json.load(f), do_normalize=do_normalize)
    st = os.path.join(model_dir, "model.safetensors")
    if os.path.exists(st):
        from safetensors.numpy import load_file
        sd = load_file(st)
    else:
        import torch
        sd = {k: v.numpy() for k, v in torch.load(os.path.join(model_dir, "pytorch_model.bin"),
                                                  map_location="cpu", weights_only=True).items()}
    sd = _strip_prefix(sd)
    missing = set(hf_shapes(cfg)) - set(sd)
    if missing:
        raise KeyError(f"checkpoint lacks {sorted(missing)[:4]} ...")
    return cfg, sd


def save_local_model(model_dir: str, cfg: W2V2Config, sd: dict):
    """Write config.json + model.safetensors (used by tests to exercise the local-directory loader), and a
    preprocessor_config.json when ``cfg.do_normalize`` is False."""
    from safetensors.numpy import save_file
    os.makedirs(model_dir, exist_ok=True)
    d = {"conv_dim": list(cfg.conv_dim), "conv_kernel": list(cfg.conv_kernel), "conv_stride": list(cfg.conv_stride),
         "hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.num_hidden_layers,
         "num_attention_heads": cfg.num_attention_heads, "intermediate_size": cfg.intermediate_size,
         "num_conv_pos_embeddings": cfg.num_conv_pos_embeddings,
         "num_conv_pos_embedding_groups": cfg.num_conv_pos_embedding_groups,
         "layer_norm_eps": cfg.layer_norm_eps, "feat_extract_norm": cfg.feat_extract_norm, "feat_extract_activation": "gelu",
         "hidden_act": "gelu", "do_stable_layer_norm": bool(cfg.do_stable_layer_norm), "conv_bias": bool(cfg.conv_bias),
         "model_type": "wav2vec2"}
    if cfg.model_type == "hubert":
        d.update(model_type="hubert", feat_proj_layer_norm=bool(cfg.feat_proj_layer_norm))
    elif cfg.model_type == "wavlm":
        d.update(model_type="wavlm", num_buckets=cfg.num_buckets, max_bucket_distance=cfg.max_bucket_distance)
    elif cfg.model_type == D2V:                              # num_conv_pos_embeddings above is the stack's depth
        d.update(model_type=D2V, conv_pos_kernel_size=cfg.conv_pos_kernel_size)
    with open(os.path.join(model_dir, "config.json"), "w") as f:
        json.dump(d, f)
    if not cfg.do_normalize:
        with open(os.path.join(model_dir, "preprocessor_config.json"), "w") as f:
            json.dump({"do_normalize": False, "feature_size": 1, "padding_side": "right", "padding_value": 0.0,
                       "return_attention_mask": True, "sampling_rate": SAMPLE_RATE,
                       "feature_extractor_type": "Wav2Vec2FeatureExtractor"}, f)
    save_file({k: np.ascontiguousarray(v) for k, v in sd.items()}, os.path.join(model_dir, "model.safetensors"))


# ---- chunking contract of the reference (integer-exact) -------------------------------------------
SAMPLE_RATE = 16000


def chunk_plan(n_samples: int, chunk_seconds=5, overlap_seconds=1, sample_rate: int = SAMPLE_RATE):
    """[(start, length)] exactly as ``src/foundation_model_extractor.py:97-108``: windows of
    ``chunk_seconds`` every ``chunk_seconds - overlap_seconds``; a window shorter than 0.5 s is dropped."""
    chunk = int(sample_rate * chunk_seconds)
    step = int(sample_rate * (chunk_seconds - overlap_seconds))
    if step <= 0:
        raise ValueError("range() arg 3 must not be zero" if step == 0 else "step must be positive")
    min_len = int(sample_rate * 0.5)
    plan = []
    for i in range(0, int(n_samples), step):
        ln = min(chunk, int(n_samples) - i)
        if ln < min_len:
            continue
        plan.append((i, ln))
    return plan
