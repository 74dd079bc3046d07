"""Wav2Vec2 frame-embedding extractor on the HIP path (drop-in for
``src/foundation_model_extractor.py``).

The reference walks each file in 5 s windows every 4 s, normalises every window on its own, runs
``Wav2Vec2Model`` at batch 1 and stacks the window outputs (``:97-125``).  Here all windows of all
clips of a batch are planned with the same integer arithmetic, grouped by length and pushed through
``rsaf_w2v2_forward`` in large sub-batches; the final LayerNorm writes each window's frames straight
to its ``np.vstack`` position, so the values per window are those of the batch-1 reference.

``output_layers`` selects transformers' ``hidden_states`` (``output_hidden_states=True``) instead of ``last_hidden_state``:
the LayerNorm launches of the same forward copy them out (``rsaf_w2v2_forward_ragged_hidden``), and the pooled embeddings
are averaged on the device (``rsaf_rows_segment_mean_f32``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from .w2v2_config import (SAMPLE_RATE, W2V2Config, chunk_plan, load_local_model, random_state_dict,
                          relative_position_table)
from .wavio import read_wav_mono_device

_KERNELS = (10, 3, 3, 3, 3, 2, 2)
# Device bytes of hidden-state planes per forward call of the drop-ins (n_sel x frames x hidden x 4): a file batch whose
# planes would exceed it runs as several groups of whole files.  64 files x 30 s with all 13 base states take 4.9 GB.
HIDDEN_TAP_BUDGET_BYTES = 8 << 30


def layer_selection(output_layers, num_layers=None):
    """Validate ``output_layers`` (an int, or a non-empty list / tuple of ints) against ``num_layers`` encoder layers
    (``num_layers + 1`` hidden states; Python-style negatives, -1 = the last).  Returns ``(layers, unique, pos)``: the
    requested indices made non-negative in the requested order, the strictly increasing distinct ones the forward taps,
    and for every requested index its position in ``unique``.  With ``num_layers=None`` only the types are checked."""
    items = [output_layers] if isinstance(output_layers, (int, np.integer)) else output_layers
    if not isinstance(items, (list, tuple)) or not items or \
            any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) for k in items):
        raise ValueError(f"output_layers must be an int or a non-empty list / tuple of ints, not {output_layers!r}")
    if num_layers is None:
        return None
    n = num_layers + 1
    bad = [int(k) for k in items if not -n <= k < n]
    if bad:
        raise ValueError(f"output_layers {bad} out of range: this model has hidden states 0..{num_layers} (or -{n}..-1)")
    layers = [int(k) % n for k in items]
    unique = sorted(set(layers))
    return layers, unique, [unique.index(k) for k in layers]


def _cfg_args(cfg: W2V2Config):
    return (cfg.conv_dim[0], cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads,
            cfg.intermediate_size, cfg.pos_kernel, cfg.num_conv_pos_embedding_groups)


def weight_offsets(cfg: W2V2Config):
    lib = _lib.load()
    cap = 32 + 21 + 16 * cfg.num_hidden_layers + 1 + 2 * 15
    buf = (C.c_int64 * cap)()
    n = C.c_int(0)
    _lib.check(lib.rsaf_w2v2_weight_offsets_ex(*_cfg_args(cfg), cfg.flags, buf, cap, C.byref(n)), "rsaf_w2v2_weight_offsets_ex")
    return [int(buf[i]) for i in range(n.value)], int(lib.rsaf_w2v2_weight_floats_ex(*_cfg_args(cfg), cfg.flags))


def pack_weights(cfg: W2V2Config, sd: dict) -> np.ndarray:
    """HF-keyed state_dict -> the float32 blob of ``rsaf_w2v2_forward_ragged_ex`` (weight norm folded,
    conv kernels tap-major, q/k/v fused; conv biases, conv LayerNorms, WavLM's summed gate rows and its distance table,
    data2vec-audio's positional stack from its second layer on appended per ``cfg.flags``)."""
    cfg.validate()
    offs, total = weight_offsets(cfg)
    blob = np.zeros(total, dtype=np.float32)
    it = iter(offs)

    def put(a):
        o = next(it)
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        blob[o:o + a.size] = a.astype(np.float32)

    g = lambda k: np.asarray(sd[k], dtype=np.float64)                               # noqa: E731
    layer = cfg.feat_extract_norm == "layer"
    put(g("feature_extractor.conv_layers.0.conv.weight")[:, 0, :])
    # GroupNorm slots (layer mode: unused, left zero; layer 0's LayerNorm goes to the appended segment)
    put(0.0 * g("feature_extractor.conv_layers.0.layer_norm.weight") if layer else g("feature_extractor.conv_layers.0.layer_norm.weight"))
    put(0.0 * g("feature_extractor.conv_layers.0.layer_norm.bias") if layer else g("feature_extractor.conv_layers.0.layer_norm.bias"))
    for i in range(1, 7):
        w = g(f"feature_extractor.conv_layers.{i}.conv.weight")                  # [Cout, Cin, k]
        put(np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(w.shape[0], -1))
    if cfg.feat_proj_layer_norm:
        put(g("feature_projection.layer_norm.weight")); put(g("feature_projection.layer_norm.bias"))
    else:                                                    # NO_FEAT_PROJ_LN: the two slots stay, unused
        put(np.zeros(cfg.conv_dim[-1])); put(np.zeros(cfg.conv_dim[-1]))
    put(g("feature_projection.projection.weight")); put(g("feature_projection.projection.bias"))
    stack = cfg.model_type == "data2vec-audio"               # layer 0 of its positional stack takes the single conv's slots
    if stack:
        w = g("encoder.pos_conv_embed.layers.0.conv.weight")                     # [H, H/G, K], no weight norm
    else:
        wg = g("encoder.pos_conv_embed.conv.parametrizations.weight.original0")  # [1,1,K]
        wv = g("encoder.pos_conv_embed.conv.parametrizations.weight.original1")  # [H, H/G, K]
        w = wg * wv / np.sqrt((wv * wv).sum(axis=(0, 1), keepdims=True))         # weight_norm(dim=2)
    put(np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(w.shape[0], -1))      # [H][tap*cg + ci] = [G][cg][...]
    put(g("encoder.pos_conv_embed.layers.0.conv.bias" if stack else "encoder.pos_conv_embed.conv.bias"))
    put(g("encoder.layer_norm.weight")); put(g("encoder.layer_norm.bias"))
    for l in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{l}."
        put(np.concatenate([g(p + f"attention.{n}.weight") for n in ("q_proj", "k_proj", "v_proj")], axis=0))
        put(np.concatenate([g(p + f"attention.{n}.bias") for n in ("q_proj", "k_proj", "v_proj")]))
        put(g(p + "attention.out_proj.weight")); put(g(p + "attention.out_proj.bias"))
        put(g(p + "layer_norm.weight")); put(g(p + "layer_norm.bias"))
        put(g(p + "feed_forward.intermediate_dense.weight")); put(g(p + "feed_forward.intermediate_dense.bias"))
        put(g(p + "feed_forward.output_dense.weight")); put(g(p + "feed_forward.output_dense.bias"))
        put(g(p + "final_layer_norm.weight")); put(g(p + "final_layer_norm.bias"))
    if cfg.conv_bias:
        for i in range(7):
            put(g(f"feature_extractor.conv_layers.{i}.conv.bias"))
    if layer:
        for i in range(7):
            put(g(f"feature_extractor.conv_layers.{i}.layer_norm.weight")); put(g(f"feature_extractor.conv_layers.{i}.layer_norm.bias"))
    if cfg.model_type == "wavlm":
        # the gate's 8 outputs are summed in two groups of 4 before the sigmoids: sum the weight rows (float64) instead
        for l in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{l}.attention."
            w, b = g(p + "gru_rel_pos_linear.weight"), g(p + "gru_rel_pos_linear.bias")
            put(w[:4].sum(axis=0)); put(w[4:].sum(axis=0))
            put(np.array([b[:4].sum(), b[4:].sum()]))
            put(g(p + "gru_rel_pos_const"))
        put(relative_position_table(cfg, sd["encoder.layers.0.attention.rel_attn_embed.weight"]))
    if stack:                                                # layers 1..D-1, tap-major like layer 0
        for i in range(1, cfg.num_conv_pos_embeddings):
            w = g(f"encoder.pos_conv_embed.layers.{i}.conv.weight")
            put(np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(w.shape[0], -1))
            put(g(f"encoder.pos_conv_embed.layers.{i}.conv.bias"))
    assert next(it, None) is None, "weight layout has segments pack_weights does not fill"
    return blob


class W2V2Engine:
    """Device-resident Wav2Vec2 weights + workspace; runs batches of windows through the HIP path."""

    def __init__(self, cfg: W2V2Config, sd: dict, device="cuda", max_chunks_per_call: int = 256):
        import torch
        _lib.load()
        _lib.require_gpu()
        self.cfg = cfg
        self.device = torch.device(device)
        self.blob = torch.from_numpy(pack_weights(cfg, sd)).to(self.device)
        lim = 65535 // max(cfg.num_attention_heads, cfg.num_conv_pos_embedding_groups)
        self.max_chunks = max(1, min(max_chunks_per_call, lim))
        self._ws = None
        self._keep = None

    def _workspace(self, lens_c, n):
        import torch
        need = _lib.load().rsaf_w2v2_workspace_bytes_ragged_ex(lens_c, n, *_cfg_args(self.cfg), self.cfg.flags)
        if need < 0:
            raise _lib.RsafError("a window is shorter than the encoder's receptive field (or the lengths are not non-increasing)")
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = None
            self._ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=self.device)
        return self._ws

    def forward_windows(self, wav, starts, lens, out, out_rows, stream=None, hidden=None):
        """wav: 1-D float32 device tensor; starts / lens / out_rows: host arrays (sample offset and length of each window in
        ``wav``; first output row of each window in ``out`` [rows, hidden]).  Windows of any mix of lengths run together
        (``rsaf_w2v2_forward_ragged``, or its ``_ex`` form with the config's flags): they are ordered by length here, longest first, and cut into balanced sub-batches.

        hidden: strictly increasing hidden-state indices in [0, num_hidden_layers]; then the call returns ``(out, planes)``,
        planes [len(hidden), rows of out, hidden_size] holding ``hidden_states[hidden[j]]`` in the row layout of ``out``."""
        import torch
        lib = _lib.load()
        cfg = self.cfg
        starts = np.asarray(starts, dtype=np.int64)
        lens = np.asarray(lens, dtype=np.int32)
        out_rows = np.asarray(out_rows, dtype=np.int64)
        n_total = len(starts)
        planes = None
        if hidden is not None:
            hidden = [int(k) for k in hidden]
            if not hidden or any(not 0 <= k <= cfg.num_hidden_layers for k in hidden) or \
                    any(b <= a for a, b in zip(hidden, hidden[1:])):
                raise ValueError(f"hidden must be strictly increasing indices in [0, {cfg.num_hidden_layers}], not {hidden}")
            planes = torch.empty((len(hidden), out.shape[0], cfg.hidden_size), dtype=torch.float32, device=self.device)
            hidden_c = (C.c_int * len(hidden))(*hidden)
        if n_total == 0:
            return out if planes is None else (out, planes)
        order = np.argsort(-lens.astype(np.int64), kind="stable")
        starts, lens, out_rows = starts[order], lens[order], out_rows[order]
        # balanced sub-batches: ceil(n / max) calls of (almost) equal size instead of full ones and a remainder (7 000 windows
        # with a maximum of 2 048: 4 x 1 750, whose GEMM tile counts fill the 256 CUs to 99.8 % where 2 048 left the last round
        # of every N = 768 GEMM a third full)
        n_calls = max(1, -(-n_total // self.max_chunks))
        per = max(1, -(-n_total // n_calls))
        per = min(self.max_chunks, (per + 3) & ~3)
        # one pinned staging buffer per call for the three small tables, queued on the current stream (no host wait)
        for b0 in range(0, n_total, per):
            n = min(per, n_total - b0)
            host = torch.empty(5 * n, dtype=torch.int32).pin_memory()          # starts (int64) | out rows (int64) | lengths (int32)
            hv = host.numpy()
            hv[:2 * n].view(np.int64)[:] = starts[b0:b0 + n]
            hv[2 * n:4 * n].view(np.int64)[:] = out_rows[b0:b0 + n]
            hv[4 * n:] = lens[b0:b0 + n]
            dev = host.to(self.device, non_blocking=True)
            lens_c = (C.c_int * n)(*[int(v) for v in lens[b0:b0 + n]])
            ws = self._workspace(lens_c, n)
            head = (_lib.ptr(wav), C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr() + 16 * n), lens_c, n, *_cfg_args(cfg),
                    float(cfg.layer_norm_eps))
            tail = (_lib.ptr(self.blob), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(out), C.c_void_p(dev.data_ptr() + 8 * n),
                    _lib.stream_ptr(stream))
            if planes is not None:                                             # + the hidden-state taps
                _lib.check(lib.rsaf_w2v2_forward_ragged_hidden(*head, cfg.flags, *tail[:-1], hidden_c, len(hidden), _lib.ptr(planes),
                                                                out.shape[0] * cfg.hidden_size, tail[-1]),
                           "rsaf_w2v2_forward_ragged_hidden")
            elif cfg.flags:                                                    # the large checkpoints' variants
                _lib.check(lib.rsaf_w2v2_forward_ragged_ex(*head, cfg.flags, *tail), "rsaf_w2v2_forward_ragged_ex")
            else:                                                              # base architecture (= _ex with flags 0)
                _lib.check(lib.rsaf_w2v2_forward_ragged(*head, *tail), "rsaf_w2v2_forward_ragged")
            self._keep = (host, dev)                                           # alive until the next call's copy is queued
        return out if planes is None else (out, planes)

    def plan(self, lengths, chunk_seconds=5, overlap_seconds=1):
        """Integer-exact window plan of a batch: per clip [(start, len, frames)] + total frames."""
        per_clip, totals = [], []
        for n in lengths:
            pl = [(s, l, self.cfg.frames(l)) for s, l in chunk_plan(n, chunk_seconds, overlap_seconds)]
            per_clip.append(pl)
            totals.append(sum(f for _, _, f in pl))
        return per_clip, totals

    def extract_packed(self, wav, clip_offsets, lengths, chunk_seconds=5, overlap_seconds=1, stream=None, layers=None):
        """All clips of a packed batch -> (out [sum frames, hidden] device tensor, frame offsets).

        wav: 1-D float32 device tensor holding the clips back to back; clip c = samples
        [clip_offsets[c], clip_offsets[c] + lengths[c]).
        layers: strictly increasing hidden-state indices; then the result is (out, frame offsets, planes) with planes
        [len(layers), sum frames, hidden] (``forward_windows``' ``hidden``)."""
        import torch
        per_clip, totals = self.plan(lengths, chunk_seconds, overlap_seconds)
        frame_off = np.zeros(len(lengths) + 1, dtype=np.int64)
        frame_off[1:] = np.cumsum(totals)
        out = torch.empty((max(int(frame_off[-1]), 1), self.cfg.hidden_size), dtype=torch.float32, device=self.device)
        starts, lens, rows = [], [], []
        for c, pl in enumerate(per_clip):
            row = int(frame_off[c])
            for s, l, f in pl:
                starts.append(int(clip_offsets[c]) + s)
                lens.append(l)
                rows.append(row)
                row += f
        if layers is None:
            self.forward_windows(wav, starts, lens, out, rows, stream)
            return out[:int(frame_off[-1])], frame_off
        _, planes = self.forward_windows(wav, starts, lens, out, rows, stream, hidden=layers)
        return out[:int(frame_off[-1])], frame_off, planes[:, :int(frame_off[-1])]

    def pooled_hidden(self, wav, clip_offsets, lengths, layers, chunk_seconds=5, overlap_seconds=1, stream=None):
        """Time mean per clip of the hidden states ``layers`` (strictly increasing) -> (means [len(layers), clips, hidden]
        device tensor, frame offsets); a clip without frames gets NaN.  The planes never leave the device: one
        ``rsaf_rows_segment_mean_f32`` launch pools all of them (fp64 sums in frame order)."""
        import torch
        _, frame_off, planes = self.extract_packed(wav, clip_offsets, lengths, chunk_seconds, overlap_seconds, stream, layers)
        H = self.cfg.hidden_size
        means = torch.empty((len(layers), len(lengths), H), dtype=torch.float32, device=self.device)
        seg = torch.from_numpy(frame_off).to(self.device)
        _lib.check(_lib.load().rsaf_rows_segment_mean_f32(_lib.ptr(planes), H, planes.shape[1] * H, len(layers), _lib.ptr(seg),
                                                          len(lengths), H, _lib.ptr(means), _lib.stream_ptr(stream)),
                   "rsaf_rows_segment_mean_f32")
        return means, frame_off

    def file_groups(self, lengths, n_planes, chunk_seconds=5, overlap_seconds=1, budget=None):
        """Split clips (by index) into runs of consecutive clips whose ``n_planes`` hidden-state planes fit the device
        budget (``HIDDEN_TAP_BUDGET_BYTES``); a clip larger than the budget runs alone."""
        budget = HIDDEN_TAP_BUDGET_BYTES if budget is None else budget
        _, totals = self.plan(lengths, chunk_seconds, overlap_seconds)
        per_frame = n_planes * self.cfg.hidden_size * 4
        groups, cur, used = [], [], 0
        for i, f in enumerate(totals):
            if cur and used + f * per_frame > budget:
                groups.append(cur)
                cur, used = [], 0
            cur.append(i)
            used += f * per_frame
        if cur:
            groups.append(cur)
        return groups


_ENGINES = {}


def _resolve_model(model_name):
    """(cfg, state_dict): a local HF directory, or seeded random base weights when the caller sets
    RSAF_W2V2_RANDOM_SEED (benchmarks / parity tests).  Never fetches."""
    seed = os.environ.get("RSAF_W2V2_RANDOM_SEED")
    if os.path.isdir(str(model_name)):
        return load_local_model(str(model_name))
    if seed is not None:
        cfg = W2V2Config()
        return cfg, random_state_dict(cfg, int(seed))
    raise FileNotFoundError(
        f"'{model_name}' is not a local model directory and this build never downloads checkpoints "
        "(no network): pass a directory holding config.json + model.safetensors")


def get_engine(model_name, device="cuda"):
    key = (str(model_name), os.environ.get("RSAF_W2V2_RANDOM_SEED"), str(device))
    if key not in _ENGINES:
        cfg, sd = _resolve_model(model_name)
        _ENGINES[key] = W2V2Engine(cfg, sd, device)
    return _ENGINES[key]


def _model_layers(model_name):
    """num_hidden_layers of the model the drop-ins would load, from its config only (None when it cannot be read: the
    model load reports that)."""
    try:
        if os.path.isdir(str(model_name)):
            import json
            with open(os.path.join(str(model_name), "config.json")) as f:
                return W2V2Config.from_hf_dict(json.load(f)).num_hidden_layers
        if os.environ.get("RSAF_W2V2_RANDOM_SEED") is not None:
            return W2V2Config().num_hidden_layers
    except Exception:
        pass
    return None


def extract_wav2vec2_sequences(input_df, model_name="facebook/wav2vec2-base-960h", audio_file_column="filepath",
                               chunk_seconds=5, overlap_seconds=1, verbose=True, batch_files=64, output_layers=None):
    """Drop-in for ``src/foundation_model_extractor.py:37-131``: dict basename -> float32 [T, hidden_size] (768 for base,
    1024 for the large / XLS-R checkpoints).

    Files shorter than 0.5 s (``:88``) or failing to load are absent; a model that cannot be
    loaded gives the reference's convention ``print + {}`` (``:73-74``).

    output_layers: None (default) = ``last_hidden_state``.  An int k = transformers' ``hidden_states[k]`` (0 = the encoder
    input, num_hidden_layers = the last layer; negatives count from the end, -1 = ``last_hidden_state`` bit for bit), still
    [T, hidden_size] per file.  A list / tuple = float32 [len(output_layers), T, hidden_size] per file, in the requested
    order.  An index out of range raises ValueError before any device work."""
    return _extract(input_df, model_name, audio_file_column, chunk_seconds, overlap_seconds, verbose, batch_files,
                    output_layers, pooled=False)[0]


def _extract(input_df, model_name, audio_file_column, chunk_seconds, overlap_seconds, verbose, batch_files, output_layers,
             pooled):
    """The drop-ins' file loop -> ({basename: result}, layer_selection(...) or None).  pooled=False: per file the frames
    ([T, H], or [n_sel, T, H] for a list of layers); pooled=True (output_layers given): per file the time means ([H], or
    [n_sel, H]), averaged on the device."""
    import torch
    sel = None
    if output_layers is not None:
        layer_selection(output_layers)                                     # the types, before anything else
        n_layers = _model_layers(model_name)
        if n_layers is not None:
            sel = layer_selection(output_layers, n_layers)
    device = "cuda" if torch.cuda.is_available() else "cpu"
    if verbose:
        print(f"Using device: {device}")
    try:
        _lib.load()
        _lib.require_gpu()
        eng = get_engine(model_name, device)
    except Exception as e:
        print(f"Error loading model '{model_name}': {e}")
        return {}, sel
    if output_layers is not None:
        sel = layer_selection(output_layers, eng.cfg.num_hidden_layers)
    sequences = {}
    paths = list(input_df[audio_file_column])
    for b0 in range(0, len(paths), batch_files):
        clips, names = [], []
        for pth in paths[b0:b0 + batch_files]:
            filename = os.path.basename(pth)
            try:
                mono, fs, n_in = read_wav_mono_device(pth, device=eng.device)   # :87,91 decode + channel mean on the device
                if n_in < int(SAMPLE_RATE * 0.5):                             # :88 (pre-resample count)
                    if verbose:
                        print(f"INFO: Skipping very short file '{filename}'.")
                    continue
                if fs != SAMPLE_RATE:                                         # :92-94 torchaudio Resample defaults
                    from .resample import resample_sinc_hann
                    mono = resample_sinc_hann(mono, fs, SAMPLE_RATE, device=eng.device)
                clips.append(mono)
                names.append(filename)
            except Exception as e:
                if verbose:
                    print(f"FATAL ERROR processing file '{filename}': {e}. Skipping.")
        if not clips:
            continue
        def run(batch_clips):
            lengths = [int(c.numel()) for c in batch_clips]
            offs = np.zeros(len(batch_clips) + 1, dtype=np.int64)
            offs[1:] = np.cumsum(lengths)
            wav = torch.cat(batch_clips) if len(batch_clips) > 1 else batch_clips[0].contiguous()
            out, frame_off = eng.extract_packed(wav, offs[:-1], lengths, chunk_seconds, overlap_seconds)
            torch.cuda.synchronize()
            return out.cpu().numpy(), frame_off

        def run_layers(batch_clips):
            """-> per clip: [n_sel, T, H] frames (pooled: [n_sel, H] means), or None when no window survived."""
            _, unique, pos = sel
            res = [None] * len(batch_clips)
            for grp in eng.file_groups([int(batch_clips[i].numel()) for i in range(len(batch_clips))],
                                       len(unique), chunk_seconds, overlap_seconds):
                gc = [batch_clips[i] for i in grp]
                lengths = [int(c.numel()) for c in gc]
                offs = np.zeros(len(gc) + 1, dtype=np.int64)
                offs[1:] = np.cumsum(lengths)
                wav = torch.cat(gc) if len(gc) > 1 else gc[0].contiguous()
                if pooled:
                    means, frame_off = eng.pooled_hidden(wav, offs[:-1], lengths, unique, chunk_seconds, overlap_seconds)
                    torch.cuda.synchronize()
                    host = means.cpu().numpy()
                    for k, i in enumerate(grp):
                        if int(frame_off[k + 1]) > int(frame_off[k]):
                            res[i] = host[pos, k]
                else:
                    _, frame_off, planes = eng.extract_packed(wav, offs[:-1], lengths, chunk_seconds, overlap_seconds,
                                                              layers=unique)
                    torch.cuda.synchronize()
                    host = planes.cpu().numpy()
                    del planes
                    for k, i in enumerate(grp):
                        a, b = int(frame_off[k]), int(frame_off[k + 1])
                        if b > a:
                            res[i] = host[pos, a:b]                            # fancy index: a copy per file
            return res

        def per_clip(batch_clips):
            if sel is not None:
                return run_layers(batch_clips)
            host, frame_off = run(batch_clips)
            return [host[int(frame_off[i]):int(frame_off[i + 1])].copy() if int(frame_off[i + 1]) > int(frame_off[i]) else None
                    for i in range(len(batch_clips))]

        def keep(fn, r):
            if r is not None:                                                  # :123 (no chunk survived)
                sequences[fn] = r[0] if isinstance(output_layers, (int, np.integer)) else r

        try:
            for fn, r in zip(names, per_clip(clips)):
                keep(fn, r)
        except (_lib.RsafError, torch.cuda.OutOfMemoryError) as e:
            # one bad file (or an allocation failure of the whole batch) must not take the other files of the batch or
            # the files already done with it: the reference skips only the offending file (:127-129).  Any other
            # RuntimeError (a HIP fault surfacing at the synchronize) is NOT retried on the poisoned context: it propagates.
            if verbose:
                print(f"WARNING: batch of {len(clips)} files failed ({e}); retrying file by file.")
            for fn, c in zip(names, clips):
                try:
                    keep(fn, per_clip([c])[0])
                except (_lib.RsafError, torch.cuda.OutOfMemoryError) as e1:
                    if verbose:
                        print(f"FATAL ERROR processing file '{fn}': {e1}. Skipping.")
    return sequences, sel


def extract_wav2vec2_embeddings(input_df, **kwargs):
    """Drop-in for ``src/foundation_model_extractor.py:133-166``: time-mean per file.

    output_layers (see ``extract_wav2vec2_sequences``): the means of the selected hidden states, pooled on the device
    (only [files, n_sel, hidden] reaches the host).  Columns: ``dim_{k}`` for an int, ``l{layer}_dim_{k}`` for a list
    (layer = the non-negative index), then ``filename``."""
    import pandas as pd
    output_layers = kwargs.pop("output_layers", None)                   # keyword only: the reference's (input_df, **kwargs)
    if output_layers is None:
        seqs = extract_wav2vec2_sequences(input_df, **kwargs)
        if not seqs:
            return pd.DataFrame()
        rows = []
        for filename, seq in seqs.items():
            m = np.mean(seq, axis=0)
            d = {f"dim_{k}": v for k, v in enumerate(m)}
            d["filename"] = filename
            rows.append(d)
        return pd.DataFrame(rows)
    args = dict(model_name="facebook/wav2vec2-base-960h", audio_file_column="filepath", chunk_seconds=5, overlap_seconds=1,
                verbose=True, batch_files=64)
    unknown = set(kwargs) - set(args)
    if unknown:
        raise TypeError(f"extract_wav2vec2_embeddings() got unexpected keyword arguments {sorted(unknown)}")
    args.update(kwargs)
    means, sel = _extract(input_df, output_layers=output_layers, pooled=True, **args)
    if not means:
        return pd.DataFrame()
    return pd.DataFrame(embedding_rows(means, None if isinstance(output_layers, (int, np.integer)) else sel[0]))


def embedding_rows(means, layers):
    """{filename: means} -> the rows of ``extract_wav2vec2_embeddings``: ``dim_{k}`` of [H] means when ``layers`` is None,
    else ``l{layers[j]}_dim_{k}`` of [len(layers), H] means; then ``filename``."""
    rows = []
    for filename, m in means.items():
        if layers is None:
            d = {f"dim_{k}": v for k, v in enumerate(m)}
        else:
            d = {}
            for j, layer in enumerate(layers):
                d.update({f"l{int(layer)}_dim_{k}": v for k, v in enumerate(m[j])})
        d["filename"] = filename
        rows.append(d)
    return rows
