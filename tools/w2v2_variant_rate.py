"""Rate of the Wav2Vec2 stage per architecture: Wav2Vec2 base and large stable-layer-norm, WavLM base, HuBERT base,
data2vec-audio base (beside ``base_layer_norm``, the Wav2Vec2 geometry it differs from in the positional stage alone).

Times ``W2V2Engine.extract_packed`` on 64 x 30 s synthetic clips (the reference's 5 s / 4 s window plan: 448 windows)
with seeded random weights, and prints audio seconds per second for each architecture.  The architectures alternate
within every repetition (one process, one device), so a drift of the device hits all of them alike; ratios are taken
per repetition.

After the timed repetitions one more pass per architecture runs under the library's profiler and reports the
positional stage's families (``w2v2_posconv_stack``, ``w2v2_posconv_gemm``, ``w2v2_regroup``) in milliseconds per pass.

    python tools/w2v2_variant_rate.py [--models base,wavlm_base] [--clips 64] [--seconds 30] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from robust_speech_analysis_framework_amd import _lib, synth  # noqa: E402
from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine  # noqa: E402
from robust_speech_analysis_framework_amd.w2v2_config import W2V2Config, random_state_dict  # noqa: E402

LARGE = dict(conv_dim=(512,) * 7, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
             intermediate_size=4096, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
             feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)


BASE = dict(conv_dim=(512,) * 7, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
MODELS = {
    "base": W2V2Config(),
    "large_stable_ln": W2V2Config(**LARGE),
    "wavlm_base": W2V2Config(**BASE, model_type="wavlm"),
    "hubert_base": W2V2Config(**BASE, model_type="hubert", feat_proj_layer_norm=False),
    "base_layer_norm": W2V2Config(**BASE, feat_extract_norm="layer"),
    "data2vec_base": W2V2Config(**BASE, model_type="data2vec-audio", feat_extract_norm="layer", num_conv_pos_embeddings=5,
                                conv_pos_kernel_size=19, num_conv_pos_embedding_groups=16),
}
POS_FAMILIES = ("w2v2_posconv_stack", "w2v2_posconv_gemm", "w2v2_regroup")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="base,large_stable_ln", help="comma-separated: " + ", ".join(MODELS))
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = a.models.split(",")
    unknown = [n for n in names if n not in MODELS]
    if unknown:
        ap.error(f"unknown models {unknown}")
    clips = synth.synth_batch(a.clips, a.seconds, pool=8)
    lengths = [clips.shape[1]] * a.clips
    offs = np.arange(a.clips, dtype=np.int64) * clips.shape[1]
    wav = torch.from_numpy(clips.reshape(-1)).cuda()
    audio = sum(lengths) / 16000.0
    engines, frames = {}, {}
    for n in names:                                        # warm-up (workspace, weight planes, code objects)
        engines[n] = W2V2Engine(MODELS[n], random_state_dict(MODELS[n], seed=0))
        frames[n] = int(engines[n].extract_packed(wav, offs, lengths)[0].shape[0])
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for rep in range(a.reps):                              # the architectures alternate within every repetition
        for n in names[rep % len(names):] + names[:rep % len(names)]:
            t0 = time.perf_counter()
            engines[n].extract_packed(wav, offs, lengths)
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
    pos_ms = {}
    for n in names:                                        # one profiled pass each: the positional stage's kernel families
        _lib.prof_begin()
        engines[n].extract_packed(wav, offs, lengths)
        torch.cuda.synchronize()
        prof = _lib.prof_end()
        pos_ms[n] = {k: prof[k]["ms"] for k in POS_FAMILIES if k in prof}
    res = {"device": torch.cuda.get_device_name(0), "clips": a.clips, "seconds": a.seconds, "reps": a.reps, "order": "alternating"}
    for n in names:
        cfg, t = MODELS[n], np.array(times[n])
        med = float(np.median(t))
        res[n] = {"model_type": cfg.model_type, "flags": cfg.flags, "hidden": cfg.hidden_size, "layers": cfg.num_hidden_layers,
                  "frames": frames[n], "median_s": med, "min_s": float(t.min()), "max_s": float(t.max()), "audio_s": audio,
                  "audio_s_per_s": audio / med, "times_s": [float(v) for v in t], "positional_stage_ms": pos_ms[n]}
        print(f"{n:16s} {cfg.model_type:8s} flags {cfg.flags:3d}  {audio:.0f} audio-s in {med * 1e3:.1f} ms (median of {a.reps}, "
              f"{t.min() * 1e3:.1f} .. {t.max() * 1e3:.1f})  -> {audio / med:.0f} audio-s/s", flush=True)
        print(f"{'':16s} positional stage, one profiled pass: "
              + ", ".join(f"{k} {v:.3f} ms" for k, v in pos_ms[n].items()), flush=True)
    for n in names[1:]:                                    # time ratio to the first model, per repetition
        r = np.array(times[n]) / np.array(times[names[0]])
        res[f"{n}_over_{names[0]}_time"] = {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())}
        print(f"{n} / {names[0]} time: median {np.median(r):.4f} ({r.min():.4f} .. {r.max():.4f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
