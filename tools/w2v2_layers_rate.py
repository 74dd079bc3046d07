"""Rate of Wav2Vec2 hidden-state extraction at the base geometry: last layer only, all 13 hidden states as device
sequences, and all 13 pooled per clip on the device.

Times ``W2V2Engine.extract_packed`` (without and with ``layers``) and ``W2V2Engine.pooled_hidden`` on 64 x 30 s synthetic
clips (the reference's 5 s / 4 s window plan) with seeded random weights, in one process, the three variants alternating
within every repeat, and prints audio seconds per second for each plus the pooled / last-layer ratio.

    python tools/w2v2_layers_rate.py [--clips 64] [--seconds 30] [--reps 7] [--out FILE]
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

from robust_speech_analysis_framework_amd import synth  # noqa: E402
from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine  # noqa: E402
from robust_speech_analysis_framework_amd.w2v2_config import W2V2Config, random_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    clips = synth.synth_batch(a.clips, a.seconds, pool=8)
    lengths = [clips.shape[1]] * a.clips
    offs = np.arange(a.clips, dtype=np.int64) * clips.shape[1]
    wav = torch.from_numpy(clips.reshape(-1)).cuda()
    cfg = W2V2Config()
    eng = W2V2Engine(cfg, random_state_dict(cfg, seed=0))
    layers = list(range(cfg.num_hidden_layers + 1))
    variants = {
        "last_layer": lambda: eng.extract_packed(wav, offs, lengths),
        "all_sequences": lambda: eng.extract_packed(wav, offs, lengths, layers=layers),
        "all_pooled": lambda: eng.pooled_hidden(wav, offs, lengths, layers),
    }
    for f in variants.values():                            # warm-up (workspace, weight planes, code objects, allocator)
        f()
        torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, f in variants.items():
            t0 = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
            del r
    audio = sum(lengths) / 16000.0
    res = {"device": torch.cuda.get_device_name(0), "clips": a.clips, "seconds": a.seconds, "reps": a.reps,
           "hidden_states": len(layers)}
    for k, t in times.items():
        med = float(np.median(t))
        res[k] = {"median_s": med, "min_s": float(min(t)), "max_s": float(max(t)), "audio_s": audio, "audio_s_per_s": audio / med}
        print(f"{k:14s} {audio:.0f} audio-s in {med * 1e3:.1f} ms (median of {a.reps}, {min(t) * 1e3:.1f}-{max(t) * 1e3:.1f})"
              f"  -> {audio / med:.0f} audio-s/s", flush=True)
    for k in ("all_sequences", "all_pooled"):
        res[f"{k}_over_last"] = res[k]["audio_s_per_s"] / res["last_layer"]["audio_s_per_s"]
        print(f"{k} / last_layer: {res[f'{k}_over_last']:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
