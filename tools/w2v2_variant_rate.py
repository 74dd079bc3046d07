"""Rate of the Wav2Vec2 stage at the base geometry and at the large stable-layer-norm geometry.

Times ``W2V2Engine.extract_packed`` on 64 x 30 s synthetic clips (the reference's 5 s / 4 s window plan: 448 windows)
with seeded random weights, and prints audio seconds per second for each architecture.

    python tools/w2v2_variant_rate.py [--clips 64] [--seconds 30] [--reps 5] [--out FILE]
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

LARGE = dict(conv_dim=(512,) * 7, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
             intermediate_size=4096, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
             feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)


def rate(cfg, wav, offs, lengths, reps):
    eng = W2V2Engine(cfg, random_state_dict(cfg, seed=0))
    eng.extract_packed(wav, offs, lengths)                 # warm-up (workspace, weight planes, code objects)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out, _ = eng.extract_packed(wav, offs, lengths)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    audio = sum(lengths) / 16000.0
    med = float(np.median(times))
    return {"flags": cfg.flags, "hidden": cfg.hidden_size, "layers": cfg.num_hidden_layers, "frames": int(out.shape[0]),
            "median_s": med, "min_s": float(min(times)), "audio_s": audio, "audio_s_per_s": audio / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    clips = synth.synth_batch(a.clips, a.seconds, pool=8)
    lengths = [clips.shape[1]] * a.clips
    offs = np.arange(a.clips, dtype=np.int64) * clips.shape[1]
    wav = torch.from_numpy(clips.reshape(-1)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "clips": a.clips, "seconds": a.seconds, "reps": a.reps}
    for name, cfg in (("base", W2V2Config()), ("large_stable_ln", W2V2Config(**LARGE))):
        r = rate(cfg, wav, offs, lengths, a.reps)
        res[name] = r
        print(f"{name:16s} flags {r['flags']:2d}  {r['audio_s']:.0f} audio-s in {r['median_s'] * 1e3:.1f} ms (median of {a.reps})"
              f"  -> {r['audio_s_per_s']:.0f} audio-s/s", flush=True)
    res["base_over_large"] = res["base"]["audio_s_per_s"] / res["large_stable_ln"]["audio_s_per_s"]
    print(f"base / large: {res['base_over_large']:.2f}x")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
