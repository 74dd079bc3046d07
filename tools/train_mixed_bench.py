"""Time the fused training step of 15 CNN-LSTM replicas of FIVE architectures (three folds each: what a hyper-parameter
search with five trials in flight trains, src/dl_cv_strategies.py:216-251) three ways:

  (a) 15 steps of one replica each (``cnnlstm_train_step_group`` with K = 1),
  (b) five group steps of K = 3, one per architecture: what the group step can do without ``mixed=True``,
  (c) one mixed group step of K = 15 (``mixed=True``).

All three run the fused step (``FusedAdam``, cross-entropy, running statistics in HIP) with dropout masks from a
``DropoutStream`` per replica, on the same models and batches.  The architectures are drawn from the reference's search space
(cnn_out_channels in {32, 64, 128}, lstm_hidden_dim in {64, 128}, activation silu / gelu), input_dim 768, batch 4, at the two
sequence lengths of tools/train_bench.py.  After one warm-up round of all three, every repetition times (a), (b), (c) in
turn (alternating, so that drift of the machine hits all three alike); times are host clocks around work that ends in a
device synchronise.  A last pass under rsaf_prof_* gives the recurrence families' share of (b) and (c).

    python tools/train_mixed_bench.py [--reps 5] [--shapes 4x4378,4x20000] [--out PATH.txt] [--json PATH.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from robust_speech_analysis_framework_amd import _lib
from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, DropoutStream, FusedAdam, cnnlstm_train_step_group

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shapes", default="4x4378,4x20000")
ap.add_argument("--folds", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()
_lib.require_gpu()
_lib.load()

ARCHS = [(32, 64, "silu", 0.3), (64, 128, "gelu", 0.4), (128, 64, "silu", 0.2), (128, 128, "gelu", 0.5), (64, 64, "gelu", 0.3)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"mean_ms": sum(v) / len(v), "min_ms": min(v), "max_ms": max(v)}


def rec_ms(prof):
    return sum(v["ms"] for k, v in prof.items() if k in ("lstm_recurrent", "lstm_bwd_recurrent"))


def row(B, T):
    models, groups = [], []
    for a, (C, H, act, p) in enumerate(ARCHS):
        part = []
        for f in range(args.folds):
            m = CNNLSTM(input_dim=768, cnn_out_channels=C, lstm_hidden_dim=H, activation_fn=act, dropout_rate=p).to("cuda").train()
            m.dropout_stream = DropoutStream(1000 + 10 * a + f)
            part.append(len(models))
            models.append(m)
        groups.append(part)
    K = len(models)
    opts = [FusedAdam(m, lr=1e-4) for m in models]
    xs = [torch.randn((B, T, 768), device="cuda") for _ in range(K)]
    ys = [torch.randint(0, 2, (B,), device="cuda") for _ in range(K)]
    pick = lambda idx: ([models[k] for k in idx], [opts[k] for k in idx], [xs[k] for k in idx], [ys[k] for k in idx])   # noqa: E731

    def singles():
        for k in range(K):
            cnnlstm_train_step_group(*pick([k]))

    def per_arch():
        for part in groups:
            cnnlstm_train_step_group(*pick(part))

    def mixed():
        cnnlstm_train_step_group(*pick(range(K)), mixed=True)

    for fn in (singles, per_arch, mixed):                 # warm-up: every shape of every path
        fn()
    ta, tb, tc = [], [], []
    for _ in range(args.reps):
        ta.append(timed(singles))
        tb.append(timed(per_arch))
        tc.append(timed(mixed))
    prof = {}
    for name, fn in (("per_arch", per_arch), ("mixed", mixed)):
        torch.cuda.synchronize()
        _lib.prof_begin()
        fn()
        torch.cuda.synchronize()
        prof[name] = _lib.prof_end()
    a, b, c = stats(ta), stats(tb), stats(tc)
    say(f"== B={B} T={T}: {K} replicas = {len(ARCHS)} architectures x {args.folds} folds, fused step, {args.reps} repetitions after 1 warm-up")
    say(f"   (a) {K} single steps                    {a['mean_ms']:9.2f} ms  (min {a['min_ms']:.2f}, max {a['max_ms']:.2f})")
    say(f"   (b) {len(ARCHS)} group steps of K = {args.folds}, one per arch. {b['mean_ms']:9.2f} ms  (min {b['min_ms']:.2f}, max {b['max_ms']:.2f})")
    say(f"   (c) one mixed group step of K = {K}      {c['mean_ms']:9.2f} ms  (min {c['min_ms']:.2f}, max {c['max_ms']:.2f})")
    say(f"   (c) / (b) = {c['mean_ms'] / b['mean_ms']:.3f}    (c) / (a) = {c['mean_ms'] / a['mean_ms']:.3f}    (b) / (a) = {b['mean_ms'] / a['mean_ms']:.3f}")
    for name in ("per_arch", "mixed"):
        fam = prof[name]
        say(f"   recurrence families of {'(b)' if name == 'per_arch' else '(c)'}: {rec_ms(fam):9.2f} ms in "
            f"{fam['lstm_recurrent']['launches'] + fam['lstm_bwd_recurrent']['launches']} launches; all families {sum(v['ms'] for v in fam.values()):.2f} ms")
    del models, opts, xs, ys
    torch.cuda.empty_cache()
    return {"B": B, "T": T, "K": K, "archs": [list(a) for a in ARCHS], "folds": args.folds, "singles": a, "per_architecture_groups": b,
            "mixed_group": c, "mixed_over_per_architecture": c["mean_ms"] / b["mean_ms"], "mixed_over_singles": c["mean_ms"] / a["mean_ms"],
            "recurrence_ms": {k: rec_ms(v) for k, v in prof.items()},
            "families": {k: {n: {"launches": f["launches"], "ms": f["ms"]} for n, f in v.items()} for k, v in prof.items()}}


rows = [row(*[int(v) for v in s.split("x")]) for s in args.shapes.split(",")]
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
if args.json:
    with open(args.json, "w") as f:
        json.dump({"reps": args.reps, "warmup": 1, "rows": rows}, f, indent=1)
        f.write("\n")
