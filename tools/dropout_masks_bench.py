"""Time the drawing of the dropout masks of one group training step of K CNN-LSTM replicas, from either source:
``draw_masks`` per replica (torch's device RNG: rand / >= / to / div per mask, the path of a model without a stream) against
one ``draw_masks_group`` call (``rsaf_dropout_masks_group``: every mask of every replica in one launch).  The two alternate
within every repetition in one process; times are host clocks around work that ends in a device synchronise.  The kernel's
own time comes from the ``train_dropout_masks`` family of rsaf_prof_* in a pass of its own, and the write rate is the bytes
of the masks over that time.  Then ``cnnlstm_train_step_group`` at the same K with masks from each source, alternating.

Default row: the training shape the README quotes (B = 4, T = 20 000, reference architecture: C = H = 128, two LSTM
layers), p = 0.3 everywhere, K = 16; a second row at T = 500 shows the launch-bound end.

    python tools/dropout_masks_bench.py [--k 16] [--reps 10] [--step-reps 3] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from robust_speech_analysis_framework_amd import _lib
from robust_speech_analysis_framework_amd.cnnlstm import (CNNLSTM, DropoutStream, FusedAdam, cnnlstm_train_step_group, draw_masks,
                                                          draw_masks_group)

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=16)
ap.add_argument("--p", type=float, default=0.3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--step-reps", type=int, default=3)
ap.add_argument("--shapes", default="4x20000,4x500")
ap.add_argument("--json", default=None)
args = ap.parse_args()
_lib.require_gpu()
_lib.load()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def mask_floats(mk):
    return sum(t.numel() for t in [mk["res_block1"], mk["res_block2"], mk["fc"], *mk["lstm"]] if t is not None)


def stats(v):
    return {"mean_ms": sum(v) / len(v), "min_ms": min(v), "max_ms": max(v)}


def row(B, T):
    K = args.k
    models = []
    for _ in range(K):
        m = CNNLSTM(dropout_rate=args.p).to("cuda").train()
        m.res_block1.dropout.p = m.res_block2.dropout.p = args.p
        models.append(m)
    streams = [DropoutStream(1000 + k) for k in range(K)]
    shapes = [(B, T)] * K

    def per_replica():
        return [draw_masks(m, B, T, "cuda") for m in models]

    def group():
        return draw_masks_group(models, shapes, streams, "cuda")

    nbytes = 4 * sum(mask_floats(mk) for mk in group())
    for _ in range(2):                                  # warm up both (allocator pools, code objects)
        per_replica()
        group()
    t_old, t_new = [], []
    for _ in range(args.reps):
        t_old.append(timed(per_replica))
        t_new.append(timed(group))
    torch.cuda.synchronize()
    _lib.prof_begin()
    for _ in range(args.reps):
        group()
    torch.cuda.synchronize()
    fam = _lib.prof_end()["train_dropout_masks"]
    kernel_ms = fam["ms"] / fam["launches"]
    rec = {"B": B, "T": T, "K": K, "p": args.p, "mask_bytes": nbytes, "draw_masks_per_replica": stats(t_old),
           "draw_masks_group": stats(t_new), "kernel_ms": kernel_ms, "kernel_launches_per_call": fam["launches"] / args.reps,
           "kernel_write_GBps": nbytes / kernel_ms / 1e6}
    print(f"== B={B} T={T} K={K} p={args.p}: {nbytes / 1e6:.1f} MB of masks per step", flush=True)
    print(f"   draw_masks per replica (torch RNG)  {stats(t_old)['mean_ms']:9.3f} ms  (min {min(t_old):.3f}, max {max(t_old):.3f})", flush=True)
    print(f"   draw_masks_group (one launch)       {stats(t_new)['mean_ms']:9.3f} ms  (min {min(t_new):.3f}, max {max(t_new):.3f})", flush=True)
    print(f"   kernel alone                        {kernel_ms:9.3f} ms  = {rec['kernel_write_GBps']:.0f} GB/s written, "
          f"{rec['kernel_launches_per_call']:.0f} launch per call", flush=True)

    # the whole fused step with masks from either source
    opts = [FusedAdam(m, lr=1e-4) for m in models]
    xs = [torch.randn((B, T, 768), device="cuda") for _ in range(K)]
    ys = [torch.randint(0, 2, (B,), device="cuda") for _ in range(K)]

    def step(with_stream):
        for m, st in zip(models, streams):
            m.dropout_stream = st if with_stream else None
        cnnlstm_train_step_group(models, opts, xs, ys)

    try:
        step(False)
        step(True)
        s_old, s_new = [], []
        for _ in range(args.step_reps):
            s_old.append(timed(lambda: step(False)))
            s_new.append(timed(lambda: step(True)))
        rec["train_step_torch_rng"] = stats(s_old)
        rec["train_step_stream"] = stats(s_new)
        print(f"   cnnlstm_train_step_group, torch RNG {stats(s_old)['mean_ms']:9.2f} ms  (min {min(s_old):.2f}, max {max(s_old):.2f})", flush=True)
        print(f"   cnnlstm_train_step_group, streams   {stats(s_new)['mean_ms']:9.2f} ms  (min {min(s_new):.2f}, max {max(s_new):.2f})", flush=True)
    except torch.cuda.OutOfMemoryError:
        rec["train_step_skipped"] = "out of device memory"
        print("   cnnlstm_train_step_group: skipped, out of device memory", flush=True)
    del models, opts, xs, ys
    torch.cuda.empty_cache()
    return rec


rows = [row(*[int(v) for v in s.split("x")]) for s in args.shapes.split(",")]
if args.json:
    with open(args.json, "w") as f:
        json.dump({"reps": args.reps, "step_reps": args.step_reps, "warmup": 2, "rows": rows}, f, indent=1)
        f.write("\n")
