"""Time one GROUP training step of K independent CNN-LSTM replicas (zero_grad / group forward / summed CrossEntropy / one
backward / one Adam over all replicas' parameters) on the HIP path, with the per-kernel-family event breakdown of
rsaf_prof_*.  Shapes are those of tools/train_bench.py (reference defaults D = 768, C = H = 128, silu), K runs over
1, 2, 3, 5, 8, 16, and one ragged row has K = 3 replicas of different length.  One timed step per configuration after
one warm-up step unless --steps says otherwise, as train_bench.py does.  Every row also prints wall - sum of the
families: the time the step spends outside this project's kernels (torch ops, launches, host).

--fused runs the same shapes and K through cnnlstm_train_step_group with one FusedAdam per replica: cross-entropy, Adam,
the packing of the parameter blobs and the BatchNorm running statistics are then one launch each per group step.

    python tools/train_group_bench.py [--fused] [--json PATH] [--only-shape I] [--ks 1,3,5]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from robust_speech_analysis_framework_amd import _lib
from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, cnnlstm_train_group

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=1)
ap.add_argument("--ks", default="1,2,3,5,8,16")
ap.add_argument("--only-shape", type=int, default=-1, help="0: reading task, 1: interview sessions, 2: the ragged row")
ap.add_argument("--fused", action="store_true", help="FusedAdam per replica + cnnlstm_train_step_group")
ap.add_argument("--json", default=None)
args = ap.parse_args()
lib = _lib.load()

SHAPES = [(4, 4378, "reading task, batch 4"), (4, 20000, "interview sessions, batch 4")]
RAGGED = [(4, 3000), (4, 4378), (4, 6000)]
KS = [int(k) for k in args.ks.split(",")]


def step_bytes(shapes):
    """Device bytes the step holds per replica: saved activations, scratch, input (parameters and Adam state are small)."""
    d = CNNLSTM().dims
    n = 0
    for B, T in shapes:
        a = (B, T, d["input_dim"], d["channels"], d["hidden"], d["layers"])
        n += 4 * (int(lib.rsaf_cnnlstm_train_saved_floats(*a)) + int(lib.rsaf_cnnlstm_train_scratch_floats(*a)) + B * T * d["input_dim"])
    return n


def run(shapes, steps):
    models = [CNNLSTM().to("cuda").train() for _ in shapes]
    xs = [torch.randn((B, T, 768), device="cuda") for B, T in shapes]
    ys = [torch.randint(0, 2, (B,), device="cuda") for B, _ in shapes]
    if args.fused:
        from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, cnnlstm_train_step_group
        opts = [FusedAdam(m, lr=1e-4) for m in models]

        def one():
            cnnlstm_train_step_group(models, opts, xs, ys)
    else:
        opt = torch.optim.Adam([p for m in models for p in m.parameters()], lr=1e-4)
        loss_fn = torch.nn.CrossEntropyLoss()

        def one():
            opt.zero_grad()
            outs = cnnlstm_train_group(models, xs)
            loss = torch.stack([loss_fn(o, y) for o, y in zip(outs, ys)]).sum()
            loss.backward()
            opt.step()

    one()
    torch.cuda.synchronize()
    _lib.prof_begin()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return dt, _lib.prof_end()


def row(tag, shapes):
    need = step_bytes(shapes)
    free = torch.cuda.mem_get_info()[0]
    head = f"== {tag}: K={len(shapes)}, {need / 2**30:.2f} GiB of saved activations + scratch + inputs"
    rec = {"tag": tag, "K": len(shapes), "shapes": [list(s) for s in shapes], "step_bytes": need}
    if need > 0.85 * free:
        print(f"{head}: skipped, {free / 2**30:.1f} GiB free", flush=True)
        return dict(rec, skipped="does not fit the device memory")
    try:
        dt, prof = run(shapes, args.steps)
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        print(f"{head}: skipped, out of device memory", flush=True)
        return dict(rec, skipped="out of device memory")
    rec_ms = sum(v["ms"] for k, v in prof.items() if k in ("lstm_recurrent", "lstm_bwd_recurrent")) / args.steps
    fam_ms = sum(v["ms"] for v in prof.values()) / args.steps
    print(f"{head}: {dt * 1e3:.1f} ms per group step, {dt * 1e3 / len(shapes):.1f} ms per replica, recurrences {rec_ms:.1f} ms, "
          f"families {fam_ms:.1f} ms, wall - families {dt * 1e3 - fam_ms:.1f} ms", flush=True)
    for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
        print(f"   {k:26s} {v['launches'] / args.steps:6.0f} launches  {v['ms'] / args.steps:9.2f} ms", flush=True)
    torch.cuda.empty_cache()
    return dict(rec, fused=args.fused, ms_per_step=dt * 1e3, recurrence_ms=rec_ms, families_ms=fam_ms, outside_ms=dt * 1e3 - fam_ms,
                families={k: {"launches": v["launches"] / args.steps, "ms": v["ms"] / args.steps} for k, v in prof.items()})


rows = []
for i, (B, T, tag) in enumerate(SHAPES):
    if args.only_shape not in (-1, i):
        continue
    for K in KS:
        rows.append(row(f"{tag} (B={B} T={T})", [(B, T)] * K))
if args.only_shape in (-1, 2):
    rows.append(row("ragged, T = 3000 / 4378 / 6000", RAGGED))
    rows.append(row("single step of the longest ragged replica (B=4 T=6000)", RAGGED[2:]))
if args.json:
    with open(args.json, "w") as f:
        json.dump({"steps": args.steps, "warmup": 1, "rows": rows}, f, indent=1)
        f.write("\n")
