"""Time the eval-mode forward of K independent CNN-LSTM (model, batch) pairs on the HIP path: one group call
(cnnlstm_forward_group) or, with --sequential, the plain loop of model(x) calls, which uses nothing newer than
CNNLSTM.forward and therefore also runs on a checkout without the group entry.  Shapes are the reference defaults
(D = 768, C = H = 128, silu) at 4 x 4 378, 4 x 20 000 and 8 x 20 000 frames; K runs over 1, 2, 3, 5, 8, 16 distinct models,
one row takes 16 batches of ONE model (a validation loader) and one ragged row K = 3 batches of different length.  Per
row: one warm-up call, --steps timed calls between device synchronisations with the profiler off, then one more call under
rsaf_prof_* for the per-kernel-family breakdown.

    python tools/eval_group_bench.py [--sequential] [--json PATH] [--only-shape I] [--ks 1,3,5] [--steps N]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from robust_speech_analysis_framework_amd import _lib
from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--ks", default="1,2,3,5,8,16")
ap.add_argument("--only-shape", type=int, default=-1,
                help="0: reading task, 1: interview sessions, 2: interview sessions at batch 8, 3: one model x 16 batches, 4: the ragged row")
ap.add_argument("--sequential", action="store_true", help="the loop of model(x) calls in place of the group call")
ap.add_argument("--json", default=None)
args = ap.parse_args()
lib = _lib.load()

SHAPES = [(4, 4378, "reading task, batch 4"), (4, 20000, "interview sessions, batch 4"), (8, 20000, "interview sessions, batch 8")]
RAGGED = [(4, 3000), (4, 4378), (4, 6000)]
KS = [int(k) for k in args.ks.split(",")]
MODE = "sequential model(x) calls" if args.sequential else "one group call"


def call_bytes(shapes):
    """Device bytes the call holds: workspaces and inputs (the weights are small)."""
    d = CNNLSTM().dims
    return sum(int(lib.rsaf_cnnlstm_workspace_bytes(B, T, d["input_dim"], d["channels"], d["hidden"], d["layers"])) +
               4 * B * T * d["input_dim"] for B, T in shapes)


def run(shapes, n_models, steps):
    made = [CNNLSTM().to("cuda").eval() for _ in range(n_models)]
    models = [made[k % n_models] for k in range(len(shapes))]
    xs = [torch.randn((B, T, 768), device="cuda") for B, T in shapes]
    if args.sequential:
        def one():
            return [m(x) for m, x in zip(models, xs)]
    else:
        from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group

        def one():
            return cnnlstm_forward_group(models, xs)

    one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    _lib.prof_begin()
    one()
    torch.cuda.synchronize()
    return dt, _lib.prof_end()


def row(tag, shapes, n_models=None):
    n_models = n_models or len(shapes)
    need = call_bytes(shapes)
    free = torch.cuda.mem_get_info()[0]
    head = f"== {tag}: K={len(shapes)} items of {n_models} model(s), {need / 2**30:.2f} GiB of workspaces + inputs"
    rec = {"tag": tag, "K": len(shapes), "models": n_models, "shapes": [list(s) for s in shapes], "call_bytes": need}
    if need > 0.85 * free:
        print(f"{head}: skipped, {free / 2**30:.1f} GiB free", flush=True)
        return dict(rec, skipped="does not fit the device memory")
    try:
        dt, prof = run(shapes, n_models, args.steps)
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        print(f"{head}: skipped, out of device memory", flush=True)
        return dict(rec, skipped="out of device memory")
    ms = lambda name: prof.get(name, {}).get("ms", 0.0)                             # noqa: E731
    fam_ms = sum(v["ms"] for v in prof.values())
    print(f"{head}: {dt * 1e3:.2f} ms per call, {dt * 1e3 / len(shapes):.2f} ms per item; profiled call: recurrences "
          f"{ms('lstm_recurrent'):.2f} ms ({100 * ms('lstm_recurrent') / max(fam_ms, 1e-9):.0f} % of the kernel time), attention "
          f"pooling {ms('attnpool_fc'):.2f} ms ({100 * ms('attnpool_fc') / max(fam_ms, 1e-9):.0f} %)", flush=True)
    for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
        print(f"   {k:26s} {v['launches']:6.0f} launches  {v['ms']:9.2f} ms", flush=True)
    torch.cuda.empty_cache()
    return dict(rec, ms_per_call=dt * 1e3, ms_per_item=dt * 1e3 / len(shapes), recurrence_ms=ms("lstm_recurrent"),
                attnpool_ms=ms("attnpool_fc"), kernel_ms=fam_ms,
                families={k: {"launches": v["launches"], "ms": v["ms"]} for k, v in prof.items()})


print(f"# eval forward, {MODE}; {args.steps} timed calls per row after one warm-up", flush=True)
rows = []
for i, (B, T, tag) in enumerate(SHAPES):
    if args.only_shape not in (-1, i):
        continue
    for K in KS:
        rows.append(row(f"{tag} (B={B} T={T})", [(B, T)] * K))
if args.only_shape in (-1, 3):
    rows.append(row("one model x 16 batches (B=4 T=4378)", [(4, 4378)] * 16, n_models=1))
if args.only_shape in (-1, 4):
    rows.append(row("ragged, T = 3000 / 4378 / 6000", RAGGED))
if args.json:
    with open(args.json, "w") as f:
        json.dump({"mode": MODE, "steps": args.steps, "warmup": 1, "rows": rows}, f, indent=1)
        f.write("\n")
