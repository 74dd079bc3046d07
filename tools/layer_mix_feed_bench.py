"""What a learned layer mix costs a lock-step group step, by route:

    A  what the code could do before resident layer stacks: per replica the zero-padded stack h [B, L, T, D] built on the host
       (np.stack of the members' [L, T, D] arrays), copied to the device, LayerMix(h) -> cnnlstm_train_group -> loss.backward(),
       FusedAdam.step() for the classifier and torch.optim.Adam for the mix weights, one replica at a time;
    B  the fused mix step: DeviceBatchLoader over one DeviceSequenceStore(layers=L), train_replicas_lockstep(mixes=...) with
       FusedAdam(layer_mix=...): one cnnlstm_mix_train_step_group call per group step.

One small store (--pool sequences of full length T) is reused by all replicas and, through repeated indices, by all steps of a
window, so that memory bounds nothing but the route under test.  Both routes are warmed at the timed shapes, then the windows
run A / B / A / B in one process, timed with a host clock around work that ends in a synchronise.  Route A is slow (a host copy
and an upload of L + 1 times the batch per replica and step), so its windows may take fewer group steps (--a-steps); the figures
are per group step either way, and the record says how many were timed.  Peak intermediate memory is counted from the shapes.

    python tools/layer_mix_feed_bench.py [--out-dir profiles/r29] [--ks 1,3,16] [--steps 20] [--a-steps 20] [--shapes 4378,20000]

--kernels runs only the kernels, for a separate `rocprofv3 --kernel-trace --stats` run: the collate-mix forward and backward on one
batch beside layer_mix_forward / layer_mix_backward on the padded stack of the same batch (same L, same positions) and the plain
collate launch, --kernel-reps times each, alternating; it writes the bytes each kernel moves per launch, counted from the shapes,
to <out-dir>/layer_mix_kernels_bytes.json.  --rates <stats.csv> then turns rocprofv3's kernel_stats into a table per kernel (mean,
min .. max per dispatch, bytes over kernel time, share of the 8.0 TB/s HBM peak) in <out-dir>/layer_mix_kernel_rates_T<shapes>.txt
(no GPU needed); one --kernels run per shape keeps the shapes apart."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12               # bytes / s, spec
HBM_COPY = 6.29e12              # bytes / s, a float4 copy as measured on this chip

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=os.path.join("profiles", "r29"))
ap.add_argument("--ks", default="1,3,16")
ap.add_argument("--shapes", default="4378,20000", help="sequence lengths T; the batch is --batch x T x --width")
ap.add_argument("--steps", type=int, default=20, help="group steps per timed window of route B")
ap.add_argument("--a-steps", type=int, default=None, help="group steps per timed window of route A (default: --steps)")
ap.add_argument("--layers", type=int, default=13)
ap.add_argument("--width", type=int, default=768)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--pool", type=int, default=4, help="sequences in the store")
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--kernel-reps", type=int, default=10)
ap.add_argument("--rates", default=None, help="kernel_stats.csv of a rocprofv3 run of --kernels")
args = ap.parse_args()
a_steps = args.a_steps or args.steps
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def write_lines(name):
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, name), "w") as f:
        f.write("\n".join(lines) + "\n")


def kernel_bytes(T):
    """Bytes per launch of one batch, counted from the shapes (every member has all T frames)."""
    pos = args.batch * T * args.width * 4
    return {"collate_mix_group_kernel": (args.layers + 1) * pos, "layer_mix_fwd_kernel": (args.layers + 1) * pos,
            "collate_mix_bwd_partial_kernel": (args.layers + 1) * pos, "layer_mix_bwd_partial_kernel": (args.layers + 1) * pos,
            "collate_pad_group_kernel": 2 * pos}


if args.rates:
    with open(os.path.join(args.out_dir, "layer_mix_kernels_bytes.json")) as f:
        meta = json.load(f)
    with open(args.rates) as f:
        stats = list(csv.DictReader(f))
    say(f"# kernel rates from rocprofv3 --kernel-trace --stats ({os.path.basename(args.rates)}): bytes counted from the shapes over the "
        f"kernel's total time; {meta['reps']} launches per kernel and shape, L = {meta['layers']}, batch {meta['batch']} x T x {meta['width']}")
    say("# per dispatch in microseconds: mean (min .. max); the rate is the bytes of all dispatches over their total time")
    for r in sorted(stats, key=lambda r: r["Name"]):
        name = r["Name"]
        short = name.split("(")[0].split("::")[-1]
        for key in meta["bytes_total"]:
            if key in name:
                b, ns = meta["bytes_total"][key], float(r["TotalDurationNs"])
                say(f"{short:36s} calls {int(r['Calls']):3d}  {float(r['AverageNs']) / 1e3:8.1f} ({float(r['MinNs']) / 1e3:.1f} .. {float(r['MaxNs']) / 1e3:.1f})  "
                    f"{b / ns * 1e9 / 1e12:5.2f} TB/s = {100 * b / ns * 1e9 / HBM_PEAK:3.0f} % of the 8.0 TB/s peak "
                    f"({100 * b / ns * 1e9 / HBM_COPY:3.0f} % of a measured float4 copy)")
        if "_bwd_final_kernel" in name:
            say(f"{short:36s} calls {int(r['Calls']):3d}  {float(r['AverageNs']) / 1e3:8.1f} ({float(r['MinNs']) / 1e3:.1f} .. {float(r['MaxNs']) / 1e3:.1f})")
    write_lines(f"layer_mix_kernel_rates_T{meta['shapes'].replace(',', '_')}.txt")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from robust_speech_analysis_framework_amd import _lib  # noqa: E402
from robust_speech_analysis_framework_amd.cnnlstm import (CNNLSTM, DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore,  # noqa: E402
                                                          FusedAdam, cnnlstm_train_group, collate_batches, train_replicas_lockstep)
from robust_speech_analysis_framework_amd.layer_mix import LayerMix, layer_mix_backward, layer_mix_forward  # noqa: E402
from robust_speech_analysis_framework_amd.layer_mix_train import collate_mix_backward, collate_mix_forward  # noqa: E402

_lib.load()
_lib.require_gpu()


def make_pool(T):
    """--pool stacks [L, T, width] (windows of one random block) and their labels."""
    rng = np.random.Generator(np.random.PCG64(29))
    block = rng.standard_normal((args.layers, T + args.pool, args.width), dtype=np.float32)
    return [np.ascontiguousarray(block[:, i:i + T]) for i in range(args.pool)], rng.integers(0, 2, args.pool)


def run_kernels():
    total = {}
    for T in [int(t) for t in args.shapes.split(",")]:
        pool, labels = make_pool(T)
        store = DeviceSequenceStore(pool, layers=args.layers)
        plain = DeviceSequenceStore([s[0] for s in pool])
        loader = DeviceBatchLoader(DeviceSequenceDataset(store, labels), batch_size=args.batch)
        plan = next(loader.plans())
        plain_plan = next(DeviceBatchLoader(DeviceSequenceDataset(plain, labels), batch_size=args.batch).plans())
        h = next(iter(loader))[0]
        p = torch.softmax(torch.linspace(-1, 1, args.layers, device="cuda"), 0).contiguous()
        dx = 1e-3 * torch.randn((args.batch, T, args.width), device="cuda")
        for rep in range(args.kernel_reps + 1):                 # the first round is the warm-up and is in the trace too
            collate_mix_forward([plan], [p])
            layer_mix_forward(h, p)
            collate_mix_backward([plan], [dx])
            layer_mix_backward(h, dx)
            collate_batches([plain_plan])
        torch.cuda.synchronize()
        for k, b in kernel_bytes(T).items():
            total[k] = total.get(k, 0) + b * (args.kernel_reps + 1)
        # the padded stack itself comes from collate_pad_group_kernel once: B * L members
        total["collate_pad_group_kernel"] += 2 * args.layers * args.batch * T * args.width * 4
        del store, plain, h
        torch.cuda.empty_cache()
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "layer_mix_kernels_bytes.json"), "w") as f:
        json.dump({"reps": args.kernel_reps + 1, "layers": args.layers, "batch": args.batch, "width": args.width, "shapes": args.shapes,
                   "bytes_total": total}, f, indent=1)
        f.write("\n")
    print("kernels done", flush=True)


if args.kernels:
    run_kernels()
    sys.exit(0)


def replicas(K, own_mix):
    torch.manual_seed(0)
    models = [CNNLSTM(input_dim=args.width).to("cuda").train() for _ in range(K)]
    mixes = [LayerMix(args.layers).cuda() for _ in range(K)]
    if own_mix:
        return models, mixes, [FusedAdam(m, lr=1e-4, layer_mix=x, layer_mix_lr=1e-3) for m, x in zip(models, mixes)], None
    return models, mixes, [FusedAdam(m, lr=1e-4) for m in models], [torch.optim.Adam([x.weights], lr=1e-3) for x in mixes]


def route_a(models, mixes, opts, mix_opts, pool, labels, steps):
    """Per group step and replica: host stack, upload, LayerMix -> model -> loss -> backward -> both optimizers."""
    loss_fn = torch.nn.CrossEntropyLoss()
    rng = np.random.Generator(np.random.PCG64(7))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        for m, x, o, xo in zip(models, mixes, opts, mix_opts):
            idx = rng.integers(0, len(pool), args.batch)
            h = torch.from_numpy(np.stack([pool[i] for i in idx])).to("cuda")          # all members have T frames: no padding to add
            lab = torch.from_numpy(labels[idx]).to("cuda")
            o.zero_grad()
            xo.zero_grad()
            out, = cnnlstm_train_group([m], [x(h)])
            loss_fn(out, lab).backward()
            o.step()
            xo.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def route_b(models, mixes, opts, store, labels, steps):
    idx = np.tile(np.arange(len(store)), steps * args.batch // len(store) + 1)[:steps * args.batch]
    ds = DeviceSequenceDataset(store, labels, indices=idx)
    loaders = [DeviceBatchLoader(ds, batch_size=args.batch, shuffle=True, generator=torch.Generator().manual_seed(1000 + k))
               for k in range(len(models))]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train_replicas_lockstep(models, opts, loaders, torch.nn.CrossEntropyLoss(), 1, "cuda", mixes=mixes)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def spread(pair):
    return abs(pair[0] - pair[1])


rows = []
say(f"# tools/layer_mix_feed_bench.py --ks {args.ks} --shapes {args.shapes} --steps {args.steps} --a-steps {a_steps} --layers {args.layers}: one "
    f"MI355X; per row both routes warmed, then A / B / A / B; a window is {a_steps} (A) or {args.steps} (B) group steps of batch {args.batch}")
for T in [int(t) for t in args.shapes.split(",")]:
    pool, labels = make_pool(T)
    store = DeviceSequenceStore(pool, layers=args.layers)
    torch.cuda.synchronize()
    stack = args.batch * args.layers * T * args.width * 4
    say(f"== T={T}: store of {len(pool)} stacks [{args.layers}, {T}, {args.width}], {store.nbytes / 2**30:.2f} GiB, resident")
    for K in [int(k) for k in args.ks.split(",")]:
        ma, xa, oa, xoa = replicas(K, False)
        mb, xb, ob, _ = replicas(K, True)
        route_a(ma, xa, oa, xoa, pool, labels, 1)
        route_b(mb, xb, ob, store, labels, 2)
        a, b = [], []
        for _ in range(2):
            a.append(route_a(ma, xa, oa, xoa, pool, labels, a_steps))
            b.append(route_b(mb, xb, ob, store, labels, args.steps))
        _lib.prof_begin()
        route_b(mb, xb, ob, store, labels, args.steps)
        prof = _lib.prof_end()
        fam = {k: prof[k] for k in ("train_collate_mix", "train_collate_mix_backward", "layer_mix_adam")}
        a_mean, b_mean = sum(a) / 2, sum(b) / 2
        parts = int(_lib.load().rsaf_layer_mix_partials(args.batch, args.layers, T, args.width))
        rec = {"T": T, "K": K, "layers": args.layers, "a_ms_per_group_step": a, "b_ms_per_group_step": b, "a_steps_per_window": a_steps,
               "b_steps_per_window": args.steps, "a_spread_ms": spread(a), "b_spread_ms": spread(b), "a_over_b": a_mean / b_mean,
               "counted_peak_intermediate_bytes": {"a_one_replica_at_a_time": stack, "a_if_grouped": K * stack, "b": K * parts * 8},
               "launches_per_group_step": {k: v["launches"] / args.steps for k, v in fam.items()},
               "event_ms_per_launch": {k: v["ms"] / max(v["launches"], 1) for k, v in fam.items()}}
        rows.append(rec)
        say(f"T={T:6d} K={K:2d}: A {a[0]:10.2f} / {a[1]:10.2f} ms per group step (spread {spread(a):.2f}), B {b[0]:9.2f} / {b[1]:9.2f} "
            f"(spread {spread(b):.2f}), A / B = {a_mean / b_mean:.2f}")
        say(f"            peak intermediates, counted: A {stack / 1e9:.2f} GB of padded stack per replica in flight ({K * stack / 1e9:.1f} GB if the "
            f"K stacks of a group step were held together), B {K * parts * 8 / 1e3:.0f} kB of partial sums and no stack")
        say("            launches per group step of B: " + ", ".join(f"{k} {v['launches'] / args.steps:g}" for k, v in fam.items())
            + "; device-event ms per launch: " + ", ".join(f"{k} {v['ms'] / max(v['launches'], 1):.3f}" for k, v in fam.items()))
        del ma, xa, oa, xoa, mb, xb, ob
        torch.cuda.empty_cache()
    del store, pool
    torch.cuda.empty_cache()
os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "layer_mix_feed.json"), "w") as f:
    json.dump({"windows": "A/B/A/B", "rows": rows}, f, indent=1)
    f.write("\n")
write_lines("layer_mix_feed.txt")
