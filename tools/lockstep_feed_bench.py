"""What feeding costs a lock-step epoch: fused lock-step training (FusedAdam + nn.CrossEntropyLoss, train_replicas_lockstep)
of K CNN-LSTM replicas at the shapes of tools/train_group_bench.py, fed

    A  by DataLoader(num_workers=0) over host arrays with the reference's SequenceDataset / collate_fn arithmetic
       (torch.FloatTensor(seq.copy()), pad_sequence) and the loop's pageable .to(device): the path before device loaders;
    B  by DeviceBatchLoader over one DeviceSequenceStore: the K batches of a group step from one rsaf_collate_pad_group launch.

Every replica draws from the same pool of sequences (its own shuffled order), as every fold of every trial draws from one
sequences_dict.  All sequences have the full length T, so a batch is exactly B x T x 768 as in train_group_bench.py.
Both paths are warmed up at the timed shapes; then the windows run A / B / A / B in one process, each one epoch of
--steps group steps, timed with a host clock around work that ends in a synchronise.  A further B epoch under
rsaf_prof gives the train_collate time and its bytes (floats read + written, times four) per second as a share of the
HBM peak; the same batches through aggregate.pad_batch_device (host-built int64 row index + the gather_rows kernel)
and through one-item collate calls, alternating, compare the two kernels on the same bytes.

    python tools/lockstep_feed_bench.py [--out-dir profiles/r24] [--ks 1,3,16] [--steps 20] [--shapes 4378,20000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import DataLoader, Dataset

from robust_speech_analysis_framework_amd import _lib
from robust_speech_analysis_framework_amd.aggregate import pad_batch_device
from robust_speech_analysis_framework_amd.cnnlstm import (CNNLSTM, DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore,
                                                          FusedAdam, collate_batches, train_replicas_lockstep)

HBM_PEAK = 8.0e12               # bytes / s, spec
HBM_COPY = 6.29e12              # bytes / s, a float4 copy as measured on this chip

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=os.path.join("profiles", "r24"))
ap.add_argument("--ks", default="1,3,16")
ap.add_argument("--shapes", default="4378,20000", help="sequence lengths T; the batch is 4 x T x --width")
ap.add_argument("--steps", type=int, default=20, help="group steps per timed window (= batches per epoch)")
ap.add_argument("--width", type=int, default=768)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--kernel-reps", type=int, default=10)
args = ap.parse_args()
_lib.load()
_lib.require_gpu()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


class HostSequences(Dataset):
    """SequenceDataset of the reference without a transform: a copy and a cast per item."""

    def __init__(self, sequences, labels):
        self.sequences, self.labels = sequences, labels

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, i):
        return torch.FloatTensor(self.sequences[i].copy()), torch.tensor(self.labels[i])


def host_collate(batch):
    seqs, labels = zip(*batch)
    return pad_sequence(seqs, batch_first=True, padding_value=0), torch.stack(labels)


def make_pool(T, n):
    """n float32 sequences [T, width] (windows of one random block: distinct values, cheap to make) and their labels."""
    rng = np.random.Generator(np.random.PCG64(24))
    block = rng.standard_normal((T + n, args.width), dtype=np.float32)
    return [block[i:i + T].copy() for i in range(n)], rng.integers(0, 2, n)


def replicas(K):
    torch.manual_seed(0)
    models = [CNNLSTM(input_dim=args.width).to("cuda").train() for _ in range(K)]
    return models, [FusedAdam(m, lr=1e-4) for m in models]


def epoch(models, opts, loaders):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train_replicas_lockstep(models, opts, loaders, torch.nn.CrossEntropyLoss(), 1, "cuda")
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_compare(store, T):
    """The collate kernel (one item) and pad_batch_device (host index + gather_rows) on the same batches, alternating:
    kernel ms per batch out of rsaf_prof, two rounds each for the spread; wall ms per batch for pad_batch_device."""
    dataset = DeviceSequenceDataset(store, np.zeros(len(store), dtype=np.int64))
    plans = list(DeviceBatchLoader(dataset, batch_size=args.batch).plans())[:args.kernel_reps]
    members = [[int(i) for i in dataset.indices[k * args.batch:(k + 1) * args.batch]] for k in range(len(plans))]

    def collate_round():
        for p in plans:
            collate_batches([p])

    def gather_round():
        for m in members:
            pad_batch_device(store.arena, store.frame_off, [[i] for i in m])

    collate_round(), gather_round()                       # warm-up
    torch.cuda.synchronize()
    out = {"collate_ms": [], "gather_ms": [], "gather_wall_ms": [], "collate_wall_ms": []}
    for _ in range(2):
        for name, family, fn in (("collate", "train_collate", collate_round), ("gather", "gather_rows", gather_round)):
            _lib.prof_begin()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            prof = _lib.prof_end()
            assert prof[family]["launches"] == len(plans), prof
            out[f"{name}_ms"].append(prof[family]["ms"] / len(plans))
            out[f"{name}_wall_ms"].append(wall * 1e3 / len(plans))
    out["batch_bytes_read_and_written"] = 2 * args.batch * T * args.width * 4
    return out


def spread(pair):
    return abs(pair[0] - pair[1])


def row(T, K, pool, labels, store):
    n = len(pool)
    host = HostSequences(pool, labels)
    dev = DeviceSequenceDataset(store, labels)
    gen = lambda k: torch.Generator().manual_seed(1000 + k)                                 # noqa: E731
    loaders_a = lambda idx=None: [DataLoader(host if idx is None else torch.utils.data.Subset(host, idx), batch_size=args.batch,  # noqa: E731
                                             shuffle=True, collate_fn=host_collate, num_workers=0, generator=gen(k)) for k in range(K)]
    loaders_b = lambda idx=None: [DeviceBatchLoader(dev if idx is None else dev.subset(idx), batch_size=args.batch, shuffle=True,  # noqa: E731
                                                    generator=gen(k)) for k in range(K)]
    models, opts = replicas(K)
    warm = list(range(2 * args.batch))
    epoch(models, opts, loaders_a(warm))
    epoch(models, opts, loaders_b(warm))
    a, b = [], []
    for _ in range(2):
        a.append(epoch(models, opts, loaders_a()) * 1e3 / args.steps)
        b.append(epoch(models, opts, loaders_b()) * 1e3 / args.steps)
    _lib.prof_begin()
    epoch(models, opts, loaders_b())
    prof = _lib.prof_end()
    col = prof["train_collate"]
    assert col["launches"] == args.steps, col
    rate = col["bytes"] / (col["ms"] * 1e-3)
    gpu_ms = sum(v["ms"] for v in prof.values()) / args.steps
    a_mean, b_mean = sum(a) / 2, sum(b) / 2
    rec = {"T": T, "K": K, "batch": args.batch, "width": args.width, "steps_per_window": args.steps, "pool_sequences": n,
           "a_ms_per_group_step": a, "b_ms_per_group_step": b, "a_spread_ms": spread(a), "b_spread_ms": spread(b),
           "a_over_b": a_mean / b_mean, "b_no_slower_than_a_beyond_spread": b_mean <= a_mean + spread(a),
           "gpu_ms_per_group_step_all_families": gpu_ms, "host_share_of_a": 1.0 - gpu_ms / a_mean,
           "train_collate": {"launches_per_step": col["launches"] / args.steps, "ms_per_launch": col["ms"] / col["launches"],
                             "bytes_per_launch": col["bytes"] / col["launches"], "bytes_per_s": rate,
                             "share_of_hbm_peak_8.0TBs": rate / HBM_PEAK, "share_of_measured_copy_6.29TBs": rate / HBM_COPY}}
    say(f"T={T:6d} K={K:2d}: A {a[0]:9.2f} / {a[1]:9.2f} ms per group step (spread {spread(a):.2f}), B {b[0]:9.2f} / {b[1]:9.2f} "
        f"(spread {spread(b):.2f}), A / B = {a_mean / b_mean:.2f}; kernels of a B step {gpu_ms:.2f} ms, so {100 * (1 - gpu_ms / a_mean):.0f} % "
        f"of an A step is feeding and host")
    say(f"            train_collate: {col['ms'] / col['launches']:.3f} ms per launch of {K} batches, {col['bytes'] / col['launches'] / 1e6:.0f} MB "
        f"read + written, {rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f} % of the 8.0 TB/s peak ({100 * rate / HBM_COPY:.0f} % of a measured float4 copy)")
    del models, opts
    torch.cuda.empty_cache()
    return rec


rows, kernels = [], []
say(f"# tools/lockstep_feed_bench.py --ks {args.ks} --shapes {args.shapes} --steps {args.steps}: one MI355X; per row both paths "
    f"warmed up (2 group steps), then A / B / A / B, each window one epoch of {args.steps} group steps of batch {args.batch}")
for T in [int(t) for t in args.shapes.split(",")]:
    pool, labels = make_pool(T, args.steps * args.batch)
    t0 = time.perf_counter()
    store = DeviceSequenceStore(pool)
    torch.cuda.synchronize()
    say(f"== T={T}: pool of {len(pool)} sequences, {store.nbytes / 2**30:.2f} GiB, uploaded once in {time.perf_counter() - t0:.2f} s")
    kc = kernel_compare(store, T)
    c, g = sum(kc["collate_ms"]) / 2, sum(kc["gather_ms"]) / 2
    kc.update(T=T, collate_no_slower_than_gather_beyond_spread=c <= g + spread(kc["collate_ms"]), gather_over_collate=g / c)
    kernels.append(kc)
    say(f"   one batch 4 x {T} x {args.width} ({kc['batch_bytes_read_and_written'] / 1e6:.0f} MB read + written): collate kernel "
        f"{kc['collate_ms'][0]:.3f} / {kc['collate_ms'][1]:.3f} ms, gather_rows kernel {kc['gather_ms'][0]:.3f} / {kc['gather_ms'][1]:.3f} ms "
        f"(gather / collate = {g / c:.2f}); wall per batch: collate_batches {sum(kc['collate_wall_ms']) / 2:.3f} ms, "
        f"pad_batch_device with its host-built index {sum(kc['gather_wall_ms']) / 2:.3f} ms")
    for K in [int(k) for k in args.ks.split(",")]:
        rows.append(row(T, K, pool, labels, store))
    del store, pool
    torch.cuda.empty_cache()
ok_rows = all(r["b_no_slower_than_a_beyond_spread"] for r in rows)
ok_kernel = all(k["collate_no_slower_than_gather_beyond_spread"] for k in kernels)
say(f"# B no slower than A beyond the A-to-A spread at every row: {ok_rows}; collate kernel no slower than gather_rows beyond its "
    f"own spread at every shape: {ok_kernel}")
os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "lockstep_feed.json"), "w") as f:
    json.dump({"steps_per_window": args.steps, "warmup_group_steps": 2, "windows": "A/B/A/B", "rows": rows, "kernel_on_one_batch": kernels,
               "b_no_slower_than_a": ok_rows, "collate_no_slower_than_gather_rows": ok_kernel}, f, indent=1)
    f.write("\n")
with open(os.path.join(args.out_dir, "lockstep_feed.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
