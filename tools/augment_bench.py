"""What the augmentations cost inside the collate launch: one launch of K batches of 4 x T x 768 out of one DeviceSequenceStore
(distinct sequences for every member, all of the full length T), assembled

    full    by rsaf_collate_augment_group with the pipeline [Scale, GaussianNoise(p=1), TimeMask, FeatureMask], every op at p = 1
            so that every member pays for all of it (the noise is the expensive one);
    n_ops0  by the same entry with n_ops = 0: the plain copy through the new kernel;
    plain   by rsaf_collate_pad_group of this build;
    parent  by rsaf_collate_pad_group of another build of the library (--parent-lib, the parent commit's librsaf.so), if given.

The items are built once per variant over preallocated outputs, all variants are warmed up, then the windows run
full / n_ops0 / plain / parent twice in that order (A / B / A / B), each window --reps launches under rsaf_prof of the library
that launches: the figure is kernel ms per launch, and bytes (floats read + written, times four) per second.

    python tools/augment_bench.py [--out-dir profiles/r25] [--ks 1,16] [--shapes 4378,20000] [--reps 20] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from robust_speech_analysis_framework_amd import _lib
from robust_speech_analysis_framework_amd.cnnlstm import (Compose, DeviceSequenceStore, FeatureMask, GaussianNoise, Scale, TimeMask)

HBM_PEAK = 8.0e12               # bytes / s, spec

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=os.path.join("profiles", "r25"))
ap.add_argument("--ks", default="1,16")
ap.add_argument("--shapes", default="4378,20000", help="sequence lengths T; a batch is --batch x T x --width")
ap.add_argument("--width", type=int, default=768)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--parent-lib", default=None, help="librsaf.so of the parent commit, for the fourth timing")
args = ap.parse_args()
lib = _lib.load()
_lib.require_gpu()
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    for name in ("rsaf_collate_pad_group", "rsaf_prof_begin", "rsaf_prof_end"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def profiled(library, fn, family):
    """(kernel ms per launch, bytes per launch) of the launches `fn` issues, out of `library`'s own rsaf_prof."""
    _lib.check(library.rsaf_prof_begin(), "rsaf_prof_begin")
    fn()
    torch.cuda.synchronize()
    recs, n = (_lib.ProfRecord * 64)(), C.c_int(0)
    _lib.check(library.rsaf_prof_end(recs, 64, C.byref(n)), "rsaf_prof_end")
    rec = {r.name.decode(): r for r in recs[:n.value]}[family]
    assert rec.launches == args.reps, (family, rec.launches)
    return rec.ms / rec.launches, rec.bytes / rec.launches


def variants(store, K, T):
    """name -> (library, family, launch): the K batches of one group step, members 4 k .. 4 k + 3 of the store in batch k."""
    B, width = args.batch, store.width
    idx = torch.arange(K * B, dtype=torch.int64, device="cuda")
    start = store.frame_off_device[idx].contiguous()
    count = (store.frame_off_device[idx + 1] - start).to(torch.int32).contiguous()
    outs = [torch.empty((B, T, width), dtype=torch.float32, device="cuda") for _ in range(K)]
    full = Compose([Scale(0.5, 1.5, p=1.0), GaussianNoise(p=1.0), TimeMask(p=1.0), FeatureMask(p=1.0)])
    keep = [idx, start, count, outs, full, full.table("cuda")]

    def items(kind, transform):
        arr = (kind * K)()
        for k, it in enumerate(arr):
            it.arena, it.arena_rows = store.arena.data_ptr(), int(store.arena.shape[0])
            it.row_start, it.row_count = start.data_ptr() + 8 * B * k, count.data_ptr() + 4 * B * k
            it.B, it.T, it.out, it.frames = B, T, outs[k].data_ptr(), B * T
            if transform is not None:
                it.ops, it.ops_host, it.n_ops = transform.table("cuda").data_ptr(), C.addressof(transform.table_host), len(transform)
                it.seed, it.epoch, it.sample_id = 25, 0, idx.data_ptr() + 8 * B * k
        return arr

    def launcher(library, entry, arr):
        fn = getattr(library, entry)

        def launch():
            for _ in range(args.reps):
                _lib.check(fn(arr, K, width, _lib.stream_ptr(None)), entry)
        return launch

    out = {"full": (lib, "train_collate_augment", launcher(lib, "rsaf_collate_augment_group", items(_lib.CollateAugmentItem, full))),
           "n_ops0": (lib, "train_collate_augment", launcher(lib, "rsaf_collate_augment_group", items(_lib.CollateAugmentItem, None))),
           "plain": (lib, "train_collate", launcher(lib, "rsaf_collate_pad_group", items(_lib.CollateItem, None)))}
    if parent is not None:
        out["parent"] = (parent, "train_collate", launcher(parent, "rsaf_collate_pad_group", items(_lib.CollateItem, None)))
    return out, keep


say(f"# tools/augment_bench.py --ks {args.ks} --shapes {args.shapes} --reps {args.reps}: one MI355X; kernel ms per launch of K batches "
    f"{args.batch} x T x {args.width} out of rsaf_prof, every variant warmed up, then two rounds full / n_ops0 / plain"
    f"{' / parent' if parent is not None else ''}; TB/s = floats read + written, times four, per second")
rows = []
for T in [int(t) for t in args.shapes.split(",")]:
    for K in [int(k) for k in args.ks.split(",")]:
        n = K * args.batch
        arena = torch.randn((n * T, args.width), dtype=torch.float32, device="cuda")
        store = DeviceSequenceStore._from_arena(arena, np.full(n, T, dtype=np.int64))
        vs, keep = variants(store, K, T)
        for _, _, launch in vs.values():
            launch()
        torch.cuda.synchronize()
        ms, nbytes = {name: [] for name in vs}, 0
        for _ in range(2):
            for name, (library, family, launch) in vs.items():
                t, nbytes = profiled(library, launch, family)
                ms[name].append(t)
        mean = {name: sum(v) / 2 for name, v in ms.items()}
        spread = {name: abs(v[0] - v[1]) for name, v in ms.items()}
        say(f"T={T:6d} K={K:2d} ({nbytes / 1e6:.0f} MB read + written per launch):")
        for name in vs:
            say(f"    {name:7s} {ms[name][0]:8.4f} / {ms[name][1]:8.4f} ms (spread {spread[name]:.4f}), {nbytes / (mean[name] * 1e-3) / 1e12:5.2f} TB/s "
                f"= {100 * nbytes / (mean[name] * 1e-3) / HBM_PEAK:3.0f} % of the 8.0 TB/s peak")
        text = f"    full / plain = {mean['full'] / mean['plain']:.2f}, n_ops0 / plain = {mean['n_ops0'] / mean['plain']:.3f}"
        if parent is not None:
            text += (f", plain / parent = {mean['plain'] / mean['parent']:.3f} (difference {mean['plain'] - mean['parent']:+.4f} ms against a "
                     f"spread of {max(spread['plain'], spread['parent']):.4f})")
        say(text)
        rows.append({"T": T, "K": K, "bytes_per_launch": nbytes, "ms_per_launch": ms})
        del vs, keep, store, arena
        torch.cuda.empty_cache()
os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "augment.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
