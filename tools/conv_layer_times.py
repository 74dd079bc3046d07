"""Time of every feature-encoder convolution GEMM inside the pipeline, from a rocprofv3 kernel trace.

  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python bench.py --config C3 --steps 2 --warmup 1
  python tools/conv_layer_times.py DIR [--clips 1000 --seconds 30 --windows 2048]

The gemm_f16x3 dispatches are labelled by their position in the forward call, as tools/pmc_traffic.py labels them (its
call_sequence is the replay); the convolutions are then split by window group.  Per group and layer: rows, mean time over
the traced steps and TFLOP/s-equivalent (2 x frames x C x K, junk rows not counted)."""
import argparse
import csv
import glob
import json
import os
import sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pmc_traffic as pt  # noqa: E402


def trace(root):
    files = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {root}")
    out = []
    for fn in files:
        with open(fn, newline="") as f:
            for r in csv.DictReader(f):
                if "gemm_f16x3_kernel" not in r["Kernel_Name"]:
                    continue
                v = pt.variant(r["Kernel_Name"])
                if v is not None and v[0] == "M":
                    continue
                out.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), v))
    out.sort()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--windows", type=int, default=2048)
    ap.add_argument("--conv-group", type=int, default=512)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    C = 512
    tr = trace(a.trace_dir)
    calls = pt.plan_calls(a.clips, a.seconds, a.windows)
    step = []                                              # (key or None, variant, flop)
    for ci, lens in enumerate(calls):
        seq, _ = pt.call_sequence(lens, conv_group=a.conv_group)
        n = len(lens)
        n_groups = -(-n // a.conv_group)
        gstep = -(-n // n_groups)
        k = 0
        for gi, g0 in enumerate(range(0, n, gstep)):
            grp = [pt.frames(l) for l in lens[g0:g0 + gstep]]
            for i in range(1, 7):
                kk = (3 if i <= 4 else 2) * C
                frames = sum(t[i] for t in grp)
                step.append(((ci, gi, i, len(grp), lens[g0], lens[min(g0 + gstep, n) - 1], frames), seq[k][1], 2.0 * frames * C * kk))
                k += 1
        step += [(None, var, 0.0) for _, var, _ in seq[k:]]
    per = len(step)
    n_steps = len(tr) // per
    agg = defaultdict(lambda: [0.0, 0, 0.0])
    mism = 0
    other = 0.0
    for j, (t0, t1, var) in enumerate(tr[:n_steps * per]):
        key, want, flop = step[j % per]
        mism += var != want
        if key is None:
            other += (t1 - t0) * 1e-6
            continue
        agg[key][0] += (t1 - t0) * 1e-6
        agg[key][1] += 1
        agg[key][2] = flop
    rows = []
    print(f"{len(tr)} dispatches, {per} per step, {n_steps} steps, {len(tr) - n_steps * per} left over, {mism} variant mismatches")
    tot = defaultdict(lambda: [0.0, 0.0])
    for key in sorted(agg):
        ms, cnt, flop = agg[key]
        ci, gi, i, nw, l0, l1, frames = key
        ms /= cnt
        tf = flop / (ms * 1e-3) / 1e12
        rows.append({"call": ci + 1, "group": gi + 1, "layer": f"conv{i}", "windows": nw, "longest": l0, "shortest": l1, "frames": frames,
                     "ms": round(ms, 3), "tflops_equivalent": round(tf, 1)})
        tot[i][0] += ms
        tot[i][1] += flop
        print(f"call {ci + 1} group {gi + 1} ({nw} windows of {l0}..{l1} samples) conv{i}: {frames:9d} frames {ms:8.3f} ms {tf:6.1f} TFLOP/s-eq")
    summ = {}
    for i in sorted(tot):
        summ[f"conv{i}"] = {"ms_per_step": round(tot[i][0], 2), "tflops_equivalent": round(tot[i][1] / (tot[i][0] * 1e-3) / 1e12, 1)}
    allms = sum(v[0] for v in tot.values())
    summ["conv1..6"] = {"ms_per_step": round(allms, 2), "tflops_equivalent": round(sum(v[1] for v in tot.values()) / (allms * 1e-3) / 1e12, 1)}
    summ["other w2v2_gemm dispatches"] = {"ms_per_step": round(other / max(n_steps, 1), 2)}
    print(json.dumps(summ))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"labelling": {"dispatches": len(tr), "per_step": per, "steps": n_steps, "variant_mismatches": int(mism)},
                       "per_step_summary": summ, "per_group_and_layer": rows}, f, indent=1)


if __name__ == "__main__":
    main()
