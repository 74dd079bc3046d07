"""What the input gradient of the CNN-LSTM training step costs, and what the layer mix in front of it moves.

step  One training step (rsaf_cnnlstm_train_forward + backward) of the shipped model (D 768, C 128, H 128, two layers, no
      dropout masks) at --batch x T x 768, through the C entries so that two builds of the library can run side by side:
          with_dx  backward by rsaf_cnnlstm_train_backward_dx
          without  backward by rsaf_cnnlstm_train_backward of this build
          parent   the same by another build of the library (--parent-lib, the parent commit's librsaf.so), if given
      Every variant is warmed up, then the windows run with_dx / without / parent twice in that order (A / B / A / B), each
      --reps steps between two device events.  From shapes the input gradient adds 2 B T D 4C FLOP (the k = 3 and the 1x1
      data-gradient GEMM) and one B T D float store.
mix   LayerMix forward and backward (rsaf_layer_mix_forward / _backward) at L = --layers over the same shapes: kernel ms per
      call out of rsaf_prof, bytes = (L + 1) n 4 each way from shapes, and the share of the HBM peak.  For kernel times by
      name run this part alone under `rocprofv3 --kernel-trace --stats`.

    python tools/input_grad_bench.py [--part step,mix] [--shapes 4378,20000] [--reps 10] [--parent-lib PATH] [--out-dir profiles/r27]
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from robust_speech_analysis_framework_amd import _lib
from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, _pack_train_blob

HBM_PEAK = 8.0e12               # bytes / s, spec

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="step,mix")
ap.add_argument("--out-dir", default=os.path.join("profiles", "r27"))
ap.add_argument("--shapes", default="4378,20000", help="sequence lengths T; a batch is --batch x T x 768")
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--layers", type=int, default=13)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--parent-lib", default=None, help="librsaf.so of the parent commit, for the third timing of the step")
args = ap.parse_args()
lib = _lib.load()
_lib.require_gpu()
STEP_ENTRIES = ("rsaf_cnnlstm_train_forward", "rsaf_cnnlstm_train_backward")
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    for name in STEP_ENTRIES:
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
lines = []
D, CH, H, NC, LAYERS, ACT = 768, 128, 128, 2, 2, 2


def say(text):
    print(text, flush=True)
    lines.append(text)


def new(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device="cuda")


def timed(fn):
    """ms per call of `fn`, --reps calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.reps


def step_variants(B, T):
    model = CNNLSTM().cuda().train()
    blob = _pack_train_blob(model, "cuda")[1]
    sizes = (B, T, D, CH, H, LAYERS)
    x = torch.randn((B, T, D), device="cuda")
    saved, scratch = new(int(lib.rsaf_cnnlstm_train_saved_floats(*sizes))), new(int(lib.rsaf_cnnlstm_train_scratch_floats(*sizes)))
    logits, dlogits, grads = new(B, NC), torch.full((B, NC), 0.1, device="cuda"), torch.zeros_like(blob)
    dx, dx_scr = new(B, T, D), new(int(lib.rsaf_cnnlstm_train_dx_scratch_floats(D, CH)))
    head = (_lib.ptr(x), B, T, D, CH, H, NC, LAYERS, ACT, _lib.ptr(blob), None, None, None, None, _lib.ptr(saved), saved.numel(),
            _lib.ptr(scratch), scratch.numel())
    keep = [model, blob, x, saved, scratch, logits, dlogits, grads, dx, dx_scr]

    def step(library, with_dx):
        def run():
            s = _lib.stream_ptr(None)
            _lib.check(library.rsaf_cnnlstm_train_forward(*head, _lib.ptr(logits), None, s), "forward")
            if with_dx:
                _lib.check(library.rsaf_cnnlstm_train_backward_dx(*head, _lib.ptr(dlogits), _lib.ptr(grads), _lib.ptr(dx), _lib.ptr(dx_scr),
                                                                  dx_scr.numel(), s), "backward_dx")
            else:
                _lib.check(library.rsaf_cnnlstm_train_backward(*head, _lib.ptr(dlogits), _lib.ptr(grads), s), "backward")
        return run

    out = {"with_dx": step(lib, True), "without": step(lib, False)}
    if parent is not None:
        out["parent"] = step(parent, False)
    return out, keep


def bench_step():
    say(f"# step: one MI355X; ms per training step (forward + backward, C entries) of D {D}, C {CH}, H {H}, {LAYERS} layers at "
        f"{args.batch} x T x {D}; {args.reps} steps per window between device events, every variant warmed up, then two rounds "
        f"with_dx / without{' / parent' if parent is not None else ''}")
    for T in [int(t) for t in args.shapes.split(",")]:
        vs, keep = step_variants(args.batch, T)
        for run in vs.values():
            run()
        torch.cuda.synchronize()
        ms = {name: [] for name in vs}
        for _ in range(2):
            for name, run in vs.items():
                ms[name].append(timed(run))
        mean = {k: sum(v) / 2 for k, v in ms.items()}
        spread = {k: abs(v[0] - v[1]) for k, v in ms.items()}
        flop = 2.0 * args.batch * T * D * 4 * CH
        say(f"T={T:6d}: the input gradient adds {flop / 1e9:.1f} GFLOP and one {args.batch * T * D * 4 / 1e6:.0f} MB store (from shapes)")
        for name in vs:
            say(f"    {name:8s} {ms[name][0]:9.3f} / {ms[name][1]:9.3f} ms (spread {spread[name]:.3f})")
        text = (f"    with_dx - without = {mean['with_dx'] - mean['without']:+.3f} ms ({100 * (mean['with_dx'] / mean['without'] - 1):+.1f} %): "
                f"{flop / max(mean['with_dx'] - mean['without'], 1e-9) / 1e9:.1f} TFLOP/s over the added time")
        if parent is not None:
            text += (f"; without / parent = {mean['without'] / mean['parent']:.4f} (difference {mean['without'] - mean['parent']:+.3f} ms "
                     f"against a spread of {max(spread['without'], spread['parent']):.3f})")
        say(text)
        del vs, keep
        torch.cuda.empty_cache()


def bench_mix():
    L = args.layers
    say(f"# mix: one MI355X; kernel ms per call out of rsaf_prof, L = {L}, {args.reps} calls per window, warmed up, two rounds forward / "
        f"backward; bytes = (L + 1) n 4 from shapes; share of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak")
    for T in [int(t) for t in args.shapes.split(",")]:
        B = args.batch
        h = torch.randn((B, L, T, D), device="cuda")
        p = torch.softmax(torch.randn(L, device="cuda"), 0)
        x, dx, dp = new(B, T, D), torch.randn((B, T, D), device="cuda"), new(L)
        n_part = int(lib.rsaf_layer_mix_partials(B, L, T, D))
        partials = new(n_part, dtype=torch.float64)
        nbytes = (L + 1) * B * T * D * 4

        def fwd():
            _lib.check(lib.rsaf_layer_mix_forward(_lib.ptr(h), B, L, T, D, _lib.ptr(p), _lib.ptr(x), _lib.stream_ptr(None)), "forward")

        def bwd():
            _lib.check(lib.rsaf_layer_mix_backward(_lib.ptr(h), _lib.ptr(dx), B, L, T, D, _lib.ptr(partials), n_part, _lib.ptr(dp),
                                                   _lib.stream_ptr(None)), "backward")

        vs = {"layer_mix_forward": fwd, "layer_mix_backward": bwd}
        for run in vs.values():
            run()
        torch.cuda.synchronize()
        ms = {name: [] for name in vs}
        for _ in range(2):
            for name, run in vs.items():
                _lib.prof_begin()
                for _ in range(args.reps):
                    run()
                torch.cuda.synchronize()
                rec = _lib.prof_end()[name]
                assert rec["launches"] == args.reps
                ms[name].append(rec["ms"] / rec["launches"])
        say(f"T={T:6d}: {nbytes / 1e6:.0f} MB per call, {n_part // L} parts in the backward")
        for name in vs:
            mean = sum(ms[name]) / 2
            say(f"    {name:18s} {ms[name][0]:8.4f} / {ms[name][1]:8.4f} ms (spread {abs(ms[name][0] - ms[name][1]):.4f}), "
                f"{nbytes / (mean * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (mean * 1e-3) / HBM_PEAK:3.0f} % of the peak")
        del h, x, dx, partials
        torch.cuda.empty_cache()


parts = args.part.split(",")
if "step" in parts:
    bench_step()
if "mix" in parts:
    bench_mix()
os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "input_grad_" + "_".join(parts) + ".txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
