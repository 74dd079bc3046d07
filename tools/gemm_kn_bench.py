"""The B[K,N] instances of the fp32 MFMA GEMM at their production shapes, this tree's library against another build of it.

    python tools/gemm_kn_bench.py --other /path/to/other/librsaf.so [--this PATH] [--windows 4] [--iters 50]

Shapes: the two input-gradient GEMMs of a 4 x 4 378 x 768 CNN-LSTM training step (dgates . W_ih of LSTM layer 0 and
dy_sc . W_sc of the first residual block, cnnlstm_train.hip) and P . V of the three-launch attention (w2v2_encoder.hip:
64 windows x 12 heads, Tq = 249, lda = 256, the pad columns of P holding zeros so that both libraries may run it).
Windows alternate A / B / A / B ... in one process (A = the other library, B = this tree's or --this); each window warms up, then
times `iters` launches between two events.  Prints every window, the A-to-A spread and the difference of the means, and
checks that both libraries give the same bits."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from robust_speech_analysis_framework_amd import _lib  # noqa: E402


def _bind(path):
    lib = C.CDLL(path)
    res, args = _lib.SIGNATURES["rsaf_gemm_f32"]
    lib.rsaf_gemm_f32.restype, lib.rsaf_gemm_f32.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="librsaf.so of the build to compare against (window A)")
    ap.add_argument("--this", default=None, help="library of window B (default: this tree's)")
    ap.add_argument("--windows", type=int, default=4, help="windows in all, alternating A / B")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    _lib.require_gpu()
    libs = {"B": _lib.load(), "A": _bind(a.other)}              # _lib.load() first: it brings in torch's HIP runtime
    if a.this:
        libs["B"] = _bind(a.this)
    g = torch.Generator(device="cpu").manual_seed(0)
    Bt, T, D, Cc, H = 4, 4378, 768, 128, 128
    nw, NH, Tq, Tpq, hd = 64, 12, 249, 256, 64
    Hd = NH * hd
    shapes = []
    # (tag, M, N, K, lda, ldb, ldc, nz, nz2, strides, A, B, C)
    rows2 = Bt * (T // 2)
    shapes.append(("dgrad lstm l0   dgates.W_ih", rows2, Cc, 8 * H, 8 * H, Cc, Cc, 1, 1, None,
                   torch.randn((rows2, 8 * H), generator=g), torch.randn((8 * H, Cc), generator=g)))
    rows = Bt * T
    shapes.append(("dgrad shortcut  dy_sc.W_sc ", rows, D, Cc, Cc, D, D, 1, 1, None,
                   torch.randn((rows, Cc), generator=g), torch.randn((Cc, D), generator=g)))
    P = torch.zeros((nw, NH, Tq, Tpq))
    P[..., :Tq] = torch.softmax(torch.randn((nw, NH, Tq, Tq), generator=g), dim=-1)
    qkv = torch.randn((nw, Tq, 3 * Hd), generator=g)
    shapes.append(("attention P.V   Tq=249     ", Tq, hd, Tq, Tpq, 3 * Hd, Hd, nw * NH, NH,
                   [NH * Tq * Tpq, Tq * Tpq, Tq * 3 * Hd, hd, Tq * Hd, hd, 0, 0], P, qkv))
    print(f"windows {a.windows} (A = {a.other}, B = {a.this or 'this tree'}), {a.iters} launches per window, ms per launch")
    for tag, M, N, K, lda, ldb, ldc, nz, nz2, strides, hA, hB in shapes:
        dA, dB = hA.cuda(), hB.cuda()
        b_off = 2 * Hd if strides else 0
        st = (C.c_int64 * 8)(*strides) if strides else None
        out = {k: torch.zeros((nz // nz2 if strides else 1, M, ldc), device="cuda") for k in libs}

        def run(k):
            rc = libs[k].rsaf_gemm_f32(_lib.ptr(dA), _lib.c_void_p_off(dB, b_off), _lib.ptr(out[k]), None, None, M, N, K, lda, ldb,
                                       ldc, 0, nz, nz2, st, 0, 0, 1.0, 1, None)
            if rc != 0:
                raise RuntimeError(f"{tag}: library {k} returned {rc}")

        ms = {"A": [], "B": []}
        for w in range(a.windows):
            k = "AB"[w % 2]
            for _ in range(5):
                run(k)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.iters)
        same = torch.equal(out["A"], out["B"])
        ma, mb = sum(ms["A"]) / len(ms["A"]), sum(ms["B"]) / len(ms["B"])
        spread = max(ms["A"]) - min(ms["A"])
        tf = 2.0 * M * N * K * nz / 1e9
        print(f"{tag} M={M:6d} N={N:4d} K={K:5d} nz={nz:4d}  A " + " ".join(f"{v:.4f}" for v in ms["A"]) + "  B "
              + " ".join(f"{v:.4f}" for v in ms["B"]) + f"  mean A {ma:.4f} ({tf / ma:.1f} TFLOP/s) B {mb:.4f} ({tf / mb:.1f} TFLOP/s)"
              f"  B-A {100 * (mb - ma) / ma:+.2f} %  A-to-A spread {100 * spread / ma:.2f} %  same bits: {same}", flush=True)


if __name__ == "__main__":
    main()
