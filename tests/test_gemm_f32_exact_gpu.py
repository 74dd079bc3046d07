"""Every kernel instance of rsaf_gemm_f32 held per element: exact on integer operands, blind to operand padding, writing
nothing but [M][N] of each batch, inside a derived float bar, with its activations at exact inputs, and refusing what the
launcher documents.  The case table, the references and the bars live in tests/gemm_f32_cases.py.

Integer operands (|a|, |b| <= 8, integer bias and residual, alpha in {1, 0.125, 2}) keep every partial sum below 2^24, so
the expected value is the int64 result in any order of accumulation and the comparison is bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_f32_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x4B1DFACE], dtype=np.uint32).view(np.float32)[0]       # a finite pattern no result takes
JUNK = 1000.0                                                                 # finite padding: a leak shifts an integer result


def _launch(c, ops, act=gc.ACT_NONE):
    """One launch of the case on its storage; returns C's whole buffer as numpy, prefilled with SENTINEL."""
    import ctypes as C
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    _, _, lc, _ = gc.buffer_lengths(c)
    dA = torch.from_numpy(ops.bufA).cuda()
    dB = dA if c.shared_ab else torch.from_numpy(ops.bufB).cuda()
    dC = torch.full((lc,), float(SENTINEL), dtype=torch.float32, device="cuda")
    dbias = torch.from_numpy(ops.bias).cuda() if ops.bias is not None else None
    dR = torch.from_numpy(ops.bufR).cuda() if ops.bufR is not None else None
    st = (C.c_int64 * 8)(*c.strides)
    rc = lib.rsaf_gemm_f32(_lib.c_void_p_off(dA, c.a_off), _lib.c_void_p_off(dB, c.b_off), _lib.c_void_p_off(dC, c.c_off),
                           _lib.optr(dbias), _lib.c_void_p_off(dR, c.r_off) if dR is not None else None,
                           c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.ldr if c.residual else 0, c.nz, c.nz2, st, c.a_pad_k, act,
                           c.alpha, c.b_kn, None)
    _lib.check(rc, c.name)
    torch.cuda.synchronize()
    return dC.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _int_runs(inst):
    """Every case of one instance on integer operands, launched twice on the same values: padding JUNK, padding NaN.
    [(case, expected [nz][M][N], C buffer with junk padding, C buffer with NaN padding)]"""
    out = []
    for i, c in enumerate(c for c in gc.CASES if c.instance == inst):
        junk = gc.materialize(c, "int", 100 + i, fill=JUNK)
        nan = gc.materialize(c, "int", 100 + i, fill=np.nan)
        assert np.array_equal(junk.A, nan.A) and np.array_equal(junk.B, nan.B)
        out.append((c, gc.expected(c, junk), _launch(c, junk), _launch(c, nan)))
    return out


def _first_diff(c, got, want):
    bad = np.argwhere(got.astype(np.float64) != want)
    z, m, n = bad[0]
    return f"{c.instance}, case '{c.name}': {len(bad)} elements differ, first at (z, m, n) = ({z}, {m}, {n}): " \
           f"{got[z, m, n]} for {want[z, m, n]}"


@pytest.mark.parametrize("inst", gc.INSTANCES)
def test_bit_exact_per_element(rsaf_lib, inst):
    """(a) the int64 result, bit for bit, per batch of every case of the instance."""
    for c, want, cbuf, _ in _int_runs(inst):
        got = cbuf[gc.c_index(c)]
        for z in range(c.nz):
            assert np.array_equal(got[z].astype(np.float64), want[z]), _first_diff(c, got, want)


@pytest.mark.parametrize("inst", gc.INSTANCES)
def test_padding_reaches_no_result(rsaf_lib, inst):
    """(b) the same launches with NaN in every storage element that is no logical operand element (A's columns K .. lda-1
    and its masked taps, B's and R's row padding, batch gaps, guard rows and tails): the same bits come out."""
    for c, want, _, cnan in _int_runs(inst):
        got = cnan[gc.c_index(c)]
        assert np.array_equal(got.astype(np.float64), want), "NaN padding: " + _first_diff(c, got, want)


@pytest.mark.parametrize("inst", gc.INSTANCES)
def test_nothing_outside_the_result_is_written(rsaf_lib, inst):
    """(c) C keeps its sentinel bits in columns N .. ldc-1, in batch gaps and in the guards in front and behind."""
    for c, _, cjunk, cnan in _int_runs(inst):
        keep = np.ones(cjunk.size, dtype=bool)
        keep[gc.c_index(c).reshape(-1)] = False
        assert keep[:gc.GUARD].all() and keep[-gc.GUARD:].all()
        for buf in (cjunk, cnan):
            stray = np.flatnonzero(buf.view(np.uint32)[keep] != SENTINEL.view(np.uint32))
            assert stray.size == 0, f"{c.instance}, case '{c.name}': {stray.size} elements outside [M][N] written, first " \
                                    f"at buffer index {np.flatnonzero(keep)[stray[0]]} (C starts at {c.c_off}, ldc {c.ldc})"


def test_float_data_inside_the_derived_bar(rsaf_lib, capsys):
    """(d) Gaussian operands with outlier channels (x 40), float64 reference, per element
    |got - c| <= 1.01 (K + 3) 2^-24 (|alpha| sum_k |a_k||b_k| + |bias_n| + |R_mn|) + K 2^-126
    (one rounding per accumulated product in any order, three in the epilogue, flushed subnormals), NaN padding."""
    worst = {}
    for i, c in enumerate(gc.FLOAT_CASES):
        ops = gc.materialize(c, "float", 500 + i)
        ref, bar = gc.expected(c, ops), gc.float_bound(c, ops)
        got = _launch(c, ops)[gc.c_index(c)].astype(np.float64)
        ratio = np.abs(got - ref) / bar
        ratio[~np.isfinite(got)] = np.inf
        worst[c.instance] = max(worst.get(c.instance, 0.0), float(ratio.max()))
        with capsys.disabled():
            print(f"\n[gemm_f32 float] {c.instance:20s} {c.name:45s} worst |err| / bar = {ratio.max():.4f}", end="")
        z, m, n = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio.max() <= 1.0, f"{c.instance}, case '{c.name}': |err| / bar = {ratio.max():.3f} at (z, m, n) = ({z}, {m}, {n})"
    with capsys.disabled():
        print("\n[gemm_f32 float] worst ratio per instance: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
    assert set(worst) == set(gc.INSTANCES)


# (M, N, K, b_kn): glds, generic<128,128> NT, generic<128,64> NT, generic<128,32> NT, the three KN tiles
ACT_SHAPES = ((140, 132, 160, 0), (140, 132, 136, 0), (140, 36, 136, 0), (133, 31, 136, 0), (140, 132, 133, 1),
              (140, 36, 135, 1), (133, 32, 134, 1))


@pytest.mark.parametrize("act", [gc.ACT_GELU, gc.ACT_SILU], ids=["gelu", "silu"])
def test_activation_at_exact_preactivations(rsaf_lib, act, capsys):
    """(e) integer operands and alpha = 0.125 make the pre-activation x exact on the grid n / 8 over [-8, 8] plus +-20 and
    +-90, each row and column in its own order (a wrong element mapping is an error of order 0.1), on every instance; then
    the a_pad_k cases of the table with their own activation, bias and residual on operands in {-1, 0, 1} (x an exact
    integer).  Metric |got - f64(x)| / max(|x|, 2^-10); bar 4 x the same fp32 formula on the CPU, GELU not below 1.1e-7.

    Measured on one MI355X: GELU CPU 8.24e-8 (bar 3.30e-7), device 8.24e-8; SiLU CPU 7.90e-8 (bar 3.16e-7), device
    7.90e-8 (to the digits printed, the device's worst figure is the CPU's)."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    bar, cpu = gc.act_bar(act), gc.act_cpu_figure(act)
    worst = 0.0
    seen = set()
    for M, N, K, b_kn in ACT_SHAPES:
        A, B, x = gc.act_operands(M, N, K, b_kn)
        ldb = N if b_kn else K
        lda = gc._up4(K)
        Ap = np.full((M, lda), np.nan, dtype=np.float32)
        Ap[:, :K] = A
        c = gc.Case(f"act M{M} N{N} K{K} kn{b_kn}", M, N, K, b_kn=b_kn, lda=lda, ldb=ldb, ldc=N, alpha=0.125, a_off=0, b_off=0,
                    c_off=0)
        seen.add(c.instance)
        dA, dB = torch.from_numpy(Ap).cuda(), torch.from_numpy(B).cuda()
        dC = torch.full((M, N), float("nan"), device="cuda")
        _lib.check(lib.rsaf_gemm_f32(_lib.ptr(dA), _lib.ptr(dB), _lib.ptr(dC), None, None, M, N, K, lda, ldb, N, 0, 1, 1, None, 0,
                                     act, 0.125, b_kn, None), c.name)
        torch.cuda.synchronize()
        e = gc.act_metric(dC.cpu().numpy(), x, act)
        assert np.isfinite(e).all(), c.name
        m, n = np.unravel_index(np.argmax(e), e.shape)
        assert e.max() <= bar, f"{c.instance}, {c.name}: {e.max():.3e} at (m, n) = ({m}, {n}), x = {x[m, n]} (bar {bar:.3e})"
        worst = max(worst, float(e.max()))
    assert seen == set(gc.INSTANCES)
    for i, c in enumerate(c for c in gc.CASES if c.a_pad_k and c.act == act):
        ops = gc.materialize(c, "int", 900 + i, amax=1)
        x = gc.expected(c, ops)
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() < 2 ** 24
        got = _launch(c, ops, act=act)[gc.c_index(c)]
        e = gc.act_metric(got, x, act)
        z, m, n = np.unravel_index(np.argmax(e), e.shape)
        assert e.max() <= bar, f"{c.instance}, case '{c.name}': {e.max():.3e} at (z, m, n) = ({z}, {m}, {n}), x = {x[z, m, n]}"
        worst = max(worst, float(e.max()))
    with capsys.disabled():
        print(f"\n[gemm_f32 act] {'gelu' if act == gc.ACT_GELU else 'silu'}: CPU fp32 {cpu:.3e}, bar {bar:.3e}, device {worst:.3e}")


def test_refusals_before_any_launch(rsaf_lib):
    """(f) every RSAF_CHECK_ARG of launch_gemm_f32 and of the C wrapper, with its message, on real allocated buffers; empty
    problems return OK and write nothing."""
    import ctypes as C
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    M, N, K = 8, 8, 8
    A = torch.ones((M + 1, 16), device="cuda")
    B = torch.ones((N + 1, 16), device="cuda")
    R = torch.ones((M, N), device="cuda")
    Cb = torch.full((M, N), float(SENTINEL), device="cuda")

    def call(a_off=0, b_off=0, M=M, N=N, K=K, lda=16, ldb=16, ldr=0, nz=1, nz2=1, strides=None, a_pad_k=0, act=0, b_kn=0,
             resid=False, null_b=False):
        st = (C.c_int64 * 8)(*strides) if strides else None
        return lib.rsaf_gemm_f32(_lib.c_void_p_off(A, a_off), None if null_b else _lib.c_void_p_off(B, b_off), _lib.ptr(Cb), None,
                                 _lib.ptr(R) if resid else None, M, N, K, lda, ldb, N, ldr, nz, nz2, st, a_pad_k, act, 1.0, b_kn, None)

    def refused(msg, **kw):
        with pytest.raises(_lib.RsafError, match=msg):
            _lib.check(call(**kw), "rsaf_gemm_f32")

    refused("16-byte aligned", a_off=1)
    refused("16-byte aligned", b_off=2)
    refused("lda/ldb must be multiples of 4", lda=18)
    refused("lda/ldb must be multiples of 4", ldb=10)
    for i in range(4):
        st = [0] * 8
        st[i] = 6
        refused("batch strides of A/B must be multiples of 4", strides=st, nz=2)
    refused("K must be a multiple of 4 for B\\[N,K\\]", K=6)
    refused("N must be a multiple of 4 for B\\[K,N\\]", N=6, b_kn=1)
    refused("a_pad_k must be a multiple of 4", a_pad_k=2)
    refused("a_pad_k must be a multiple of 4", a_pad_k=-4)
    refused("residual needs ldr", resid=True, ldr=0)
    refused("nz must be a multiple of nz2", nz=3, nz2=2)
    refused("at most 65535 batches", nz=65536)
    refused("act must be 0", act=3)
    refused("act must be 0", act=-1)
    refused("negative dimension", K=-4)
    refused("NULL operand", null_b=True)
    for kw in (dict(M=0), dict(N=0), dict(nz=0)):
        _lib.check(call(**kw), "empty problem")
    # what the launcher accepts next to each refusal runs: K % 4 != 0 with B [K][N], a residual with ldr
    _lib.check(call(M=1, N=4, K=3, b_kn=1, resid=True, ldr=N), "accepted")
    torch.cuda.synchronize()
    got = Cb.cpu().numpy()
    assert np.array_equal(got[0, :4], np.full(4, 4.0, dtype=np.float32))                 # 3 ones x ones + R
    rest = np.ones((M, N), dtype=bool)
    rest[0, :4] = False
    assert (got.view(np.uint32)[rest] == SENTINEL.view(np.uint32)).all()                # the refused and empty calls wrote nothing
