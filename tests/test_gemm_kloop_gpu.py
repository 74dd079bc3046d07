"""The main loop and the tile walk of gemm_f16x3_kernel on exact operands, through rsaf_gemm_f16x3.

The planes hold small integers (|hi| <= 8, lo in {-1, 0, 1}) and the scales are 1, so every product and every partial sum
is an integer below 2^24: exact in fp32 in any order.  The kernel drops lo x lo by design, so the expected value is the
int64 Ah Bh^T + Ah Bl^T + Al Bh^T and the comparison is bit-exact.  K = 16 .. 80 is 1 .. 5 k-tiles: every combination of
the peeled first and last k-tiles of both wave groups with an empty, a one-trip and a two-trip steady loop; K = 768 is a
long loop.  N = 48, 128, 272 takes the 256 x 64, the 512 x 128 and the 256 x 256 tile (the last with a partial column
tile); M = 1 and 257 a single row and a partial second row tile."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _operand(rng, rows, k):
    hi = rng.integers(-8, 9, size=(rows, k)).astype(np.int64)
    lo = rng.integers(-1, 2, size=(rows, k)).astype(np.int64)
    return hi, lo


def _planes(hi, lo, panels):
    """[2][rows * k] fp16 bit patterns, row-major or as k16 panels [k / 16][rows][16]"""
    import torch
    rows, k = hi.shape
    p = np.stack([hi, lo]).astype(np.float16)
    if panels:
        p = np.ascontiguousarray(p.reshape(2, rows, k // 16, 16).transpose(0, 2, 1, 3))
    return torch.from_numpy(p.reshape(2, rows * k).view(np.int16)).cuda()


def _expected(a, b):
    (ah, al), (bh, bl) = a, b
    return ah @ bh.T + ah @ bl.T + al @ bh.T


def _run(lib, ap, bp, M, N, K, panels, planes_out=False):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    ones_m, ones_n = torch.ones(M, device="cuda"), torch.ones(N, device="cuda")
    C = None if planes_out else torch.full((M, N), float("nan"), device="cuda")
    P = torch.zeros((2, M * N), dtype=torch.int16, device="cuda") if planes_out else None
    _lib.check(lib.rsaf_gemm_f16x3(_lib.ptr(ap), M * K, _lib.ptr(ones_m), 1, _lib.ptr(bp), N * K, _lib.ptr(ones_n),
                                   _lib.ptr(C) if C is not None else None, _lib.ptr(P) if planes_out else None, M * N,
                                   _lib.ptr(ones_m) if planes_out else None, 1, None, None, None, M, N, K, K, K, N, N, 0, 1.0,
                                   int(panels), int(panels), int(planes_out), None), "gemm3")
    torch.cuda.synchronize()
    return P if planes_out else C


@pytest.mark.parametrize("N", [48, 128, 272])
@pytest.mark.parametrize("K", [16, 32, 48, 64, 80, 768])
def test_kloop_exact(rsaf_lib, K, N):
    """fp32 output, row-major and panel operands, M = 1 and 257: the int64 result, bit for bit."""
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1000 * K + N)
    for M in (1, 257):
        a, b = _operand(rng, M, K), _operand(rng, N, K)
        want = _expected(a, b)
        assert np.abs(want).max() < 2 ** 24
        for panels in (False, True):
            C = _run(lib, _planes(*a, panels), _planes(*b, panels), M, N, K, panels).cpu().numpy()
            bad = np.argwhere(C.astype(np.float64) != want)
            assert bad.size == 0, (f"M={M} N={N} K={K} panels={panels}: {len(bad)} elements differ, first at {bad[0]}: "
                                   f"{C[tuple(bad[0])]} for {want[tuple(bad[0])]}")


def test_kloop_exact_plane_output(rsaf_lib):
    """The plane output in the panel layout of the next GEMM's A (c_panels = 1), decoded as (hi + lo) / c_scale."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    M, N, K = 257, 272, 80
    rng = np.random.default_rng(7)
    a, b = _operand(rng, M, K), _operand(rng, N, K)
    want = _expected(a, b)
    assert np.abs(want).max() < 65504                                   # c_scale = 1 bounds the output
    P = _run(lib, _planes(*a, True), _planes(*b, True), M, N, K, True, planes_out=True)
    v = P.view(torch.float16).double()
    got = ((v[0] + v[1]).view(N // 16, M, 16).permute(1, 0, 2).reshape(M, N) / 1.0).cpu().numpy()
    assert np.array_equal(got, want.astype(np.float64))


def test_persistent_walk_more_tiles_than_workgroups(rsaf_lib):
    """M = 256 (CUs + 3), N = 144, K = 48: more tiles than persistent workgroups, so the walk goes on to second tiles and
    the last round is partial; every element exact."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, K = 256 * (cus + 3), 144, 48
    rng = np.random.default_rng(11)
    a, b = _operand(rng, M, K), _operand(rng, N, K)
    want = _expected(a, b)
    C = _run(lib, _planes(*a, True), _planes(*b, True), M, N, K, True).cpu().numpy()
    bad = np.argwhere(C.astype(np.float64) != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first at {bad[0]} (row tile {bad[0][0] // 256})"
