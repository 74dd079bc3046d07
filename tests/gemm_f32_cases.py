"""Case table, dispatch rule and references of the exact-fp32 GEMM (``rsaf_gemm_f32``, csrc/gemm_f32.hip).

Importable without a GPU: tests/test_gemm_f32_cases.py checks the table itself, tests/test_gemm_f32_exact_gpu.py launches it.

A case names the whole launch: shape, operand layout, the two batch levels with all eight strides, the leading dimensions
(``*_slack`` is what each exceeds its minimum by), where each operand starts inside its buffer, alpha, bias, residual and
activation.  Storage comes first: ``materialize`` draws one value per storage element that some logical operand element
maps to and fills every other element of the buffers with ``fill`` (NaN for the padding test), so operands that overlap
in storage (a convolution read in place, A and B inside one packed qkv buffer, a weight shared by every chunk with
sB1 = 0) are consistent by construction, and the logical operands are read back out of the storage.

``a_pad_k`` masks k < a_pad_k of the first row and k >= K - a_pad_k of the last row of every batch; the masked elements
are not logical operand elements (they hold ``fill``).  Besides the k = 3 / pad = 1 convolutions (lda = Cin, K = 3 Cin,
a_pad_k = Cin, sequences back to back, so a leak across a sequence boundary picks up the neighbour's data, and a guard row
of ``fill`` in front of the first and behind the last sequence) the table uses a_pad_k = 4 on plain row-major operands
to reach ``generic<128,128>`` NT at K = 32 and 64, which the launcher otherwise hands to ``glds<128,128>``.

``sBias2`` (a bias offset per inner batch) is a field of GemmParams that ``rsaf_gemm_f32`` does not expose, so no case
uses it: the grouped positional convolution appears with its strides (sB1 = 0, sC2 = cg, ldc = groups * cg) and one bias
for every group.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

INSTANCES = ("glds<128,128>", "generic<128,32> NT", "generic<128,32> KN", "generic<128,64> NT", "generic<128,64> KN",
             "generic<128,128> NT", "generic<128,128> KN")

ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2
GUARD = 8                                   # floats of `fill` in front of and behind every buffer's operand


def instance_of(M, N, K, a_pad_k, b_kn):
    """The kernel ``launch_gemm_f32`` chooses (the four ``if``s at its end)."""
    if not b_kn and a_pad_k == 0 and K % 32 == 0 and K >= 32 and N > 64:
        return "glds<128,128>"
    lay = "KN" if b_kn else "NT"
    if N <= 32:
        return f"generic<128,32> {lay}"
    if N <= 64:
        return f"generic<128,64> {lay}"
    return f"generic<128,128> {lay}"


# the edge values every instance must meet (tests/test_gemm_f32_cases.py holds the table to them)
EDGE_M = (1, 127, 128, 129, 257)
EDGE_N = {
    "glds<128,128>": (65, 68, 128, 129, 132, 272),
    "generic<128,32> NT": (1, 4, 31, 32),
    "generic<128,32> KN": (4, 32),
    "generic<128,64> NT": (33, 36, 64),
    "generic<128,64> KN": (36, 64),
    "generic<128,128> NT": (65, 68, 128, 129, 132, 272),
    "generic<128,128> KN": (68, 128, 132, 272),
}
EDGE_K_NT = (4, 28, 32, 36, 64, 68, 100)    # 1, 2, 3, 4 k-tiles with and without a tail
EDGE_K_GLDS = (32, 64, 96, 768)
EDGE_K_KN = (1, 2, 3, 5, 31, 32, 33, 249)


def edge_k(instance):
    return EDGE_K_GLDS if instance.startswith("glds") else EDGE_K_KN if instance.endswith("KN") else EDGE_K_NT


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    b_kn: int = 0
    a_pad_k: int = 0
    nz: int = 1
    nz2: int = 1
    strides: tuple = (0,) * 8               # sA1, sA2, sB1, sB2, sC1, sC2, sR1, sR2
    lda: int = 0
    ldb: int = 0
    ldc: int = 0
    ldr: int = 0
    alpha: float = 1.0
    bias: bool = False
    residual: bool = False
    act: int = ACT_NONE
    a_off: int = GUARD                      # first element of each operand inside its buffer
    b_off: int = GUARD
    c_off: int = GUARD
    r_off: int = GUARD
    shared_ab: bool = False                 # B lives in A's buffer (packed qkv)

    @property
    def instance(self):
        return instance_of(self.M, self.N, self.K, self.a_pad_k, self.b_kn)

    @property
    def lda_slack(self):
        return max(self.lda - max(_up4(self.K), 4), 0)

    @property
    def ldb_slack(self):
        return self.ldb - (self.N if self.b_kn else self.K)

    @property
    def ldc_slack(self):
        return self.ldc - self.N

    @property
    def ldr_slack(self):
        return self.ldr - self.N if self.residual else 0


def _up4(v):
    return (v + 3) // 4 * 4


def _plain(name, M, N, K, b_kn, i, a_pad_k=0, **kw):
    """A row-major case; the running number i picks slack, alpha, bias, residual and a second batch behind a gap."""
    lda = max(_up4(K), 4) + (0, 4, 8)[i % 3]
    ldb = (N if b_kn else max(K, 4)) + (0, 8, 4)[(i // 2) % 3]
    ldc = N + (0, 3, 5, 8)[i % 4]
    ldr = N + (0, 1, 4)[(i // 3) % 3]
    nz = 2 if i % 4 == 3 else 1
    rows_b = max(K, 1) if b_kn else N
    strides = (M * lda + 8, 0, rows_b * ldb + 4, 0, M * ldc + 7, 0, M * ldr + 5, 0) if nz > 1 else (0,) * 8
    f = dict(b_kn=b_kn, a_pad_k=a_pad_k, nz=nz, nz2=1, strides=strides, lda=lda, ldb=ldb, ldc=ldc, ldr=ldr,
             alpha=(1.0, 0.125, 2.0)[i % 3], bias=bool(i % 2), residual=bool((i // 2) % 2))
    f.update(kw)
    return Case(name, M, N, K, **f)


def _edges():
    out = []
    for inst in INSTANCES:
        b_kn = int(inst.endswith("KN"))
        ns = EDGE_N[inst]
        i = 0
        for j, M in enumerate(EDGE_M):                      # M crossed with K; N and the rest cycle
            for K in edge_k(inst):
                N = ns[(i + j) % len(ns)]
                # generic<128,128> NT at K = 32, 64: only with masked taps (see the module docstring)
                pad = 4 if (inst == "generic<128,128> NT" and K % 32 == 0) else 0
                c = _plain(f"edge {inst} M{M} N{N} K{K}", M, N, K, b_kn, i, a_pad_k=pad)
                assert c.instance == inst, (c, inst)
                out.append(c)
                i += 1
    return out


def _k0():
    return [_plain("K0 NT", 129, 36, 0, 0, 3, alpha=2.0, bias=True, residual=True),
            _plain("K0 KN", 129, 68, 0, 1, 7, alpha=2.0, bias=True, residual=True)]


def _convs():
    out = []
    i = 0
    for T in (1, 2, 3, 129):
        for Cin in (4, 32, 36):
            for Cout in (48, 128):
                ldr = Cout + (0, 4, 7)[i % 3]
                out.append(Case(f"conv3 T{T} Cin{Cin} Cout{Cout}", T, Cout, 3 * Cin, a_pad_k=Cin, nz=3, nz2=1,
                                strides=(T * Cin, 0, 0, 0, T * Cout, 0, T * ldr + 4, 0), lda=Cin, ldb=3 * Cin, ldc=Cout,
                                ldr=ldr, alpha=1.0, bias=True, residual=True, act=(ACT_SILU, ACT_GELU)[i % 2]))
                i += 1
    return out


def _batched():
    out = []
    # S = scale Q K^T per (chunk, head) over a packed qkv buffer [nc][T][3 D] (w2v2_encoder.hip, attention_three_launch)
    nc, nh, T, hd = 2, 2, 37, 8
    D, Tp = nh * hd, 40
    # (the residual is not the call site's: it puts sR1 and sR2, different from sC1 and sC2, and an ldr of its own under
    # the second batch level of the register-staged kernels, B[N,K] here, B[K,N] in the next case)
    ldr = T + 6
    out.append(Case("attention QK^T", T, T, hd, nz=nc * nh, nz2=nh,
                    strides=(T * 3 * D, hd, T * 3 * D, hd, nh * T * Tp, T * Tp, nh * (T * ldr + 4) + 8, T * ldr + 4),
                    lda=3 * D, ldb=3 * D, ldc=Tp, ldr=ldr, alpha=0.125, residual=True, b_off=GUARD + D, shared_ab=True))
    # O = P V: B [K][N] inside the qkv buffer, K = T = 249 is no multiple of 4, lda = 256 (same place)
    T, Tp = 249, 256
    ldr = D + 5                                              # R interleaved like C, in rows of its own length
    out.append(Case("attention PV", T, hd, T, b_kn=1, nz=nc * nh, nz2=nh,
                    strides=(nh * T * Tp, T * Tp, T * 3 * D, hd, T * D, hd, T * ldr + 3, hd), lda=Tp, ldb=3 * D, ldc=D,
                    ldr=ldr, residual=True, b_off=GUARD + 2 * D))
    # grouped positional convolution (w2v2_posconv.hip, conv_runs_fp32): A rows overlap (lda = cg < K = PK cg), one weight
    # per group for every window (sB1 = 0), the groups side by side in the output row (sC2 = cg, ldc = groups cg)
    nw, PG, cg, PK, Tq = 2, 2, 8, 4, 9
    TT, Hd = Tq + PK - 1, PG * cg
    out.append(Case("grouped posconv", Tq, cg, PK * cg, nz=nw * PG, nz2=PG,
                    strides=(PG * TT * cg, TT * cg, 0, cg * PK * cg, Tq * Hd, cg, 0, 0), lda=cg, ldb=PK * cg, ldc=Hd,
                    bias=True))
    # the LDS-DMA kernel under two batch levels (no call site does this today; the kernel forms its pointers itself): all
    # eight strides in use and different from one another, bias and residual
    M, N, K = 40, 68, 32
    out.append(Case("two-level glds", M, N, K, nz=4, nz2=2,
                    strides=(2 * M * 40 + 8, M * 40 + 4, 2 * N * 36 + 4, N * 36, 2 * M * 72 + 9, M * 72 + 2, 2 * M * 70 + 7, M * 70 + 1),
                    lda=40, ldb=36, ldc=72, ldr=70, alpha=2.0, bias=True, residual=True))
    # split-K weight gradient (cnnlstm_train.hip, wgrad): s slices of kc columns out of rows of kp, one partial each
    M, NN, kc, s = 20, 36, 36, 3
    kp = s * kc
    out.append(Case("split-K wgrad", M, NN, kc, nz=s, nz2=1, strides=(kc, 0, kc, 0, M * NN, 0, 0, 0), lda=kp, ldb=kp,
                    ldc=NN))
    # the two input-gradient GEMMs of the training step, B [K][N] (cnnlstm_train.hip): dgates . W_ih and dy_sc . W_sc
    out.append(Case("dgrad lstm", 45, 32, 64, b_kn=1, lda=64, ldb=32, ldc=32))
    out.append(Case("dgrad shortcut", 150, 68, 32, b_kn=1, lda=32, ldb=68, ldc=68))
    # LSTM input projection and the 1x1 shortcut convolution: plain NT with bias
    out.append(Case("lstm inproj", 45, 128, 32, lda=32, ldb=32, ldc=128, bias=True))
    return out


CASES = tuple(_edges() + _k0() + _convs() + _batched())


def case_by_name(name):
    for c in CASES:
        if c.name == name:
            return c
    raise KeyError(name)


def _float_cases():
    """The float-data subset: per instance the edge cases with M = 257 at the longest and the shortest K, then the a_pad_k
    shape (both tiles), both attention shapes and the split-K shape."""
    out = []
    for inst in INSTANCES:
        ks = edge_k(inst)
        out += [c for c in CASES if c.name.startswith(f"edge {inst} M257 ") and c.K in (max(ks), min(ks))]
    out += [case_by_name(n) for n in ("conv3 T129 Cin36 Cout128", "conv3 T129 Cin32 Cout48", "conv3 T3 Cin4 Cout48",
                                      "attention PV", "attention QK^T", "split-K wgrad")]
    return tuple(out)


FLOAT_CASES = _float_cases()


# ---- storage maps ------------------------------------------------------------------------------------------------------
def _zoff(c, s1, s2):
    z = np.arange(c.nz, dtype=np.int64)
    return (z // c.nz2) * s1 + (z % c.nz2) * s2


def a_index(c):
    """(index [nz][M][K] into A's buffer, valid [M][K]): valid is False where a_pad_k masks the element."""
    m = np.arange(c.M, dtype=np.int64)[:, None]
    k = np.arange(c.K, dtype=np.int64)[None, :]
    idx = c.a_off + _zoff(c, c.strides[0], c.strides[1])[:, None, None] + (m * c.lda + k)[None]
    valid = np.ones((c.M, c.K), dtype=bool)
    if c.a_pad_k > 0:
        valid &= ~((m == 0) & (k < c.a_pad_k))
        valid &= ~((m == c.M - 1) & (k >= c.K - c.a_pad_k))
    return idx, valid


def b_index(c):
    """index [nz][K][N] into B's buffer of the logical B(k, n)"""
    k = np.arange(c.K, dtype=np.int64)[:, None]
    n = np.arange(c.N, dtype=np.int64)[None, :]
    inner = k * c.ldb + n if c.b_kn else n * c.ldb + k
    return c.b_off + _zoff(c, c.strides[2], c.strides[3])[:, None, None] + inner[None]


def _mn_index(c, off, s1, s2, ld):
    m = np.arange(c.M, dtype=np.int64)[:, None]
    n = np.arange(c.N, dtype=np.int64)[None, :]
    return off + _zoff(c, s1, s2)[:, None, None] + (m * ld + n)[None]


def c_index(c):
    return _mn_index(c, c.c_off, c.strides[4], c.strides[5], c.ldc)


def r_index(c):
    return _mn_index(c, c.r_off, c.strides[6], c.strides[7], c.ldr)


def buffer_lengths(c):
    """Floats of the A, B, C and R buffers: the operand's rows in full, one more row and GUARD floats behind them."""
    za = int(_zoff(c, c.strides[0], c.strides[1]).max())
    zb = int(_zoff(c, c.strides[2], c.strides[3]).max())
    zc = int(_zoff(c, c.strides[4], c.strides[5]).max())
    zr = int(_zoff(c, c.strides[6], c.strides[7]).max())
    la = c.a_off + za + (c.M - 1) * c.lda + max(_up4(c.K), c.lda, 4) + c.lda + GUARD
    rows_b = max(c.K, 1) if c.b_kn else c.N
    lb = c.b_off + zb + (rows_b - 1) * c.ldb + max(c.N if c.b_kn else max(c.K, 4), c.ldb) + GUARD
    if c.shared_ab:
        la = lb = max(la, lb)
    lc = c.c_off + zc + (c.M - 1) * c.ldc + max(c.N, c.ldc) + GUARD
    lr = c.r_off + zr + (c.M - 1) * c.ldr + max(c.N, c.ldr) + GUARD if c.residual else 0
    return la, lb, lc, lr


def read_extents(c):
    """What the kernels may load, restated from their address arithmetic: {operand: (lowest, highest) buffer index}.
    A and B (NT) are loaded as float4 at k = 0, 4, ... of every k-tile (tile 0 also when K = 0); an element past K, and a
    tap that a_pad_k masks, is replaced by the float4 at offset a_pad_k of its row; rows past M or N re-read the last row.
    B (KN) is loaded as float4 along N, a row past K replaced by row 0.  R and bias are loaded per element of [M][N]."""
    nk = max((c.K + 31) // 32, 1)
    gk = np.arange(0, nk * 32, 4, dtype=np.int64)
    m = np.arange(c.M, dtype=np.int64)[:, None]
    off = np.where(gk < c.K, gk, c.a_pad_k)[None, :] + 0 * m
    if c.a_pad_k > 0:
        hit = ((m == 0) & (gk[None] < c.a_pad_k)) | ((m == c.M - 1) & (gk[None] >= c.K - c.a_pad_k))
        off = np.where(hit, c.a_pad_k, off)
    rel = m * c.lda + off
    za = _zoff(c, c.strides[0], c.strides[1])
    ext = {"A": (c.a_off + int(za.min()) + int(rel.min()), c.a_off + int(za.max()) + int(rel.max()) + 3)}
    zb = _zoff(c, c.strides[2], c.strides[3])
    if c.b_kn:
        hi = (max(c.K, 1) - 1) * c.ldb + c.N - 1
    else:
        hi = (c.N - 1) * c.ldb + int(np.where(gk < c.K, gk, 0).max()) + 3
    ext["B"] = (c.b_off + int(zb.min()), c.b_off + int(zb.max()) + hi)
    if c.residual:
        zr = _zoff(c, c.strides[6], c.strides[7])
        ext["R"] = (c.r_off + int(zr.min()), c.r_off + int(zr.max()) + (c.M - 1) * c.ldr + c.N - 1)
    return ext


# ---- operands and references --------------------------------------------------------------------------------------------
INT_AMAX = 8            # |a|, |b| of the integer operands
INT_EPI = 64            # |bias|, |R| of the integer operands


def int_magnitude_bound(c, amax=INT_AMAX):
    """|alpha| K max|a| max|b| + |bias| + |R|: below 2^24 every partial sum is exact in fp32 in any order"""
    return abs(c.alpha) * c.K * amax * amax + INT_EPI * (int(c.bias) + int(c.residual))


@dataclasses.dataclass
class Operands:
    bufA: np.ndarray                        # float32 storage (bufB is bufA for a shared buffer)
    bufB: np.ndarray
    bias: np.ndarray | None                 # [N] float32
    bufR: np.ndarray | None
    A: np.ndarray                           # logical [nz][M][K] float64 (masked taps 0)
    B: np.ndarray                           # logical [nz][K][N] float64
    R: np.ndarray | None                    # logical [nz][M][N] float64


def materialize(c, kind, seed, fill=np.nan, amax=INT_AMAX):
    """Storage and logical operands of a case.  kind "int": integers |a|, |b| <= amax, |bias|, |R| <= INT_EPI;
    kind "float": Gaussian, the first three k of A scaled by 40 (outlier channels), B scaled by K^-1/2."""
    rng = np.random.default_rng(seed)
    la, lb, _, lr = buffer_lengths(c)

    def draw(n, scale=1.0, lim=amax):
        if kind == "int":
            return rng.integers(-lim, lim + 1, size=n).astype(np.float32)
        return (rng.standard_normal(n) * scale).astype(np.float32)

    bufA = np.full(la, fill, dtype=np.float32)
    bufB = bufA if c.shared_ab else np.full(lb, fill, dtype=np.float32)
    ia, va = a_index(c)
    ib = b_index(c)
    ua = np.unique(ia[:, va])
    bufA[ua] = draw(ua.size)
    if kind == "float" and c.K > 0:
        hot = np.unique(ia[:, :, :3][:, va[:, :3]])
        bufA[hot] *= 40.0
    ub = np.unique(ib)
    if c.shared_ab:
        ub = np.setdiff1d(ub, ua)
    bufB[ub] = draw(ub.size, scale=1.0 / max(c.K, 1) ** 0.5)
    A = np.where(va[None], bufA[ia].astype(np.float64), 0.0)
    B = bufB[ib].astype(np.float64)
    bias = draw(c.N, lim=INT_EPI) if c.bias else None
    bufR = R = None
    if c.residual:
        bufR = np.full(lr, fill, dtype=np.float32)
        ir = r_index(c)
        bufR[ir.reshape(-1)] = draw(ir.size, lim=INT_EPI)
        R = bufR[ir].astype(np.float64)
    return Operands(bufA, bufB, bias, bufR, A, B, R)


def expected(c, ops):
    """float64 alpha A B + bias + R, [nz][M][N] (exact for the integer operands)"""
    out = c.alpha * np.matmul(ops.A, ops.B)
    if ops.bias is not None:
        out = out + ops.bias.astype(np.float64)[None, None, :]
    if ops.R is not None:
        out = out + ops.R
    return out


def float_bound(c, ops):
    """The bar of the float-data test per element: at most one rounding per accumulated product in any order, three in
    the epilogue (alpha, bias, residual), and products flushed as subnormals:
    1.01 (K + 3) 2^-24 (|alpha| sum_k |a_k| |b_k| + |bias_n| + |R_mn|) + K 2^-126."""
    mag = abs(c.alpha) * np.matmul(np.abs(ops.A), np.abs(ops.B))
    if ops.bias is not None:
        mag = mag + np.abs(ops.bias.astype(np.float64))[None, None, :]
    if ops.R is not None:
        mag = mag + np.abs(ops.R)
    return 1.01 * (c.K + 3) * 2.0 ** -24 * mag + c.K * 2.0 ** -126


def numpy_f32_gemm(c, ops):
    """The same launch with numpy's float32 matmul on the CPU as the kernel: what the float bar must leave room for."""
    acc = np.matmul(ops.A.astype(np.float32), ops.B.astype(np.float32))
    out = np.float32(c.alpha) * acc
    if ops.bias is not None:
        out = out + ops.bias[None, None, :]
    if ops.R is not None:
        out = out + ops.R.astype(np.float32)
    return out.astype(np.float32)


# ---- activations on exact pre-activations -------------------------------------------------------------------------------
ACT_GRID = tuple(range(-64, 65)) + (-160, 160, -720, 720)       # times alpha = 0.125: n / 8 over [-8, 8], +-20, +-90


def act_reference64(x, act):
    """GELU(erf) / SiLU of float64 x in float64"""
    import math
    x = np.asarray(x, dtype=np.float64)
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))
    if act == ACT_SILU:
        return x / (1.0 + np.exp(-x))
    return x


def act_metric(got, x, act):
    """|got - f64(x)| / max(|x|, 2^-10) per element"""
    x = np.asarray(x, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - act_reference64(x, act)) / np.maximum(np.abs(x), 2.0 ** -10)


@functools.lru_cache(maxsize=None)
def act_cpu_figure(act):
    """The worst act_metric over ACT_GRID / 8 of the two formulas of act_apply evaluated in float32 on the CPU (torch)."""
    import torch
    x = torch.tensor(ACT_GRID, dtype=torch.float32) * 0.125
    if act == ACT_GELU:
        y = 0.5 * x * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752440, dtype=torch.float32)))
    else:
        y = x / (1.0 + torch.exp(-x))
    return float(act_metric(y.numpy(), x.numpy(), act).max())


def act_bar(act):
    """4 x the CPU figure (the device's erff / expf are specified to a few ulp, the CPU's are within one); for GELU not
    below the 1.1e-7 that csrc/gemm_f16x3.h states for the library form."""
    bar = 4.0 * act_cpu_figure(act)
    return max(bar, 1.1e-7) if act == ACT_GELU else bar


def act_operands(M, N, K, b_kn):
    """Integer A [M][K] (one-hot rows) and B (as [N][K] or [K][N]) with A B^T [m][n] = ACT_GRID[(m + 13 n) % len]: with
    alpha = 0.125 the pre-activation is exact; a row walks the whole grid from N >= len on, a column from M >= len on (the
    shapes of the test have M >= len), each in a different order, and the matrix covers the grid in any case."""
    g = np.array(ACT_GRID, dtype=np.float32)
    L = len(g)
    assert K >= L and M >= L
    A = np.zeros((M, K), dtype=np.float32)
    A[np.arange(M), np.arange(M) % L] = 1.0
    Bnk = np.zeros((N, K), dtype=np.float32)
    Bnk[:, :L] = g[(np.arange(L)[None, :] + 13 * np.arange(N)[:, None]) % L]
    x = 0.125 * (A.astype(np.float64) @ Bnk.astype(np.float64).T)
    return A, (np.ascontiguousarray(Bnk.T) if b_kn else Bnk), x
