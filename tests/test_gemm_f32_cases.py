"""The case table of the exact-fp32 GEMM tests holds what it promises (no GPU): a later edit cannot hollow it out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_f32_cases as gc  # noqa: E402


def _of(inst):
    return [c for c in gc.CASES if c.instance == inst]


def test_dispatch_rule_restated():
    assert gc.instance_of(300, 200, 96, 0, 0) == "glds<128,128>"
    assert gc.instance_of(300, 200, 100, 0, 0) == "generic<128,128> NT"      # K % 32 != 0
    assert gc.instance_of(300, 200, 96, 32, 0) == "generic<128,128> NT"      # padded taps
    assert gc.instance_of(300, 65, 16, 0, 0) == "generic<128,128> NT"        # K < 32
    assert gc.instance_of(300, 64, 96, 0, 0) == "generic<128,64> NT"
    assert gc.instance_of(300, 33, 96, 0, 0) == "generic<128,64> NT"
    assert gc.instance_of(300, 32, 96, 0, 0) == "generic<128,32> NT"
    assert gc.instance_of(300, 200, 96, 0, 1) == "generic<128,128> KN"
    assert gc.instance_of(300, 64, 96, 0, 1) == "generic<128,64> KN"
    assert gc.instance_of(300, 32, 96, 0, 1) == "generic<128,32> KN"


def test_limits_and_launcher_requirements():
    names = [c.name for c in gc.CASES]
    assert len(set(names)) == len(names)
    for c in gc.CASES:
        assert 1 <= c.M <= 385 and 1 <= c.N <= 272 and 0 <= c.K <= 768 and 1 <= c.nz <= 6, c.name
        assert c.nz % c.nz2 == 0 and c.lda % 4 == 0 and c.ldb % 4 == 0 and c.a_pad_k % 4 == 0, c.name
        assert all(s % 4 == 0 for s in c.strides[:4]), c.name
        assert c.a_off % 4 == 0 and c.b_off % 4 == 0, c.name                 # 16-byte aligned inside an aligned buffer
        assert c.N % 4 == 0 if c.b_kn else c.K % 4 == 0, c.name
        assert c.alpha in (1.0, 0.125, 2.0), c.name
        assert c.lda >= 4 and c.ldb >= 4, c.name                             # one float4 per row also at K = 0
        assert c.ldc >= c.N and (not c.residual or c.ldr >= c.N), c.name


@pytest.mark.parametrize("inst", gc.INSTANCES)
def test_every_instance_meets_every_edge(inst):
    cs = _of(inst)
    assert cs, f"no case reaches {inst}"
    assert {c.M for c in cs} >= set(gc.EDGE_M)
    assert {c.N for c in cs} >= set(gc.EDGE_N[inst])
    ks = set(gc.edge_k(inst))
    assert {c.K for c in cs} >= ks
    # M is crossed with K: every row-tile edge meets every k-loop trip count and tail
    assert {(c.M, c.K) for c in cs} >= {(m, k) for m in gc.EDGE_M for k in ks}


def test_edge_values_are_the_ones_the_kernels_turn_on():
    assert gc.EDGE_M == (1, 127, 128, 129, 257)
    assert gc.EDGE_K_NT == (4, 28, 32, 36, 64, 68, 100) and gc.EDGE_K_GLDS == (32, 64, 96, 768)
    assert gc.EDGE_K_KN == (1, 2, 3, 5, 31, 32, 33, 249)
    assert gc.EDGE_N["generic<128,32> NT"] == (1, 4, 31, 32) and gc.EDGE_N["generic<128,32> KN"] == (4, 32)
    assert gc.EDGE_N["generic<128,64> NT"] == (33, 36, 64) and gc.EDGE_N["generic<128,64> KN"] == (36, 64)
    for inst in ("glds<128,128>", "generic<128,128> NT"):
        assert gc.EDGE_N[inst] == (65, 68, 128, 129, 132, 272)
    assert gc.EDGE_N["generic<128,128> KN"] == (68, 128, 132, 272)


def test_special_cases_present():
    k0 = [c for c in gc.CASES if c.K == 0]
    assert {c.b_kn for c in k0} == {0, 1} and all(c.bias and c.residual for c in k0)
    conv = [c for c in gc.CASES if c.name.startswith("conv3")]
    assert {c.M for c in conv} == {1, 2, 3, 129} and {c.a_pad_k for c in conv} == {4, 32, 36}
    assert {c.N for c in conv} == {48, 128}
    assert {(c.M, c.a_pad_k, c.N) for c in conv} == {(t, ci, co) for t in (1, 2, 3, 129) for ci in (4, 32, 36) for co in (48, 128)}
    assert {c.instance for c in conv} == {"generic<128,64> NT", "generic<128,128> NT"}
    for c in conv:
        assert c.K == 3 * c.a_pad_k and c.lda == c.a_pad_k and c.nz == 3 and c.bias and c.residual and c.act != gc.ACT_NONE
        assert c.strides[0] == c.M * c.lda                                   # sequences back to back
        assert c.strides[6] != c.strides[4] or c.ldr != c.ldc               # R has its own ldr / sR1
    assert {c.act for c in conv} == {gc.ACT_GELU, gc.ACT_SILU}
    qk = gc.case_by_name("attention QK^T")
    assert qk.alpha == 0.125 and qk.ldc > qk.N and qk.shared_ab and qk.nz2 > 1 and all(qk.strides[:6])
    pv = gc.case_by_name("attention PV")
    assert pv.b_kn and pv.K == 249 and pv.lda == 256 and pv.nz2 > 1 and all(pv.strides[:6])
    pc = gc.case_by_name("grouped posconv")
    assert pc.strides[2] == 0 and pc.strides[5] == pc.N and pc.ldc == pc.nz2 * pc.N and pc.lda < pc.K
    sk = gc.case_by_name("split-K wgrad")
    assert sk.strides[0] == sk.strides[2] == sk.K and sk.lda == sk.ldb == sk.nz * sk.K and sk.nz > 1
    # two batch levels with all eight strides in use, none equal to another of the same operand pair or to C's: on the
    # register-staged kernel with either B layout and on the LDS-DMA kernel (each forms its own batch pointers)
    full = [c for c in gc.CASES if c.nz2 > 1 and c.nz // c.nz2 > 1 and c.residual and all(c.strides)
            and c.strides[6] != c.strides[7] and c.strides[4] != c.strides[5] and c.strides[6:] != c.strides[4:6]]
    assert {c.instance.split("<")[0] + (" KN" if c.b_kn else " NT") for c in full} >= {"glds NT", "generic NT", "generic KN"}
    assert all(c.ldr != c.ldc for c in full)


def test_storage_maps_stay_inside_the_buffers_and_outputs_are_disjoint():
    """Every logical element and everything the kernels may load lies inside the buffer; no two outputs share an address;
    a guard of GUARD floats lies in front of and behind everything that is loaded or stored."""
    for c in gc.CASES:
        la, lb, lc, lr = gc.buffer_lengths(c)
        ia, va = gc.a_index(c)
        ib, ic = gc.b_index(c), gc.c_index(c)
        if ia.size:
            assert ia[:, va].min() >= gc.GUARD and ia[:, va].max() < la - gc.GUARD, c.name
        if ib.size:
            assert ib.min() >= gc.GUARD and ib.max() < lb - gc.GUARD, c.name
        assert ic.min() >= gc.GUARD and ic.max() < lc - gc.GUARD, c.name
        assert np.unique(ic).size == ic.size, c.name
        ext = gc.read_extents(c)
        assert ext["A"][0] >= gc.GUARD and ext["A"][1] < la - gc.GUARD, (c.name, ext, la)
        assert ext["B"][0] >= gc.GUARD and ext["B"][1] < lb - gc.GUARD, (c.name, ext, lb)
        if c.residual:
            ir = gc.r_index(c)
            assert np.unique(ir).size == ir.size and ir.min() >= gc.GUARD and ir.max() < lr - gc.GUARD, c.name
            assert ext["R"][0] >= gc.GUARD and ext["R"][1] < lr - gc.GUARD, c.name
        if c.a_pad_k and c.name.startswith("conv3"):
            # a whole row of fill in front of the first and behind the last sequence
            assert ia[:, va].min() == c.a_off + c.a_pad_k and la - 1 - ia[:, va].max() >= c.a_pad_k, c.name


def test_padding_exists_where_the_padding_test_needs_it():
    """The NaN test means something only if there is padding: per instance some case has A columns between K and lda,
    B padding, R padding, C padding and a batch gap; for B [K][N] some case has K % 4 != 0 (the float4 that straddles K)."""
    for inst in gc.INSTANCES:
        cs = _of(inst)
        assert any(c.lda_slack > 0 for c in cs), inst
        assert any(c.ldb_slack > 0 for c in cs), inst
        assert any(c.ldc_slack > 0 for c in cs), inst
        assert any(c.ldr_slack > 0 for c in cs), inst
        assert any(c.nz > 1 for c in cs), inst
        if inst.endswith("KN"):
            assert any(c.K % 4 and c.lda > c.K for c in cs), inst


def test_integer_cases_are_exact_in_fp32():
    for c in gc.CASES:
        assert gc.int_magnitude_bound(c) < 2 ** 24, c.name
    for c in gc.CASES[::17] + (gc.case_by_name("attention PV"), gc.case_by_name("conv3 T2 Cin4 Cout48")):
        ops = gc.materialize(c, "int", 1)
        assert np.abs(ops.A).max(initial=0) <= gc.INT_AMAX and np.abs(ops.B).max(initial=0) <= gc.INT_AMAX
        want = gc.expected(c, ops)
        assert np.isfinite(want).all() and np.abs(want).max() < 2 ** 24
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        # non-logical storage is fill and nothing else
        assert np.isnan(ops.bufA[:gc.GUARD]).all() and np.isnan(ops.bufA[-gc.GUARD:]).all()


def test_conv_case_is_a_convolution():
    """The logical A of an a_pad_k case is the k = 3 / pad = 1 window over each sequence on its own."""
    c = gc.case_by_name("conv3 T3 Cin4 Cout48")
    ops = gc.materialize(c, "int", 3)
    Cin, T = c.a_pad_k, c.M
    x = ops.bufA[c.a_off + Cin: c.a_off + Cin + c.nz * T * Cin].reshape(c.nz, T, Cin).astype(np.float64)
    assert np.isfinite(x).all()
    xp = np.pad(x, ((0, 0), (1, 1), (0, 0)))
    win = np.concatenate([xp[:, 0:T], xp[:, 1:T + 1], xp[:, 2:T + 2]], axis=2)
    assert np.array_equal(win, ops.A)


def test_float_subset_covers_every_instance():
    assert {c.instance for c in gc.FLOAT_CASES} == set(gc.INSTANCES)
    assert any(c.a_pad_k for c in gc.FLOAT_CASES) and gc.case_by_name("attention PV") in gc.FLOAT_CASES


@pytest.mark.parametrize("case", gc.FLOAT_CASES, ids=lambda c: c.name)
def test_float_bar_leaves_room_for_an_fp32_gemm(case):
    """numpy's float32 matmul as the kernel passes the derived bar: the reference alone stays inside the bound."""
    ops = gc.materialize(case, "float", 5)
    ref = gc.expected(case, ops)
    bar = gc.float_bound(case, ops)
    got = gc.numpy_f32_gemm(case, ops).astype(np.float64)
    assert case.K > 0 and np.isfinite(ref).all() and (bar > 0).all()
    ratio = np.abs(got - ref) / bar
    assert ratio.max() <= 1.0, f"{case.name}: worst ratio {ratio.max():.3f}"


def test_activation_grid_and_cpu_figures():
    A, B, x = gc.act_operands(140, 36, 136, 0)
    assert set(np.unique(np.round(x * 8)).astype(int)) == set(gc.ACT_GRID)
    assert set(np.arange(-64, 65)) | {-160, 160, -720, 720} == set(gc.ACT_GRID)
    Akn, Bkn, xkn = gc.act_operands(140, 36, 136, 1)
    assert np.array_equal(Akn @ Bkn * 0.125, x) and np.array_equal(xkn, x)
    for act in (gc.ACT_GELU, gc.ACT_SILU):
        fig = gc.act_cpu_figure(act)
        assert 0 < fig < 1e-6                                               # a few ulp of fp32, relative to max(|x|, 2^-10)
        assert gc.act_bar(act) >= 4 * fig
    assert gc.act_bar(gc.ACT_GELU) >= 1.1e-7
    # a wrong element mapping is far outside the bar
    y = gc.act_reference64(x, gc.ACT_GELU)
    assert gc.act_metric(np.roll(y, 1, axis=1), x, gc.ACT_GELU).max() > 0.1
