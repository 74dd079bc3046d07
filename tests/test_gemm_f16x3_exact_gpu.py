"""Every kernel instance of rsaf_gemm_f16x3 held per element: exact on integer planes under real scales, alpha, bias and
residual, blind to operand padding, writing nothing but [M][N] of C and of the two planes, reporting the exact maximum,
inside a derived float bar on data a global metric hides, with its activations at exact inputs, and refusing what the
launcher documents; then the two producers of plane operands.  The case table, the references and the bars live in
tests/gemm_f16x3_cases.py (held without a GPU by tests/test_gemm_f16x3_cases.py).

Measured on one MI355X (profiles/r31/gemm_f16x3_cases.txt has the run): the figures are in the docstrings of the float and
activation tests; profiles/r31/gemm_f16x3_mutations.txt shows which cases catch seven mutated kernels."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_f16x3_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

JUNK = 1000.0                               # finite padding: a leak shifts an integer result
U32, U16 = np.uint32, np.uint16


def _launch(c, ops, amax0=0):
    """One launch of the case on its storage.  Returns (C's buffer as uint32 bit patterns, the plane buffer as uint16, amax
    bits); both outputs are allocated and prefilled with their sentinel whether the call receives them or not."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    _, _, lc, lcp, _ = gc.buffer_lengths(c)
    dev = lambda a: torch.from_numpy(a).cuda()                                   # noqa: E731
    dA, dB = dev(ops.bufA.view(np.int16)), dev(ops.bufB.view(np.int16))
    dsa, dsb = dev(ops.a_scale), dev(ops.b_scale)
    dcs = dev(ops.c_scale) if c.planes else None
    dbias = dev(ops.bias) if ops.bias is not None else None
    dR = dev(ops.bufR) if c.resid else None
    dC = dev(np.full(lc, gc.SENTINEL_F32, dtype=U32).view(np.float32))
    dP = dev(np.full(lcp, gc.SENTINEL_U16, dtype=U16).view(np.int16))
    amax = dev(np.array([amax0], dtype=U32).view(np.int32))
    rc = lib.rsaf_gemm_f16x3(_lib.c_void_p_off(dA, c.a_off), c.a_plane, _lib.ptr(dsa), c.a_scale_stride,
                             _lib.c_void_p_off(dB, c.b_off), c.b_plane, _lib.ptr(dsb),
                             _lib.c_void_p_off(dC, c.c_off) if c.f32 else None,
                             _lib.c_void_p_off(dP, c.cp_off) if c.planes else None, c.c_plane, _lib.optr(dcs), c.c_scale_stride,
                             _lib.ptr(amax), _lib.optr(dbias), _lib.c_void_p_off(dR, c.r_off) if c.resid else None,
                             c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.ldr, c.act, c.alpha, c.a_panels, c.b_panels, c.c_panels, None)
    _lib.check(rc, c.name)
    torch.cuda.synchronize()
    return dC.cpu().numpy().view(U32), dP.cpu().numpy().view(U16), int(amax.cpu().numpy().view(U32)[0])


def _f32(bits):
    return bits.view(np.float32)


def _f16(bits):
    return bits.view(np.float16).astype(np.float64)


def _normalised(hi, lo):
    """hi is a nearest fp16 of hi + lo, per element: |lo| is at most half the distance from hi to its neighbour on lo's side.
    (Not `hi == fp16(hi + lo)`: where lo is subnormal it is itself rounded, hi + lo can land exactly between two fp16
    numbers, and round-to-even may then name the other one; the reference split has such elements.)"""
    h16, l64 = hi.view(np.float16), _f16(lo)
    with np.errstate(over="ignore"):
        side = np.nextafter(h16, np.where(l64 < 0, -np.inf, np.inf).astype(np.float16))
    return np.abs(l64) <= 0.5 * np.abs(side.astype(np.float64) - h16.astype(np.float64))


def _where(c, bad, what, got, want):
    m, n = np.argwhere(bad)[0]
    return f"{c.instance}, case '{c.name}': {int(bad.sum())} elements of {what} differ, first at (m, n) = ({m}, {n}): " \
           f"{got[m, n]} for {want[m, n]}"


def _act_case_bar(x, act):
    """The activation bar on the pre-activations of a case: 4 x the worst figure of the fp32 formula on the CPU over these
    x, not below the bar of the grid (gc.act_bar)."""
    return max(gc.act_bar(act), 4.0 * float(gc.act_metric(gc.act_cpu(x.astype(np.float32), act), x, act).max()))


def _check_values(c, ops, x, cbuf, pbuf):
    """(a) for one launch: None, or the message of the first failure.  act 0: C is the exact value bit for bit and the planes
    are the reference split of that fp32 value.  With an activation the pre-activation x is exact and the output is held to
    the activation bar per element (planes decoded as (hi + lo) / c_scale, with the allowance of the output split)."""
    y32 = None
    if c.f32:
        got = _f32(cbuf[gc.c_index(c)])
        if c.act == gc.ACT_NONE:
            want = x.astype(np.float32)
            bad = ~(got == want)
            if bad.any():
                return _where(c, bad, "C", got, want)
            y32 = got
        else:
            e = gc.act_metric(got, x, c.act)
            bar = _act_case_bar(x, c.act)
            bad = ~(e <= bar)
            if bad.any():
                return _where(c, bad, f"C (activation metric over {bar:.3e})", got, gc.act_reference64(x, c.act))
    if c.planes:
        ip = gc.cp_index(c)
        hi, lo = pbuf[ip[0]], pbuf[ip[1]]
        if c.act == gc.ACT_NONE:
            whi, wlo = gc.expected_planes(y32 if y32 is not None else x.astype(np.float32), ops.cs)
            for name, g, w in (("hi", hi, whi), ("lo", lo, wlo)):
                if (g != w).any():
                    return _where(c, g != w, f"plane {name} ({'panels' if c.c_panels else 'row-major'})", _f16(g), _f16(w))
        else:
            h64, l64 = _f16(hi), _f16(lo)
            dec = (h64 + l64) / ops.cs[:, None]
            # the output split: 2^-21 |y|, and 2^-25 / c_scale where lo is subnormal (a grid of 2^-24), |y| <= |x|
            bar = _act_case_bar(x, c.act) + 2.0 ** -21 + 2.0 ** -25 / ops.cs[:, None] / np.maximum(np.abs(x), 2.0 ** -10)
            bad = ~(gc.act_metric(dec, x, c.act) <= bar)
            if bad.any():
                return _where(c, bad, "decoded planes (activation metric over its bar)", dec, gc.act_reference64(x, c.act))
            norm = ~_normalised(hi, lo)
            if norm.any():
                return _where(c, norm, "plane hi (no nearest fp16 of hi + lo)", h64, h64 + l64)
    return None


def _check_sentinels(c, cbuf, pbuf):
    """(c) for one launch: the sentinel everywhere outside [M][N] of C and outside the logical elements of both planes; an
    output the call did not receive is all sentinels."""
    for name, buf, sent, idx, on in (("C", cbuf, gc.SENTINEL_F32, gc.c_index(c), c.f32),
                                     ("planes", pbuf, gc.SENTINEL_U16, gc.cp_index(c) if c.planes else None, c.planes)):
        keep = np.ones(buf.size, dtype=bool)
        if on:
            keep[idx.reshape(-1)] = False
            assert keep[:gc.GUARD].all() and keep[-gc.GUARD:].all()
        stray = np.flatnonzero(buf[keep] != sent)
        if stray.size:
            return f"{c.instance}, case '{c.name}': {stray.size} elements of {name} outside the result written, first at " \
                   f"buffer index {np.flatnonzero(keep)[stray[0]]}" + ("" if on else " (an output the call never received)")
    return None


def _check_amax(c, ops, x, cbuf, pbuf, amax):
    """(f) for one launch: the bit pattern of the largest |value written|.  Without activation the expected maximum is that
    of the exact value, independent of anything the kernel wrote, and the comparison is exact.  With an activation and an
    fp32 output it is the maximum of the C the same launch wrote (exact, but not independent: (a) holds that C).  With an
    activation into planes alone the fp32 values that were split cannot be recovered: amax_out is then held to 2^-21
    relative of the largest decoded |hi + lo| / c_scale (the split error), not exactly."""
    if c.act == gc.ACT_NONE:
        want = float(np.abs(x.astype(np.float32)).max())
    elif c.f32:
        want = float(np.abs(_f32(cbuf[gc.c_index(c)])).max())
    else:
        ip = gc.cp_index(c)
        dec = np.abs((_f16(pbuf[ip[0]]) + _f16(pbuf[ip[1]])) / ops.cs[:, None]).max()
        got = float(np.array([amax], dtype=U32).view(np.float32)[0])
        return None if abs(got - dec) <= 2.0 ** -21 * dec else f"{c.instance}, case '{c.name}': amax {got} for {dec} (planes decoded)"
    wbits = int(np.array([want], dtype=np.float32).view(U32)[0])
    return None if amax == wbits else f"{c.instance}, case '{c.name}': amax bits {amax:#x} for {wbits:#x} (max |y| = {want})"


def _int_verdicts(c, seed):
    """The integer launches of one case (padding JUNK, padding NaN, same values) and the verdict of each check."""
    junk = gc.materialize(c, "int", seed, fill=JUNK)
    nan = gc.materialize(c, "int", seed, fill=np.nan)
    assert np.array_equal(junk.Ah, nan.Ah) and np.array_equal(junk.Bl, nan.Bl)
    x = gc.expected(c, junk)
    cj, pj, aj = _launch(c, junk)
    cn, pn, an = _launch(c, nan)
    v = {"case": c.name, "a": _check_values(c, junk, x, cj, pj), "c": _check_sentinels(c, cj, pj) or _check_sentinels(c, cn, pn),
         "f": _check_amax(c, junk, x, cj, pj, aj), "b": None}
    if not (np.array_equal(cj, cn) and np.array_equal(pj, pn) and aj == an):
        for name, idx, bj, bn in (("C", gc.c_index(c), cj, cn), ("planes", gc.cp_index(c), pj, pn)):
            bad = bj[idx] != bn[idx]
            if bad.any():
                view = _f32 if name == "C" else _f16
                at = np.argwhere(bad)[0]
                v["b"] = f"{c.instance}, case '{c.name}': NaN padding changes {int(bad.sum())} elements of {name}, first at " \
                         f"{tuple(int(i) for i in at)}: {view(bn[idx])[tuple(at)]} for {view(bj[idx])[tuple(at)]}"
                break
        else:
            v["b"] = f"{c.instance}, case '{c.name}': NaN padding changes amax or bits outside the result ({aj:#x} / {an:#x})"
    return v


@functools.lru_cache(maxsize=None)
def _int_runs(inst):
    """One set of launches per instance: every case of the table twice (only the verdicts are kept)."""
    return [_int_verdicts(c, 100 + i) for i, c in enumerate(c for c in gc.CASES if c.instance == inst)]


def _assert_clean(inst, check):
    runs = _int_runs(inst)
    assert len(runs) >= 30
    bad = [v[check] for v in runs if v[check]]
    assert not bad, f"{len(bad)} of {len(runs)} cases fail; first: {bad[0]}"


@pytest.mark.parametrize("inst", gc.INSTANCES)
def test_bit_exact_per_element(rsaf_lib, inst):
    """(a) integer planes, real power-of-two scales, alpha, bias and residual: C is the exact value bit for bit; the planes
    are fp16(y c_scale) and fp16(y c_scale - hi) bit for bit, row-major and in panels (in {act 0, C, planes} of the C that
    was written).  With an activation the exact pre-activation is held to the activation bar per element."""
    _assert_clean(inst, "a")


@pytest.mark.parametrize("inst", gc.INSTANCES)
def test_padding_reaches_no_result(rsaf_lib, inst):
    """(b) the same launches with NaN in every storage element that is no logical operand element (row slack of A, B and R,
    plane-stride slack, guards, the scale elements a stride of 0 must not read): the same bits come out."""
    _assert_clean(inst, "b")


@pytest.mark.parametrize("inst", gc.INSTANCES)
def test_nothing_outside_the_result_is_written(rsaf_lib, inst):
    """(c) the sentinel survives in C's columns N .. ldc-1 and guards, in the planes' row slack, plane-stride slack and guards,
    outside [N/16][M][16] of a panel output, and in the whole of an output the call did not receive."""
    _assert_clean(inst, "c")


@pytest.mark.parametrize("inst", gc.INSTANCES)
def test_amax_is_the_maximum_written(rsaf_lib, inst):
    """(f) amax_out holds the bit pattern of max |value written| over [M][N]: exactly and against the exact value in the nine
    instances without activation, exactly against the C of the same launch in the ten with an activation and an fp32 output,
    to 2^-21 relative of the decoded planes in the six with an activation into planes (see _check_amax)."""
    _assert_clean(inst, "f")


def test_persistent_walk_per_tile_configuration(rsaf_lib):
    """More tiles than persistent workgroups on each of the three tile configurations (M = BM (CUs + 3), the smallest N,
    K = 48): every element exact, nothing else written."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for i, c in enumerate(gc.walk_cases(cus)):
        ops = gc.materialize(c, "int", 300 + i, fill=np.nan)
        x = gc.expected(c, ops)
        cbuf, pbuf, amax = _launch(c, ops)
        for msg in (_check_values(c, ops, x, cbuf, pbuf), _check_sentinels(c, cbuf, pbuf), _check_amax(c, ops, x, cbuf, pbuf, amax)):
            assert msg is None, msg


def test_amax_is_an_atomic_max_and_skips_zero(rsaf_lib):
    """(f) a start value above the maximum survives; when every written value is 0 the word is left as it was (0).  Run on
    the three tile configurations of {act 0, C} (both checks) and of {GELU, planes} (the second) only: the amax code is one
    piece of the kernel template, shared by every instance."""
    for tile in gc.TILES:
        c = next(c for c in gc.CASES if c.instance == f"{tile} none C" and c.M > 256 and not c.bias)
        ops = gc.materialize(c, "int", 41, fill=np.nan)
        big = int(np.array([3.0e38], dtype=np.float32).view(U32)[0])
        assert float(np.abs(gc.expected(c, ops)).max()) < 3.0e38
        assert _launch(c, ops, amax0=big)[2] == big
        ops.bufA[gc.a_index(c)] = 0                                                  # A = 0: every value written is 0
        cbuf, _, amax = _launch(c, ops)
        assert (cbuf[gc.c_index(c)] << 1 == 0).all() and amax == 0
        c = next(c for c in gc.CASES if c.instance == f"{tile} gelu planes" and c.M > 256 and not c.bias)
        ops = gc.materialize(c, "int", 42, fill=np.nan)
        ops.bufA[gc.a_index(c)] = 0
        _, pbuf, amax = _launch(c, ops)
        assert (pbuf[gc.cp_index(c)] << 1 == 0).all() and amax == 0


ACT_LIPSCHITZ = 1.13                        # max |GELU'| = 1.129, max |SiLU'| = 1.0998


def _check_zero_rows(c, ops, cbuf, pbuf, tag):
    """(d) the all-zero row of A (row M // 2) and of W (column N // 3) give act(bias + R).  The pre-activation there is
    z = fp32(bias + R), one rounding, whatever the accumulation did.  Without activation: C equals z and the planes equal the
    reference split of z, bit for bit.  Behind an activation: the activation bar alone on z (with the allowance of the
    output split for planes), and +-0 exactly where there is neither bias nor residual."""
    z = np.zeros((c.M, c.N), dtype=np.float32)
    if ops.bias is not None:
        z = z + ops.bias[None, :]
    if ops.R is not None:
        z = (z + ops.R.astype(np.float32)).astype(np.float32)
    sel = np.zeros((c.M, c.N), dtype=bool)
    sel[c.M // 2] = True
    sel[:, c.N // 3] = True
    zs = z[sel]
    z64 = zs.astype(np.float64)
    bar = _act_case_bar(z64, c.act) if c.act != gc.ACT_NONE else 0.0
    if c.f32:
        bits = cbuf[gc.c_index(c)][sel]
        got = _f32(bits)
        if c.act == gc.ACT_NONE:
            ok = got == zs
        else:
            ok = np.where(zs == 0, bits << 1 == 0, gc.act_metric(got, z64, c.act) <= bar)
        if not ok.all():
            i = np.flatnonzero(~ok)[0]
            return f"{tag}: {int((~ok).sum())} elements of C in the all-zero row of A or of W are not act(bias + R), first {got[i]} at z = {zs[i]}"
    if c.planes:
        ip = gc.cp_index(c)
        hi, lo = pbuf[ip[0]][sel], pbuf[ip[1]][sel]
        cs = np.broadcast_to(ops.cs[:, None], (c.M, c.N))[sel]
        if c.act == gc.ACT_NONE:
            whi, wlo = gc.split_reference(zs * cs.astype(np.float32))
            ok = (hi == whi.view(U16)) & (lo == wlo.view(U16))
        else:
            dec = (_f16(hi) + _f16(lo)) / cs
            allow = bar + 2.0 ** -21 + 2.0 ** -25 / cs / np.maximum(np.abs(z64), 2.0 ** -10)
            ok = np.where(zs == 0, (hi << 1 == 0) & (lo << 1 == 0), gc.act_metric(dec, z64, c.act) <= allow)
        if not ok.all():
            i = np.flatnonzero(~ok)[0]
            return f"{tag}: {int((~ok).sum())} elements of the planes in the all-zero row of A or of W are not the split of act(bias + R), " \
                   f"first hi {hi[i]:#x} lo {lo[i]:#x} at z = {zs[i]}"
    return None


def _float_case(c, seed, loose):
    """(d) for one float case and scale regime: (worst |err| / bar, None or the message of the first failure)."""
    ops = gc.materialize(c, "float", seed, fill=np.nan, loose=loose)
    x = gc.expected(c, ops)
    ref = gc.act_reference64(x, c.act)
    bar = gc.float_bound(c, ops)
    if c.act != gc.ACT_NONE:
        bar = ACT_LIPSCHITZ * bar + gc.act_bar(c.act) * np.maximum(np.abs(x), 2.0 ** -10)
    cbuf, pbuf, _ = _launch(c, ops)
    tag = f"{c.instance}, case '{c.name}', scales / {loose:g}"
    msg = _check_sentinels(c, cbuf, pbuf)
    outs = []                                                            # (what, decoded output, allowance of the output split)
    if c.f32:
        outs.append(("C", _f32(cbuf[gc.c_index(c)]).astype(np.float64), 0.0))
    if c.planes:
        ip = gc.cp_index(c)
        h64, l64 = _f16(pbuf[ip[0]]), _f16(pbuf[ip[1]])
        if not (np.isfinite(h64).all() and np.isfinite(l64).all()):
            msg = msg or f"{tag}: fp16 overflow in the plane output"
        elif not _normalised(pbuf[ip[0]], pbuf[ip[1]]).all():
            msg = msg or f"{tag}: hi is no nearest fp16 of hi + lo"
        outs.append(("planes", (h64 + l64) / ops.cs[:, None], 2.0 ** -21 * np.abs(ref) + 2.0 ** -25 / ops.cs[:, None]))
    worst = 0.0
    for what, got, split in outs:
        ratio = np.maximum(np.abs(got - ref) - split, 0.0) / bar         # <= 1: |err| <= bar + split
        ratio[~np.isfinite(got)] = np.inf
        m, n = np.unravel_index(np.argmax(ratio), ratio.shape)
        worst = max(worst, float(ratio.max()))
        if not ratio.max() <= 1.0:
            msg = msg or f"{tag}, {what}: |err| / bar = {ratio.max():.3f} at (m, n) = ({m}, {n}): {got[m, n]} for {ref[m, n]}"
    msg = msg or _check_zero_rows(c, ops, cbuf, pbuf, tag)
    return worst, msg


@pytest.mark.parametrize("inst", gc.INSTANCES)
def test_float_data_inside_the_derived_bar(rsaf_lib, inst, capsys):
    """(d) Gaussian A with outlier channels and row magnitudes over 2^-20 .. 2^20, one all-zero row of A and of W, NaN
    padding, exact scales and scales 4096 x smaller; float64 reference of the logical operands; per element
    |got - ref| <= gc.float_bound.  Behind an activation the bar is 1.13 x that (the largest slope of GELU and SiLU) plus the
    activation bar times max(|x|, 2^-10); a plane output is decoded as (hi + lo) / c_scale with 2^-21 |y| + 2^-25 / c_scale
    more for its split (c_scale comes from a bound on the row, so an element far below it has a subnormal lo, which lies on
    a grid of 2^-24: csrc/gemm_f16x3.hip states this absolute term, 2^-40 of the row's bound), is finite and normalised
    (hi a nearest fp16 of hi + lo).  The zero rows give act(bias + R): see _check_zero_rows.

    Measured on one MI355X with R_acc = 3 K / 16 + 2 (profiles/r31/gemm_f16x3_cases.txt): the worst |err| / bar of an
    instance lies between 0.05 and 0.36, fp32 outputs 0.20 .. 0.36, plane outputs (net of the split allowance) 0.05 .. 0.13."""
    cases = [(i, c) for i, c in enumerate(gc.FLOAT_CASES) if c.instance == inst]
    assert cases
    worst = {1.0: 0.0, gc.LOOSE: 0.0}
    for i, c in cases:
        for loose in (1.0, gc.LOOSE):
            w, msg = _float_case(c, 500 + i, loose)
            assert msg is None, msg
            worst[loose] = max(worst[loose], w)
    with capsys.disabled():
        print(f"\n[gemm_f16x3 float] {inst:22s} R_acc = {gc.R_ACC_PER_K16} K / 16 + 2: worst |err| / bar = {worst[1.0]:.4f} (exact scales), "
              f"{worst[gc.LOOSE]:.4f} (scales / 4096), {len(cases)} cases", end="")


def _act_launch(lib, M, N, K, act, resid, planes, c_panels):
    """One launch on gc.act_operands (no slack: the layouts are the table's business).  Returns (output [M][N] float64, x)."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    A, B, R, x = gc.act_operands(M, N, K, resid)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()             # noqa: E731
    pa = dev(np.stack([A, np.zeros_like(A)]).astype(np.float16).view(np.int16).reshape(2, M * K))
    pb = dev(np.stack([B, np.zeros_like(B)]).astype(np.float16).view(np.int16).reshape(2, N * K))
    sa, sb = dev(np.full(M, 2.0, dtype=np.float32)), dev(np.full(N, 4.0, dtype=np.float32))
    cs_host = gc.scale_for_bound(np.abs(x).max(axis=1))
    cs = dev(cs_host.astype(np.float32))
    dR = dev(R.astype(np.float32)) if resid else None
    C = torch.full((M, N), float("nan"), device="cuda") if not planes else None
    P = torch.zeros((2, M * N), dtype=torch.int16, device="cuda") if planes else None
    _lib.check(lib.rsaf_gemm_f16x3(_lib.ptr(pa), M * K, _lib.ptr(sa), 1, _lib.ptr(pb), N * K, _lib.ptr(sb), _lib.optr(C), _lib.optr(P),
                                   M * N if planes else 0, _lib.ptr(cs) if planes else None, 1, None, None, _lib.optr(dR), M, N, K,
                                   K, K, N, N if resid else 0, act, 1.0, 0, 0, int(c_panels), None), "act launch")
    torch.cuda.synchronize()
    if not planes:
        return C.cpu().numpy().astype(np.float64), x
    v = P.cpu().numpy().view(np.float16).astype(np.float64)
    v = v[0] + v[1]
    v = v.reshape(N // 16, M, 16).transpose(1, 0, 2).reshape(M, N) if c_panels else v.reshape(M, N)
    return v / cs_host[:, None], x


@pytest.mark.parametrize("act", [gc.ACT_GELU, gc.ACT_SILU], ids=["gelu", "silu"])
def test_activation_at_exact_preactivations(rsaf_lib, act, capsys):
    """(e) integer planes make the pre-activation x exact on the grid n / 8 over [-8, 8] plus +-20 and +-90, each row and
    column in its own order (a wrong element mapping is an error of order 0.1): the fp32 output with and without residual
    (x + r lands on the grid again) and the decoded plane output, on every tile configuration each row dispatches to.
    Metric |got - f64(x)| / max(|x|, 2^-10); bar 4 x the same fp32 formula on the CPU (GELU: the gelu_pair polynomial, not
    below 1.1e-7), 2^-21 more for the split of a plane output.

    Measured on one MI355X: GELU CPU 5.50e-8 (bar 2.20e-7), device 5.50e-8, decoded planes 1.32e-7; SiLU CPU 7.90e-8 (bar
    3.16e-7), device 7.90e-8, decoded planes 1.37e-7 (profiles/r31/gemm_f16x3_cases.txt)."""
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    bar, cpu = gc.act_bar(act), gc.act_cpu_figure(act)
    K = 144
    seen, worst = set(), {}
    for f32, planes, resid in ((True, False, False), (True, False, True), (False, True, False)):
        for N in (48, 96, 272):
            inst = gc.instance_of(N, act, f32, planes, resid)
            M = gc.TILE_BM[inst.split(" ")[0]] + 44
            for c_panels in ((0, 1) if planes else (0,)):
                got, x = _act_launch(lib, M, N, K, act, resid, planes, c_panels)
                e = gc.act_metric(got, x, act)
                b = bar + (2.0 ** -21 if planes else 0.0)
                assert np.isfinite(e).all(), inst
                m, n = np.unravel_index(np.argmax(e), e.shape)
                assert e.max() <= b, f"{inst} (c_panels {c_panels}): {e.max():.3e} at (m, n) = ({m}, {n}), x = {x[m, n]} (bar {b:.3e})"
                worst[planes] = max(worst.get(planes, 0.0), float(e.max()))
            seen.add(inst)
    name = gc.ACT_NAME[act]
    assert seen == {i for i in gc.INSTANCES if f" {name} " in i + " "}
    with capsys.disabled():
        print(f"\n[gemm_f16x3 act] {name}: CPU fp32 {cpu:.3e}, bar {bar:.3e}, device fp32 output {worst[False]:.3e}, "
              f"decoded planes {worst[True]:.3e}", end="")


# ---- (g) the producers of plane operands ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 257])
def test_row_scales_are_the_exact_power_of_two(rsaf_lib, rows):
    """scale[r] = 2^(14 - floor(log2 max |row|)), 1 for a zero row, also where the maximum is a power of two or one ulp below
    it; ld > K with NaN in the slack; norm2 within (K + 2) 2^-24 relative of float64 (a float64 sum, one rounding up)."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    K, ld = 100, 108
    rng = np.random.default_rng(rows)
    X = np.full((rows, ld), np.nan, dtype=np.float32)
    X[:, :K] = rng.standard_normal((rows, K)).astype(np.float32) * np.exp2(rng.integers(-20, 21, size=rows)).astype(np.float32)[:, None]
    X[0, :K] = np.clip(X[0, :K], -1.0, 1.0)
    X[0, K - 1] = -4.0                                                   # the maximum a power of two, in the last column
    if rows > 1:
        X[1, :K] = np.clip(X[1, :K], -1.0, 1.0)
        X[1, 0] = np.nextafter(np.float32(4.0), np.float32(0.0))         # ... and one ulp below it
    if rows > 2:
        X[2, :K] = 0.0
    dX = torch.from_numpy(X).cuda()
    s = torch.full((rows + 1,), 77.0, device="cuda")
    nrm = torch.full((rows + 1,), 77.0, device="cuda")
    _lib.check(lib.rsaf_f16x2_row_scales(_lib.ptr(dX), rows, K, ld, _lib.ptr(s), _lib.ptr(nrm), None), "row scales")
    torch.cuda.synchronize()
    s, nrm = s.cpu().numpy(), nrm.cpu().numpy()
    mx = np.abs(X[:, :K].astype(np.float64)).max(axis=1)
    want = gc.scale_for_bound(mx)
    assert want[0] == 2.0 ** 12 and (rows < 2 or want[1] == 2.0 ** 13) and (rows < 3 or want[2] == 1.0)
    assert np.array_equal(s[:rows].astype(np.float64), want), (s[:rows], want)
    n64 = np.sqrt((X[:, :K].astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(nrm[:rows] - n64) <= (K + 2) * 2.0 ** -24 * n64).all() and (nrm[:rows] >= n64).all()
    assert s[rows] == 77.0 and nrm[rows] == 77.0                         # one element past the rows: untouched


@pytest.mark.parametrize("K", [16, 48, 1040])
@pytest.mark.parametrize("panels", [0, 1], ids=["rowmajor", "panels"])
def test_split_is_the_reference_split(rsaf_lib, K, panels):
    """The planes equal the numpy reference split bit for bit (hi = fp16(x s), lo = fp16(fl32(x s) - hi)), row-major and in
    panels, with scale_stride 1 and 0, NaN in the ld slack, one row scaled 4096 x loose (lo subnormal); the sentinel
    survives in the plane-stride slack and the guards."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    rows, ld, slack, off = 259, K + 12, 24, 16
    rng = np.random.default_rng(K + panels)
    X = np.full((rows, ld), np.nan, dtype=np.float32)
    X[:, :K] = rng.standard_normal((rows, K)).astype(np.float32) * np.exp2(rng.integers(-10, 11, size=rows)).astype(np.float32)[:, None]
    X[7, :K] = 0.0
    X[5, 1:K:2] *= np.float32(2.0 ** -6)                                # small elements in the row that gets the loose scale
    dX = torch.from_numpy(X).cuda()
    for stride in (1, 0):
        mx = np.abs(X[:, :K]).max(axis=1)
        sc = gc.scale_for_bound(mx if stride else np.full(rows, mx.max())).astype(np.float32)
        if stride:
            sc[5] /= 4096.0
        arr = sc.copy()
        if not stride:
            arr[1:] = np.nan
        plane = rows * K + slack
        P = torch.from_numpy(np.full(off + plane + rows * K + 16, gc.SENTINEL_U16, dtype=U16).view(np.int16)).cuda()
        _lib.check(lib.rsaf_split_f16x2(_lib.ptr(dX), rows, K, ld, _lib.ptr(torch.from_numpy(arr).cuda()), stride,
                                        _lib.c_void_p_off(P, off), plane, panels, None), "split")
        torch.cuda.synchronize()
        got = P.cpu().numpy().view(U16)
        hi, lo = gc.split_reference(X[:, :K] * sc[:, None])
        if stride:
            nz = lo[5][lo[5] != 0].astype(np.float64)
            assert (np.abs(nz) < 2.0 ** -14).sum() >= K // 4             # the loose row: subnormal lo in its small elements
        r, k = np.arange(rows)[:, None], np.arange(K)[None, :]
        inner = gc.panel_index(rows, r, k) if panels else r * K + k
        keep = np.ones(got.size, dtype=bool)
        for pl, want in enumerate((hi, lo)):
            idx = off + pl * plane + inner
            keep[idx.reshape(-1)] = False
            bad = got[idx] != want.view(U16)
            assert not bad.any(), f"K={K} panels={panels} stride={stride} plane {pl}: {int(bad.sum())} differ, first at " \
                                  f"{np.argwhere(bad)[0]}: {got[idx][bad][0]:#x} for {want.view(U16)[bad][0]:#x}"
        assert keep.sum() == off + slack + 16 and (got[keep] == gc.SENTINEL_U16).all()


# ---- (h) refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(rsaf_lib):
    """(h) every RSAF_CHECK_ARG of launch_gemm_f16x3 that the public entry can trigger, with its message, on real allocated
    buffers, the checks of the two producers, the unsupported combinations; empty problems return OK; afterwards the outputs
    hold nothing but sentinels.  (No output at all is refused by the NULL-operand check, which comes first.)"""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    M, N, K = 32, 32, 32
    i16 = lambda n, v=0: torch.full((n,), v, dtype=torch.int16, device="cuda")   # noqa: E731
    A, B = i16(2 * M * K + 64), i16(2 * N * K + 64)
    sa, sb, cs = torch.ones(M + 8, device="cuda"), torch.ones(N + 8, device="cuda"), torch.ones(M, device="cuda")
    R = torch.ones((M, N + 8), device="cuda")
    Cb = torch.from_numpy(np.full(M * (N + 8), gc.SENTINEL_F32, dtype=U32).view(np.float32)).cuda()
    Pb = torch.from_numpy(np.full(2 * M * (N + 8) + 64, gc.SENTINEL_U16, dtype=U16).view(np.int16)).cuda()
    amax = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(M=M, N=N, K=K, a_off=0, b_off=0, sb_off=0, lda=K, ldb=K, ldc=N, ldr=0, a_plane=M * K, b_plane=N * K, c_plane=M * N + 8,
             act=0, f32=True, planes=False, resid=False, null_a=False, null_sa=False, null_cs=False, a_panels=0, b_panels=0):
        return lib.rsaf_gemm_f16x3(None if null_a else _lib.c_void_p_off(A, a_off), a_plane, None if null_sa else _lib.ptr(sa), 1,
                                   _lib.c_void_p_off(B, b_off), b_plane, _lib.c_void_p_off(sb, sb_off),
                                   _lib.ptr(Cb) if f32 else None, _lib.ptr(Pb) if planes else None, c_plane if planes else 0,
                                   None if (null_cs or not planes) else _lib.ptr(cs), 1, _lib.ptr(amax), None,
                                   _lib.ptr(R) if resid else None, M, N, K, lda, ldb, ldc, ldr, act, 1.0, a_panels, b_panels, 0, None)

    def refused(msg, **kw):
        with pytest.raises(_lib.RsafError, match=msg):
            _lib.check(call(**kw), "rsaf_gemm_f16x3")

    refused("negative dimension", M=-1)
    refused("negative dimension", K=-16)
    refused("NULL operand", null_a=True)
    refused("NULL operand", f32=False, planes=False)                     # no output at all
    refused("every plane operand needs its scales", null_sa=True)
    refused("every plane operand needs its scales", planes=True, null_cs=True)
    refused("K must be a positive multiple of 16", K=24)
    refused("K must be a positive multiple of 16", K=0)
    refused("N must be a multiple of 16", N=24)
    refused("ldc / ldr / output strides must keep 16-byte alignment", ldc=N + 4)
    refused("ldc / ldr / output strides must keep 16-byte alignment", resid=True, ldr=N + 2)
    refused("ldc / ldr / output strides must keep 16-byte alignment", planes=True, c_plane=M * N + 4)
    refused("multiples of 8 elements", lda=K + 4)
    refused("multiples of 8 elements", ldb=K + 4)
    refused("multiples of 8 elements", a_plane=M * K + 4)
    refused("multiples of 8 elements", b_plane=N * K + 4)
    refused("must be 16-byte aligned", a_off=4)
    refused("must be 16-byte aligned", b_off=4)
    refused("must be 16-byte aligned", sb_off=1)
    refused("residual needs ldr", resid=True, ldr=0)
    refused("act must be 0", act=3)
    refused("act must be 0", act=-1)
    refused("leading dimensions must be below 2\\^24", ldc=1 << 24)
    refused("leading dimensions must be below 2\\^24", resid=True, ldr=1 << 24)
    refused("the residual comes with the fp32 output", f32=False, planes=True, resid=True, ldr=N)
    refused("unsupported combination", planes=True, resid=True, ldr=N)    # {act 0, C, planes, R}
    refused("unsupported combination", act=1, planes=True)                # {act 1, C, planes}
    refused("unsupported combination", act=2, planes=True)
    # the launcher does not hold ldc against N, so a grid of 2^23 x 2^23 tiles passes every check above and is refused where
    # the tile walk is set up (h3_grid_fill: at most 2^31 - 1 tiles), before any launch
    refused("too many tiles", M=(1 << 31) - 1, N=(1 << 31) - 16)
    # in panels the leading dimension is not read: the same lda is accepted there (below), refused only row-major (above)
    for kw in (dict(M=0), dict(N=0)):
        _lib.check(call(**kw), "empty problem")

    X = torch.ones((8, 48), device="cuda")
    s8 = torch.ones(8, device="cuda")
    split = lambda rows=8, K=32, ld=48, x_off=0, p_off=0, plane=8 * 32, stride=1, null=False: lib.rsaf_split_f16x2(   # noqa: E731
        _lib.c_void_p_off(X, x_off), rows, K, ld, None if null else _lib.ptr(s8), stride, _lib.c_void_p_off(Pb, p_off), plane, 0, None)
    for msg, kw in (("K must be a non-negative multiple of 16", dict(K=24)), ("K must be a non-negative multiple of 16", dict(ld=46)),
                    ("K must be a non-negative multiple of 16", dict(K=64)), ("K must be a non-negative multiple of 16", dict(rows=-1)),
                    ("NULL pointer", dict(null=True)), ("plane stride must be a multiple of 8", dict(plane=8 * 32 + 4)),
                    ("scale stride 0 or 1", dict(stride=2)), ("16-byte alignment", dict(x_off=1)), ("16-byte alignment", dict(p_off=4))):
        with pytest.raises(_lib.RsafError, match=msg):
            _lib.check(split(**kw), "rsaf_split_f16x2")
    _lib.check(split(rows=0), "empty split")
    _lib.check(split(K=0), "empty split")
    scales = lambda rows=8, K=32, ld=48, null=False: lib.rsaf_f16x2_row_scales(                                         # noqa: E731
        _lib.ptr(X), rows, K, ld, None if null else _lib.ptr(s8), None, None)
    for msg, kw in (("bad shape", dict(ld=16)), ("bad shape", dict(rows=-1)), ("bad shape", dict(K=-1)), ("NULL pointer", dict(null=True))):
        with pytest.raises(_lib.RsafError, match=msg):
            _lib.check(scales(**kw), "rsaf_f16x2_row_scales")
    _lib.check(scales(rows=0), "empty")
    torch.cuda.synchronize()
    assert (Cb.cpu().numpy().view(U32) == gc.SENTINEL_F32).all() and (Pb.cpu().numpy().view(U16) == gc.SENTINEL_U16).all()
    assert amax.item() == 0 and (s8.cpu().numpy() == 1.0).all()
    # what the launcher accepts next to the refusals runs: panels with an lda that row-major would refuse
    _lib.check(call(a_panels=1, b_panels=1, lda=K + 4, ldb=K + 4), "accepted")
    torch.cuda.synchronize()
    got = Cb.cpu().numpy().view(U32)
    assert (got[:M * N] == 0).all() and (got[M * N:] == gc.SENTINEL_F32).all()   # zero planes: C = 0 in [M][N], ldc = N
