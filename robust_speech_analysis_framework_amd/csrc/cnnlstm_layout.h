// Layouts of the CNN-LSTM classifier (cnnlstm.hip, cnnlstm_lstm.hip, cnnlstm_train.hip, cnnlstm_optim.hip), each stated once
// for the kernels that carve the memory and the host code that sizes it: the dims and what is wrong with them, the inference
// weight blob and workspace (fp32 buffers + the planes, scales and statistics of the fp16-split front), the training
// parameter blob, saved activations and scratch, and the LDS of the four recurrence kernels.  Plain C++ (no HIP include):
// tests/test_cnnlstm_layout_host.py compiles it with g++ and checks sizes, bounds, overlap and alignment
// (tests/host/cnnlstm_layout_replay.cpp).  What needs rsaf_last_error (check_dims, fail, ...) is in cnnlstm_host.h.
#pragma once
#include <algorithm>
#include <cstdint>

#include "rsaf.h"

namespace rsaf {
namespace cnnlstm {

struct Dims {
    int D, C, H, NC, L, act;
};

inline int64_t pad4(int64_t n) { return (n + 3) & ~int64_t(3); }
inline int64_t pad32(int64_t n) { return (n + 31) & ~int64_t(31); }

constexpr int DIMS_ACT_GELU = 1, DIMS_ACT_SILU = 2;     // Act of gemm_f32.h (cnnlstm_host.h asserts the match)
constexpr int TRAIN_C_MAX = 1024;                        // the training entries: WLayout's BatchNorm sums area holds [2][1024]

// what is wrong with the dims, or NULL; c_max: the cap on cnn_out_channels (TRAIN_C_MAX for the training entries, 0: none)
inline const char* dims_problem(const Dims& d, int c_max) {
    if (!(d.D > 0 && d.D % 4 == 0)) return "input_dim must be a positive multiple of 4";
    if (!(d.C > 0 && d.C % 4 == 0 && (!c_max || d.C <= c_max)))
        return c_max ? "cnn_out_channels must be a multiple of 4 in [4, 1024]" : "cnn_out_channels must be a positive multiple of 4";
    if (!(d.H == 64 || d.H == 128)) return "lstm_hidden_dim must be 64 or 128 (reference search space)";
    if (!(d.NC >= 1 && d.NC <= 16)) return "num_classes must be in [1, 16]";
    if (!(d.L >= 1 && d.L <= 4)) return "lstm_layers must be in [1, 4]";
    if (!(d.act == DIMS_ACT_GELU || d.act == DIMS_ACT_SILU)) return "activation must be gelu (1) or silu (2)";
    return nullptr;
}

// the LSTM layers and the head: the tail of the inference and of the training blob (b: the former's bih, the latter's bsum)
template <class Blob, class Take>
inline void take_lstm_head(Blob& L, int64_t (&b)[4], const Dims& d, Take take) {
    for (int l = 0; l < d.L; ++l) {
        const int in = l == 0 ? d.C : 2 * d.H;
        L.wih[l] = take((int64_t)8 * d.H * in);
        b[l] = take(8 * d.H);
        L.whh[l] = take((int64_t)2 * 4 * d.H * d.H);
    }
    L.watt = take(2 * d.H); L.batt = take(1);
    L.wfc = take((int64_t)d.NC * 2 * d.H); L.bfc = take(d.NC);
}

// ---- inference weight blob (floats); every segment starts 16-byte aligned ---------------------------------------------
struct Layout {
    int64_t w1, b1, wsc, bsc, w2, b2, w3, b3, w4, b4;
    int64_t wih[4], bih[4], whh[4];
    int64_t watt, batt, wfc, bfc, total;
};

inline Layout make_layout(const Dims& d) {
    Layout L{};
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t s = o; o += pad4(n); return s; };
    L.w1 = take((int64_t)d.C * 3 * d.D);
    L.b1 = take(d.C);
    if (d.D != d.C) { L.wsc = take((int64_t)d.C * d.D); L.bsc = take(d.C); } else { L.wsc = L.bsc = -1; }
    L.w2 = take((int64_t)d.C * 3 * d.C); L.b2 = take(d.C);
    L.w3 = take((int64_t)d.C * 3 * d.C); L.b3 = take(d.C);
    L.w4 = take((int64_t)d.C * 3 * d.C); L.b4 = take(d.C);
    take_lstm_head(L, L.bih, d, take);
    L.total = o;
    return L;
}

// ---- inference workspace ------------------------------------------------------------------------------------------------
// widths the fp16-split GEMM takes (K and N multiples of 16); anything else (test geometries) stays on the exact-fp32 MFMA
inline bool use_f16x3(int input_dim, int channels) { return input_dim % 16 == 0 && channels % 16 == 0; }

// the f16x3 front: float offsets from InferWs::f16base
struct F16Ws {
    int64_t xp, c1p, poolp, c3p, c4p, hp, wp[5], ws[5], wih_p[4], wih_s[4], stat, amax, scale, one, total;
};
constexpr int CNN_NSTAT = 5 + 5 + 4;     // weight matrices w1 wsc w2 w3 w4, their biases, wih[l]
constexpr int CNN_NAMAX = 6, CNN_NSCALE = 6;
enum { AX = 0, ASC = 1, AC1 = 2, AC2 = 3, AC3 = 4, AC4 = 5 };   // amax [6][B]: x, shortcut, conv1, conv2, conv3, conv4
enum { SX = 0, SC1 = 1, SPOOL = 2, SC3 = 3, SC4 = 4 };          // scale [6][B]: x, conv1, pooled, conv3, conv4, (spare)
// stat [CNN_NSTAT][2] = {max row norm, max |element|}: the five weight matrices, their biases, wih[l]
enum { W1 = 0, WSC = 1, W2 = 2, W3 = 3, W4 = 4 };               // also the index into F16Ws::wp / ws
constexpr int stat_w(int i) { return i; }
constexpr int stat_b(int i) { return 5 + i; }
constexpr int stat_wih(int l) { return 10 + l; }

inline F16Ws make_f16_ws(const Dims& d, int B, int T) {
    F16Ws w{};
    int64_t o = 0;
    auto take = [&](int64_t k) { int64_t s = o; o += pad4(k); return s; };
    const int Tp = T / 2;
    w.xp = take((int64_t)B * (T + 2) * d.D);
    w.c1p = take((int64_t)B * (T + 2) * d.C);
    w.poolp = take((int64_t)B * (Tp + 2) * d.C);
    w.c3p = take((int64_t)B * (Tp + 2) * d.C);
    w.c4p = take((int64_t)B * Tp * d.C);
    w.hp = take((int64_t)B * Tp * 2 * d.H);
    const int64_t wsz[5] = {(int64_t)d.C * 3 * d.D, (int64_t)d.C * d.D, (int64_t)d.C * 3 * d.C, (int64_t)d.C * 3 * d.C, (int64_t)d.C * 3 * d.C};
    for (int i = 0; i < 5; ++i) { w.wp[i] = take(wsz[i]); w.ws[i] = take(d.C); }
    for (int l = 0; l < d.L; ++l) { w.wih_p[l] = take((int64_t)8 * d.H * (l == 0 ? d.C : 2 * d.H)); w.wih_s[l] = take(8 * d.H); }
    w.stat = take(2 * CNN_NSTAT);
    w.amax = take((int64_t)CNN_NAMAX * B);
    w.scale = take((int64_t)CNN_NSCALE * B);
    w.one = take(4);
    w.total = o;
    return w;
}

// float offsets into the workspace of one forward: three [B][T][C] buffers, the input projection [B][T'][8H], two LSTM outputs
// [B][T'][2H], and behind them the f16x3 front's area (F16Ws) at the widths that take it
struct InferWs {
    int64_t bufA, bufB, bufC, xproj, seq0, seq1, f16base, total;
    bool f16;
    F16Ws F;
};

inline InferWs make_infer_ws(const Dims& d, int B, int T) {
    InferWs w{};
    const int64_t Tp = T / 2;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t s = o; o += pad4(n); return s; };
    w.bufA = take((int64_t)B * T * d.C); w.bufB = take((int64_t)B * T * d.C); w.bufC = take((int64_t)B * T * d.C);
    w.xproj = take((int64_t)B * Tp * 8 * d.H);
    w.seq0 = take((int64_t)B * Tp * 2 * d.H); w.seq1 = take((int64_t)B * Tp * 2 * d.H);
    w.f16base = o;
    w.f16 = use_f16x3(d.D, d.C);
    if (w.f16) { w.F = make_f16_ws(d, B, T); o += w.F.total; }
    w.total = o;
    return w;
}

// ---- training: parameter / gradient blob --------------------------------------------------------------------------------
struct ConvP {
    int64_t w, b, g, be;
};
struct PLayout {
    ConvP c1, sc, c2, c3, c4;
    int64_t wih[4], bsum[4], whh[4];
    int64_t watt, batt, wfc, bfc, total;
};

inline PLayout make_playout(const Dims& d) {
    PLayout L{};
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t s = o; o += pad4(n); return s; };
    auto conv = [&](int taps, int cin) { ConvP c; c.w = take((int64_t)d.C * taps * cin); c.b = take(d.C); c.g = take(d.C); c.be = take(d.C); return c; };
    L.c1 = conv(3, d.D);
    if (d.D != d.C) L.sc = conv(1, d.D); else L.sc = ConvP{-1, -1, -1, -1};
    L.c2 = conv(3, d.C); L.c3 = conv(3, d.C); L.c4 = conv(3, d.C);
    take_lstm_head(L, L.bsum, d, take);
    L.total = o;
    return L;
}

// ---- training: saved activations ------------------------------------------------------------------------------------------
struct SLayout {
    int64_t stat;                 // [5][3][C]: mean, biased var, rstd of bn1, shortcut bn, bn2, (block 2) bn1, bn2
    int64_t y1, ysc, a1d, y2, z1, p, y3, a3d, y4, z2, r2;
    int64_t gates[4], cst[4], hout[4], hdrop[4];
    int64_t prob, ctx, total;
};

inline SLayout make_slayout(const Dims& d, int B, int T) {
    SLayout S{};
    const int64_t Tp = T / 2, n1 = pad4((int64_t)B * T * d.C), n2 = pad4((int64_t)B * Tp * d.C);
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t s = o; o += pad4(n); return s; };
    S.stat = take(5 * 3 * d.C);
    S.y1 = take(n1); S.ysc = d.D != d.C ? take(n1) : -1; S.a1d = take(n1); S.y2 = take(n1); S.z1 = take(n1);
    S.p = take(n2); S.y3 = take(n2); S.a3d = take(n2); S.y4 = take(n2); S.z2 = take(n2); S.r2 = take(n2);
    for (int l = 0; l < d.L; ++l) {
        S.gates[l] = take((int64_t)B * Tp * 8 * d.H);
        S.cst[l] = take((int64_t)B * Tp * 2 * d.H);
        S.hout[l] = take((int64_t)B * Tp * 2 * d.H);
        S.hdrop[l] = l < d.L - 1 ? take((int64_t)B * Tp * 2 * d.H) : -1;
    }
    S.prob = take((int64_t)B * Tp); S.ctx = take((int64_t)B * 2 * d.H);
    S.total = o;
    return S;
}

// split of the row dimension of a weight-gradient GEMM
struct Split { int64_t kc, s, kp; };
inline Split make_split(int64_t rows) {
    int64_t kc = 1024;
    while ((rows + kc - 1) / kc > 4096) kc *= 2;
    Split sp; sp.kc = kc; sp.s = std::max<int64_t>((rows + kc - 1) / kc, 1); sp.kp = sp.s * kc;
    return sp;
}

// ---- training: scratch (floats) shared by forward and backward ----------------------------------------------------------
// `small` holds what the head's backward and the BatchNorm backward keep per row or per channel; its sub-offsets count from
// the start of the scratch like the others.  dp is addressed float by float at a row stride of T', so unlike every other
// segment it starts on a float, not on 16 bytes.
struct WLayout {
    int64_t bufA, bufB, bufC;           // [B*T][max(C, 2H)] activations / gradients
    int64_t t1, t2;                     // transposed images [Mmax][kp], [Nmax][kp]
    int64_t part;                       // split-K partial products
    int64_t red;                        // column-reduction partials (doubles)
    int64_t wflip;                      // tap-flipped transposed conv weights [C][3][C]
    int64_t small;
    int64_t bn_sums;                    // small: BatchNorm backward [2][C], room for C = TRAIN_C_MAX
    int64_t dctx;                       //        [B][2H]
    int64_t dwatt_part, dbatt_part;     //        per-sequence partials [B][2H], [B]
    int64_t dp;                         //        [B][T']
    int64_t total;
};

constexpr int RED_PARTS = 256;

inline WLayout make_wlayout(const Dims& d, int B, int T) {
    WLayout W{};
    const int64_t Tp = T / 2;
    const int64_t wide = std::max<int64_t>(d.C, 2 * d.H);
    const int64_t rows = (int64_t)B * T;
    const Split sp = make_split(rows);
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t s = o; o += pad4(n); return s; };
    const int64_t nb = std::max<int64_t>((int64_t)B * T * d.C, (int64_t)B * Tp * wide);
    W.bufA = take(nb); W.bufB = take(nb); W.bufC = take(nb);
    const int64_t Mmax = std::max<int64_t>(d.C, 8 * d.H);
    const int64_t Nmax = std::max<int64_t>(std::max<int64_t>(3 * d.D, 3 * d.C), 2 * d.H);
    W.t1 = take(Mmax * sp.kp); W.t2 = take(Nmax * sp.kp);
    int64_t mn = std::max<int64_t>((int64_t)d.C * 3 * std::max(d.D, d.C), (int64_t)8 * d.H * std::max(d.C, 2 * d.H));
    W.part = take(sp.s * mn);
    W.red = take((int64_t)RED_PARTS * 2 * std::max<int64_t>(d.C, 8 * d.H) * 2);     // doubles
    W.wflip = take((int64_t)d.C * 3 * d.C);
    const int64_t F = 2 * d.H;
    W.small = take(2 * TRAIN_C_MAX + 64 + (int64_t)B * (2 * F + 8) + (int64_t)B * Tp + 64);
    W.bn_sums = W.small;
    W.dctx = W.bn_sums + 2 * TRAIN_C_MAX + 64;
    W.dwatt_part = W.dctx + (int64_t)B * F;
    W.dbatt_part = W.dwatt_part + (int64_t)B * F;
    W.dp = W.dbatt_part + B + 4;
    W.total = o;
    return W;
}

// ---- training: scratch of the input gradient (floats), apart from WLayout so that a step without one keeps its sizes -------
// the tap-flipped transposed weights of res_block1.conv1 [D][3][C]: WLayout::wflip holds [C][3][C] only.  The shortcut term
// of the input gradient [B*T][D] needs no room of its own: it waits in WLayout::t2 ([Nmax >= 3D][kp >= B*T]).
inline int64_t dx_scratch_floats(const Dims& d) { return pad4((int64_t)d.D * 3 * d.C); }

// ---- LDS of the recurrence kernels (cnnlstm_lstm.hip), in floats ----------------------------------------------------------
// forward, 16 rows: h double-buffered [2][16][H + 4]
constexpr int rec_ldh(int H) { return H + 4; }
constexpr int rec_lds_floats(int H) { return 2 * 16 * rec_ldh(H); }
// forward, 4 rows (HALVES bodies side by side): h [2][4][H + 4] and the gate exchange tiles [H / 16 waves][4][80]
constexpr int REC4_GX_LD = 80;
constexpr int rec4_lds_floats(int H, int halves) { return halves * (2 * 4 * rec_ldh(H) + H / 16 * 4 * REC4_GX_LD); }
// BPTT, 16 rows: dgates double-buffered [2][16][4H + 4], requested at launch (above 64 KiB for H = 128)
constexpr int bwd_ldg(int H) { return 4 * H + 4; }
constexpr int bwd_lds_floats(int H) { return 2 * 16 * bwd_ldg(H); }
// BPTT, 4 rows: dgates [2][4][4H + 20]
constexpr int bwd4_ldg(int H) { return 4 * H + 20; }
constexpr int bwd4_lds_floats(int H, int halves) { return halves * 2 * 4 * bwd4_ldg(H); }

}  // namespace cnnlstm
}  // namespace rsaf
