// csrc/cnnlstm_layout.h on the host: the inference weight blob and workspace, the training parameter blob, saved activations
// and scratch, and the LDS of the recurrence kernels, at the 12 geometries of tests/cnnlstm_geometry.py (their own B x T, 1 x 2
// and 17 x 6), the shipped geometry at two batches, the training cap C = 1024 and one B T at which make_split doubles kc.
// Per row: (1) every total and every offset list is the one recorded from the library before the layouts moved into the
// header (cnnlstm_layout_parent.inc), (2) every segment of every layout lies inside its total, no two overlap and every one
// starts 16-byte aligned - the sizes are written out here, not taken from the header; WLayout::dp is the one exception: it is
// addressed float by float at a row stride of T' and starts wherever B puts it - (3) the sub-offsets of WLayout::small are
// those of the hand arithmetic the head's backward used, (4) the LDS footprints are the recorded numbers, the static ones
// within 64 KiB, the dynamic one within 160 KiB and above 64 KiB exactly for H = 128, when the launcher raises the attribute.
// Prints "ok <row>" per row; exit status 1 on the first failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cnnlstm_layout.h"

using namespace rsaf::cnnlstm;

struct Row {
    const char* name;
    int D, C, H, NC, L, B, T;
    int64_t weight_floats;
    int nw;
    int64_t woff[26];
    int64_t ws_bytes, param_floats;
    int np;
    int64_t poff[36];
    int64_t saved_floats, scratch_floats;
};
struct LdsRow { int H; long rec, rec4, rec4_halves, bwd, bwd4, bwd4_halves; };

#include "cnnlstm_layout_parent.inc"

static const char* g_row = "";
static void fail(const std::string& what) {
    std::printf("FAIL %s: %s\n", g_row, what.c_str());
    std::exit(1);
}
static void expect(int64_t got, int64_t want, const std::string& what) {
    if (got != want) fail(what + ": " + std::to_string(got) + ", expected " + std::to_string(want));
}

struct Seg { std::string name; int64_t begin, floats; int align_bytes; };

// every segment inside [lo, hi) floats, aligned, and no two overlapping; a segment the layout leaves out (offset -1) has size -1
static void check_segs(const char* layout, std::vector<Seg> s, int64_t lo, int64_t hi) {
    std::vector<Seg> live;
    for (const Seg& a : s) {
        if (a.floats < 0) {
            if (a.begin != -1) fail(std::string(layout) + "." + a.name + " should be absent (-1)");
            continue;
        }
        if (a.begin < lo || a.floats <= 0 || a.begin + a.floats > hi)
            fail(std::string(layout) + "." + a.name + " [" + std::to_string(a.begin) + ", " + std::to_string(a.begin + a.floats) + ") leaves [" +
                 std::to_string(lo) + ", " + std::to_string(hi) + ")");
        if (a.begin * 4 % a.align_bytes) fail(std::string(layout) + "." + a.name + " is not " + std::to_string(a.align_bytes) + "-byte aligned");
        live.push_back(a);
    }
    std::sort(live.begin(), live.end(), [](const Seg& a, const Seg& b) { return a.begin < b.begin; });
    for (size_t i = 1; i < live.size(); ++i)
        if (live[i - 1].begin + live[i - 1].floats > live[i].begin) fail(std::string(layout) + "." + live[i - 1].name + " overlaps " + live[i].name);
}

static void expect_list(const std::vector<int64_t>& got, const int64_t* want, int n, const char* what) {
    expect((int64_t)got.size(), n, std::string(what) + " count");
    for (int i = 0; i < n; ++i) expect(got[i], want[i], std::string(what) + "[" + std::to_string(i) + "]");
}

static void check_row(const Row& R) {
    g_row = R.name;
    const Dims d{R.D, R.C, R.H, R.NC, R.L, DIMS_ACT_SILU};
    const int64_t D = R.D, C = R.C, H = R.H, NC = R.NC, B = R.B, T = R.T, Tp = R.T / 2, F = 2 * H;
    const bool sc = D != C;
    const auto lname = [](const char* n, int l) { return std::string(n) + "[" + std::to_string(l) + "]"; };
    if (dims_problem(d, 0) || dims_problem(d, TRAIN_C_MAX)) fail("dims_problem refuses the row");

    // ---- inference weight blob
    const Layout L = make_layout(d);
    expect(L.total, R.weight_floats, "weight floats");
    {
        std::vector<int64_t> off = {L.w1, L.b1, L.wsc, L.bsc, L.w2, L.b2, L.w3, L.b3, L.w4, L.b4};
        std::vector<Seg> s = {{"w1", L.w1, C * 3 * D, 16}, {"b1", L.b1, C, 16}, {"wsc", L.wsc, sc ? C * D : -1, 16}, {"bsc", L.bsc, sc ? C : -1, 16},
                              {"w2", L.w2, C * 3 * C, 16}, {"b2", L.b2, C, 16}, {"w3", L.w3, C * 3 * C, 16}, {"b3", L.b3, C, 16},
                              {"w4", L.w4, C * 3 * C, 16}, {"b4", L.b4, C, 16}};
        for (int l = 0; l < R.L; ++l) {
            off.insert(off.end(), {L.wih[l], L.bih[l], L.whh[l]});
            s.push_back({lname("wih", l), L.wih[l], 8 * H * (l == 0 ? C : F), 16});
            s.push_back({lname("bih", l), L.bih[l], 8 * H, 16});
            s.push_back({lname("whh", l), L.whh[l], 2 * 4 * H * H, 16});
        }
        off.insert(off.end(), {L.watt, L.batt, L.wfc, L.bfc});
        s.insert(s.end(), {{"watt", L.watt, F, 16}, {"batt", L.batt, 1, 16}, {"wfc", L.wfc, NC * F, 16}, {"bfc", L.bfc, NC, 16}});
        expect_list(off, R.woff, R.nw, "weight offset");
        check_segs("Layout", s, 0, L.total);
    }

    // ---- inference workspace: the fp32 buffers and, at the widths that take it, the f16x3 front behind them
    const InferWs W = make_infer_ws(d, R.B, R.T);
    expect(W.total * 4, R.ws_bytes, "workspace bytes");
    expect(W.f16, D % 16 == 0 && C % 16 == 0, "use_f16x3");
    check_segs("InferWs",
               {{"bufA", W.bufA, B * T * C, 16}, {"bufB", W.bufB, B * T * C, 16}, {"bufC", W.bufC, B * T * C, 16}, {"xproj", W.xproj, B * Tp * 8 * H, 16},
                {"seq0", W.seq0, B * Tp * F, 16}, {"seq1", W.seq1, B * Tp * F, 16}, {"f16", W.f16 ? W.f16base : -1, W.f16 ? W.F.total : -1, 16}},
               0, W.total);
    if (W.f16) {
        const F16Ws& P = W.F;                    // a plane pair of n elements is 2 planes x n x 2 bytes = n floats
        std::vector<Seg> s = {{"xp", P.xp, B * (T + 2) * D, 16}, {"c1p", P.c1p, B * (T + 2) * C, 16}, {"poolp", P.poolp, B * (Tp + 2) * C, 16},
                              {"c3p", P.c3p, B * (Tp + 2) * C, 16}, {"c4p", P.c4p, B * Tp * C, 16}, {"hp", P.hp, B * Tp * F, 16},
                              {"stat", P.stat, 2 * (5 + 5 + 4), 16}, {"amax", P.amax, 6 * B, 16}, {"scale", P.scale, 6 * B, 16}, {"one", P.one, 1, 16}};
        const int64_t wsz[5] = {C * 3 * D, C * D, C * 3 * C, C * 3 * C, C * 3 * C};
        for (int i = 0; i < 5; ++i) { s.push_back({lname("wp", i), P.wp[i], wsz[i], 16}); s.push_back({lname("ws", i), P.ws[i], C, 16}); }
        for (int l = 0; l < R.L; ++l) {
            s.push_back({lname("wih_p", l), P.wih_p[l], 8 * H * (l == 0 ? C : F), 16});
            s.push_back({lname("wih_s", l), P.wih_s[l], 8 * H, 16});
        }
        check_segs("F16Ws", s, 0, P.total);
        // the named slots: amax and scale rows inside their [6][B] areas, the statistics inside [CNN_NSTAT][2]
        expect(CNN_NAMAX, 6, "CNN_NAMAX"); expect(CNN_NSCALE, 6, "CNN_NSCALE"); expect(CNN_NSTAT, 14, "CNN_NSTAT");
        const int am[6] = {AX, ASC, AC1, AC2, AC3, AC4}, sl[5] = {SX, SC1, SPOOL, SC3, SC4};
        for (int i = 0; i < 6; ++i) expect(am[i], i, "amax slot");
        for (int i = 0; i < 5; ++i) expect(sl[i], i, "scale slot");
        const int wi[5] = {W1, WSC, W2, W3, W4};
        for (int i = 0; i < 5; ++i) { expect(wi[i], i, "weight index"); expect(stat_w(i), i, "stat_w"); expect(stat_b(i), 5 + i, "stat_b"); }
        for (int l = 0; l < 4; ++l) expect(stat_wih(l), 10 + l, "stat_wih");
    }

    // ---- training parameter / gradient blob
    const PLayout PL = make_playout(d);
    expect(PL.total, R.param_floats, "param floats");
    {
        std::vector<int64_t> off;
        std::vector<Seg> s;
        const struct { const char* n; const ConvP* c; int64_t w; } cv[5] = {{"c1", &PL.c1, C * 3 * D}, {"sc", &PL.sc, sc ? C * D : -1}, {"c2", &PL.c2, C * 3 * C},
                                                                            {"c3", &PL.c3, C * 3 * C}, {"c4", &PL.c4, C * 3 * C}};
        for (const auto& v : cv) {
            off.insert(off.end(), {v.c->w, v.c->b, v.c->g, v.c->be});
            const int64_t n = v.w < 0 ? -1 : C;
            s.insert(s.end(), {{std::string(v.n) + ".w", v.c->w, v.w, 16}, {std::string(v.n) + ".b", v.c->b, n, 16},
                               {std::string(v.n) + ".g", v.c->g, n, 16}, {std::string(v.n) + ".be", v.c->be, n, 16}});
        }
        for (int l = 0; l < R.L; ++l) {
            off.insert(off.end(), {PL.wih[l], PL.bsum[l], PL.whh[l]});
            s.push_back({lname("wih", l), PL.wih[l], 8 * H * (l == 0 ? C : F), 16});
            s.push_back({lname("bsum", l), PL.bsum[l], 8 * H, 16});
            s.push_back({lname("whh", l), PL.whh[l], 2 * 4 * H * H, 16});
        }
        off.insert(off.end(), {PL.watt, PL.batt, PL.wfc, PL.bfc});
        s.insert(s.end(), {{"watt", PL.watt, F, 16}, {"batt", PL.batt, 1, 16}, {"wfc", PL.wfc, NC * F, 16}, {"bfc", PL.bfc, NC, 16}});
        expect_list(off, R.poff, R.np, "param offset");
        check_segs("PLayout", s, 0, PL.total);
    }

    // ---- training saved activations
    const SLayout S = make_slayout(d, R.B, R.T);
    expect(S.total, R.saved_floats, "saved floats");
    {
        const int64_t n1 = B * T * C, n2 = B * Tp * C;
        std::vector<Seg> s = {{"stat", S.stat, 5 * 3 * C, 16}, {"y1", S.y1, n1, 16}, {"ysc", S.ysc, sc ? n1 : -1, 16}, {"a1d", S.a1d, n1, 16},
                              {"y2", S.y2, n1, 16}, {"z1", S.z1, n1, 16}, {"p", S.p, n2, 16}, {"y3", S.y3, n2, 16}, {"a3d", S.a3d, n2, 16},
                              {"y4", S.y4, n2, 16}, {"z2", S.z2, n2, 16}, {"r2", S.r2, n2, 16}, {"prob", S.prob, B * Tp, 16}, {"ctx", S.ctx, B * F, 16}};
        for (int l = 0; l < R.L; ++l) {
            s.push_back({lname("gates", l), S.gates[l], B * Tp * 8 * H, 16});
            s.push_back({lname("cst", l), S.cst[l], B * Tp * F, 16});
            s.push_back({lname("hout", l), S.hout[l], B * Tp * F, 16});
            s.push_back({lname("hdrop", l), S.hdrop[l], l < R.L - 1 ? B * Tp * F : -1, 16});
        }
        check_segs("SLayout", s, 0, S.total);
    }

    // ---- training scratch
    const WLayout WL = make_wlayout(d, R.B, R.T);
    expect(WL.total, R.scratch_floats, "scratch floats");
    {
        const int64_t rows = B * T;
        int64_t kc = 1024;
        while ((rows + kc - 1) / kc > 4096) kc *= 2;
        const int64_t s_ = std::max<int64_t>((rows + kc - 1) / kc, 1), kp = s_ * kc;
        const Split sp = make_split(rows);
        expect(sp.kc, kc, "Split.kc"); expect(sp.s, s_, "Split.s"); expect(sp.kp, kp, "Split.kp");
        expect(sp.kc, rows > 4096 * 1024 ? 2048 : 1024, "Split.kc at this B T");
        expect(RED_PARTS, 256, "RED_PARTS");
        const int64_t nb = std::max(B * T * C, B * Tp * std::max(C, F));
        const int64_t mn = std::max(C * 3 * std::max(D, C), 8 * H * std::max(C, F));
        check_segs("WLayout",
                   {{"bufA", WL.bufA, nb, 16}, {"bufB", WL.bufB, nb, 16}, {"bufC", WL.bufC, nb, 16}, {"t1", WL.t1, std::max(C, 8 * H) * kp, 16},
                    {"t2", WL.t2, std::max(std::max(3 * D, 3 * C), F) * kp, 16}, {"part", WL.part, s_ * mn, 16},
                    {"red (doubles)", WL.red, 2 * (256 * 2 * std::max(C, 8 * H)), 16}, {"wflip", WL.wflip, C * 3 * C, 16},
                    {"small", WL.small, WL.total - WL.small, 16}},
                   0, WL.total);
        // small: the last segment of the scratch, carved into five; the BatchNorm sums hold [2][1024] (the training cap on C)
        expect(TRAIN_C_MAX, 1024, "TRAIN_C_MAX");
        check_segs("WLayout.small",
                   {{"bn_sums", WL.bn_sums, 2 * 1024, 16}, {"dctx", WL.dctx, B * F, 16}, {"dwatt_part", WL.dwatt_part, B * F, 16},
                    {"dbatt_part", WL.dbatt_part, B, 16}, {"dp", WL.dp, B * Tp, 4}},
                   WL.small, WL.total);
        // the hand arithmetic of the head's backward and of the BatchNorm backward
        expect(WL.bn_sums, WL.small, "small.bn_sums");
        expect(WL.dctx, WL.small + 2 * 1024 + 64, "small.dctx");
        expect(WL.dwatt_part, WL.dctx + B * F, "small.dwatt_part");
        expect(WL.dbatt_part, WL.dwatt_part + B * F, "small.dbatt_part");
        expect(WL.dp, WL.dbatt_part + B + 4, "small.dp");
    }

    // ---- LDS of the recurrences at this H
    const LdsRow* P = nullptr;
    for (const LdsRow& r : PARENT_LDS)
        if (r.H == R.H) P = &r;
    if (!P) fail("no LDS row for this H");
    const long KiB = 1024;
    expect(rec_lds_floats(R.H) * 4L, P->rec, "LDS lstm_rec_kernel");
    expect(rec4_lds_floats(R.H, 1) * 4L, P->rec4, "LDS lstm_rec4_body");
    expect(bwd_lds_floats(R.H) * 4L, P->bwd, "LDS lstm_bwd_kernel (dynamic)");
    expect(bwd4_lds_floats(R.H, 1) * 4L, P->bwd4, "LDS lstm_bwd4_body");
    if (R.H == 64) {
        expect(rec4_lds_floats(64, 2) * 4L, P->rec4_halves, "LDS lstm_rec4_body, two halves");
        expect(bwd4_lds_floats(64, 2) * 4L, P->bwd4_halves, "LDS lstm_bwd4_body, two halves");
    }
    const long mixed_fwd = (rec4_lds_floats(128, 1) + rec4_lds_floats(64, 2)) * 4L, mixed_bwd = (bwd4_lds_floats(128, 1) + bwd4_lds_floats(64, 2)) * 4L;
    expect(mixed_fwd, PARENT_LDS_MIXED_FWD, "LDS lstm_rec4_group_mixed_kernel");
    expect(mixed_bwd, PARENT_LDS_MIXED_BWD, "LDS lstm_bwd4_group_mixed_kernel");
    for (long b : {rec_lds_floats(R.H) * 4L, rec4_lds_floats(R.H, 1) * 4L, bwd4_lds_floats(R.H, 1) * 4L, mixed_fwd, mixed_bwd})
        if (b > 64 * KiB) fail("a static LDS footprint exceeds 64 KiB");
    const long dyn = bwd_lds_floats(R.H) * 4L;
    if (dyn > 160 * KiB) fail("the dynamic LDS request exceeds 160 KiB");
    if ((dyn > 64 * KiB) != (R.H == 128)) fail("the dynamic LDS request is above 64 KiB exactly for H = 128");
    std::printf("ok %s\n", R.name);
}

int main() {
    // the caps of dims_problem: the inference entries take any C, the training entries stop at TRAIN_C_MAX, each with its message
    g_row = "dims_problem";
    const Dims wide{64, 1028, 64, 2, 1, DIMS_ACT_SILU};
    if (dims_problem(wide, 0)) fail("C = 1028 refused without a cap");
    if (std::string(dims_problem(wide, TRAIN_C_MAX)) != "cnn_out_channels must be a multiple of 4 in [4, 1024]") fail("C = 1028 under the training cap");
    const Dims odd{64, 6, 64, 2, 1, DIMS_ACT_SILU};
    if (std::string(dims_problem(odd, 0)) != "cnn_out_channels must be a positive multiple of 4") fail("C = 6 without a cap");
    for (const Row& R : PARENT_ROWS) check_row(R);
    return 0;
}
