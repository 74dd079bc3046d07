// csrc/w2v2_layout.h on the host: the weight layout, the workspace, the window geometry, the path predicates and the three
// dynamic-LDS layouts of the Wav2Vec2 forward, at the published geometries (tools/w2v2_variant_rate.py) and the small test
// geometries, each crossed with four window sets.  Per row: (1) Layout.total, the offset list in the order
// rsaf_w2v2_weight_offsets_ex emits it and the workspace bytes equal the numbers recorded from the library before the split
// (w2v2_layout_parent.inc); (2) every weight and workspace segment, with the size written out here, lies inside its total,
// no two overlap, every offset is a multiple of 4 floats and the int64 tables are 8-byte aligned; (3) the packed row tables
// of every window group fit their buffers; (4) Rag equals a recomputation made here; (5) the LDS layouts request what the
// formulas of the kernels' first form gave, stay within 160 KiB where their kernel runs, and their arrays are inside the
// request, disjoint and 16-byte aligned; (6) the predicates take the recorded values.
// With the argument `regimes`: the regime runs of ragged calls instead (see regimes_main).
// Prints "ok <row>" per row; exit status 1 on the first failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "w2v2_layout.h"

using namespace rsaf::w2v2;

struct Geom { const char* name; Cfg c; int64_t total; const int64_t* offs; int n_offs; };
struct Want { int64_t ws_bytes; int fused, on_f16x3, stack_mfma, split, resident; };
#include "w2v2_layout_parent.inc"

struct WinSet { const char* name; std::vector<int> len; };
static std::vector<WinSet> window_sets() {
    return {{"448x80000", std::vector<int>(448, 80000)},
            {"1x400", {400}},
            {"ragged", {170000, 100000, 100000, 80000, 80000, 80000, 3000, 3000, 400}},   // 531, 312 x 2, 249 x 3, 9 x 2, 1 frames
            {"513x80000", std::vector<int>(513, 80000)}};
}

static std::string g_row;
static void fail(const std::string& what) {
    std::printf("FAIL %s: %s\n", g_row.c_str(), what.c_str());
    std::exit(1);
}
static void expect(int64_t got, int64_t want, const std::string& what) {
    if (got != want) fail(what + ": " + std::to_string(got) + ", expected " + std::to_string(want));
}

struct Span { std::string name; int64_t begin, size; };
// every segment inside [0, total), its start a multiple of `align`, no two overlapping (units: the caller's)
static void check_spans(const char* what, std::vector<Span> s, int64_t total, int64_t align) {
    for (const Span& a : s) {
        if (a.begin < 0 || a.size <= 0 || a.begin + a.size > total)
            fail(std::string(what) + "." + a.name + " [" + std::to_string(a.begin) + ", " + std::to_string(a.begin + a.size) +
                 ") leaves the total of " + std::to_string(total));
        if (a.begin % align) fail(std::string(what) + "." + a.name + " is not aligned to " + std::to_string(align));
    }
    std::sort(s.begin(), s.end(), [](const Span& a, const Span& b) { return a.begin < b.begin; });
    for (size_t i = 1; i < s.size(); ++i)
        if (s[i - 1].begin + s[i - 1].size > s[i].begin) fail(std::string(what) + "." + s[i - 1].name + " overlaps " + s[i].name);
}

// frames after each of the seven convolutions (taps 10 3 3 3 3 2 2, strides 5 2 2 2 2 2 2), written out independently
static void frames7(int len, int T[7]) {
    static const int k[7] = {10, 3, 3, 3, 3, 2, 2}, s[7] = {5, 2, 2, 2, 2, 2, 2};
    for (int i = 0; i < 7; ++i) { len = len >= k[i] ? (len - k[i]) / s[i] + 1 : 0; T[i] = len; }
}

static void check_weights(const Geom& g) {
    const Cfg& c = g.c;
    const Layout L = make_layout(c);
    expect(L.total, g.total, "Layout.total");
    const int64_t C = c.C, Hd = c.Hd, I = c.I, cg = c.Hd / c.PG, hd = c.Hd / c.NH;
    static const int k[6] = {3, 3, 3, 3, 2, 2};
    // the segments with their sizes in floats, in the order of rsaf_w2v2_weight_offsets_ex (the appended [rows][C] segments
    // are listed there row by row)
    std::vector<Span> s = {{"conv0", L.conv0, C * 10}, {"gng", L.gng, C}, {"gnb", L.gnb, C}};
    for (int i = 0; i < 6; ++i) s.push_back({"conv" + std::to_string(i + 1), L.conv[i], C * k[i] * C});
    s.insert(s.end(), {{"fplg", L.fplg, C}, {"fplb", L.fplb, C}, {"fpw", L.fpw, Hd * C}, {"fpb", L.fpb, Hd},
                       {"posw", L.posw, Hd * c.PK * cg}, {"posb", L.posb, Hd}, {"elng", L.elng, Hd}, {"elnb", L.elnb, Hd}});
    expect((int64_t)L.layers.size(), c.L, "Layout.layers");
    for (const LayerOff& lo : L.layers)
        s.insert(s.end(), {{"wqkv", lo.wqkv, 3 * Hd * Hd}, {"bqkv", lo.bqkv, 3 * Hd}, {"wo", lo.wo, Hd * Hd}, {"bo", lo.bo, Hd},
                           {"ln1g", lo.ln1g, Hd}, {"ln1b", lo.ln1b, Hd}, {"w1", lo.w1, I * Hd}, {"b1", lo.b1, I},
                           {"w2", lo.w2, Hd * I}, {"b2", lo.b2, Hd}, {"ln2g", lo.ln2g, Hd}, {"ln2b", lo.ln2b, Hd}});
    std::vector<int64_t> order;
    for (const Span& a : s) order.push_back(a.begin);
    expect(L.cb >= 0, (c.flags & F_CONV_BIAS) != 0, "Layout.cb present");
    expect(L.cln >= 0, (c.flags & F_LAYER_FEAT_NORM) != 0, "Layout.cln present");
    if (L.cb >= 0) { s.push_back({"cb", L.cb, 7 * C}); for (int i = 0; i < 7; ++i) order.push_back(L.cb + i * C); }
    if (L.cln >= 0) { s.push_back({"cln", L.cln, 14 * C}); for (int i = 0; i < 14; ++i) order.push_back(L.cln + i * C); }
    expect(L.reltab >= 0, (c.flags & F_REL_POS_BIAS) != 0, "Layout.reltab present");
    if (L.reltab >= 0) {
        expect((int64_t)L.ga.size(), c.L, "Layout.ga");
        for (int l = 0; l < c.L; ++l) {
            s.insert(s.end(), {{"ga", L.ga[l], hd}, {"gb", L.gb[l], hd}, {"gbias", L.gbias[l], 2}, {"gconst", L.gconst[l], c.NH}});
            order.insert(order.end(), {L.ga[l], L.gb[l], L.gbias[l], L.gconst[l]});
        }
        s.push_back({"reltab", L.reltab, (int64_t)c.NH * (2 * RSAF_W2V2_REL_SPAN - 1)});
        order.push_back(L.reltab);
    }
    expect((int64_t)L.stackw.size(), std::max(c.pos_depth() - 1, 0), "Layout.stackw");
    for (size_t i = 0; i < L.stackw.size(); ++i) {
        s.insert(s.end(), {{"stackw", L.stackw[i], Hd * c.PK * cg}, {"stackb", L.stackb[i], Hd}});
        order.insert(order.end(), {L.stackw[i], L.stackb[i]});
    }
    expect((int64_t)order.size(), g.n_offs, "number of offsets");
    for (int i = 0; i < g.n_offs; ++i) expect(order[i], g.offs[i], "offset " + std::to_string(i));
    check_spans("Layout", s, L.total, 4);
}

static void check_workspace(const Cfg& c, const Rag& R, const Workspace& W, int64_t want_bytes) {
    expect(W.total * 4, want_bytes, "Workspace.total * 4");
    const int64_t n = R.n, C = c.C, Hd = c.Hd, I = c.I, rows = R.rows, G = std::min<int64_t>(n, 512), Tt = R.Tmax[6];
    const int* T = R.Tmax;
    const int64_t wpos = Hd * c.PK * (Hd / c.PG);
    static const int k[6] = {3, 3, 3, 3, 2, 2};
    int64_t crow = 0;                                        // {slot, destination} per packed row: G (T_i + 1) rows per conv 1..6
    for (int i = 1; i < 7; ++i) crow += G * (T[i] + 1);
    // the sizes in floats; a pair of fp16 planes of N elements takes N floats
    std::vector<Span> s = {
        {"xn", W.xn, G * R.maxlen}, {"part", W.part, G * ((T[0] + 511) / 512) * 3 * C}, {"ab", W.ab, G * 2 * C},
        {"P", W.P, (2 * G * (T[1] + 1) + 1) * C}, {"Q", W.Q, (2 * G * (T[2] + 1) + 1) * C}, {"c6", W.c6, rows * C},
        {"lnfp", W.lnfp, rows * C}, {"x", W.x, rows * Hd}, {"xp", W.xp, rows * Hd}, {"y", W.y, rows * Hd}, {"att", W.att, rows * Hd},
        {"attp", W.attp, rows * Hd}, {"xg", W.xg, n * (Tt + c.PK - 1) * Hd}, {"qkv", W.qkv, rows * 3 * Hd},
        {"S", W.S, (c.Hd / c.NH == 64 && Tt <= 256) ? 4 : n * c.NH * Tt * ((Tt + 3) / 4 * 4)}, {"ffnp", W.ffnp, rows * I},
        {"wp_fp", W.wp_fp, Hd * C}, {"ws_fp", W.ws_fp, Hd}, {"wp_pos", W.wp_pos, wpos}, {"ws_pos", W.ws_pos, Hd},
        {"wstat", W.wstat, (8 + 6 * c.L) * 2}, {"conv_scale", W.conv_scale, 7 * G}, {"conv_amax", W.conv_amax, 7 * G},
        {"pos_scale", W.pos_scale, n}, {"fp_amax", W.fp_amax, n}, {"wlen", W.wlen, n}, {"win_norm", W.win_norm, n},
        {"s_lnfp", W.s_lnfp, rows}, {"s_x", W.s_x, rows}, {"s_ffn", W.s_ffn, rows}, {"s_att", W.s_att, rows}, {"s_qkv", W.s_qkv, rows},
        {"t_Tw", W.t_Tw, 7 * n}, {"t_row0", W.t_row0, 2 * (n + 1)}, {"t_ztab", W.t_ztab, 7 * n * 2 * 2}, {"t_rowwin", W.t_rowwin, rows},
        {"t_coff", W.t_coff, 7 * (G + 1)}, {"t_crow", W.t_crow, 2 * crow}};
    for (int i = 0; i < 6; ++i) {
        s.push_back({"wp_conv" + std::to_string(i), W.wp_conv[i], C * k[i] * C});
        s.push_back({"ws_conv" + std::to_string(i), W.ws_conv[i], C});
    }
    expect((int64_t)W.wp_qkv.size(), c.L, "Workspace.wp_qkv");
    for (int l = 0; l < c.L; ++l)
        s.insert(s.end(), {{"wp_qkv", W.wp_qkv[l], 3 * Hd * Hd}, {"ws_qkv", W.ws_qkv[l], 3 * Hd}, {"wp_o", W.wp_o[l], Hd * Hd},
                           {"ws_o", W.ws_o[l], Hd}, {"wp_1", W.wp_1[l], I * Hd}, {"ws_1", W.ws_1[l], I}, {"wp_2", W.wp_2[l], Hd * I},
                           {"ws_2", W.ws_2[l], Hd}});
    expect(W.cb_max >= 0, (c.flags & F_CONV_BIAS) != 0, "Workspace.cb_max present");
    if (W.cb_max >= 0) s.push_back({"cb_max", W.cb_max, 8});
    expect(W.gate >= 0, (c.flags & F_REL_POS_BIAS) != 0, "Workspace.gate present");
    if (W.gate >= 0) s.push_back({"gate", W.gate, rows * c.NH});
    const int cgw = c.Hd / c.PG;
    const bool stack_planes = c.pos_depth() > 0 && cgw % 16 == 0 && cgw <= 64;
    expect((int64_t)W.wp_stack.size(), stack_planes ? c.pos_depth() - 1 : 0, "Workspace.wp_stack");
    for (size_t i = 0; i < W.wp_stack.size(); ++i) s.insert(s.end(), {{"wp_stack", W.wp_stack[i], wpos}, {"ws_stack", W.ws_stack[i], Hd}});
    check_spans("Workspace", s, W.total, 4);
    if ((W.t_row0 * 4) % 8 || (W.t_ztab * 4) % 8) fail("an int64 table is not 8-byte aligned");
}

// the feature encoder's passes (Forward::feature_encoder): ceil(n / G) groups of (almost) equal size; per group the rows of
// conv i's GEMM are M_i = sum over its windows of T_i + 1
static void check_packed_rows(const Rag& R) {
    const int n = R.n, G = conv_group(n), n_groups = (n + G - 1) / G, gstep = (n + n_groups - 1) / n_groups;
    const int* T = R.Tmax;
    // layer mode: P holds G x T[0] rows of planes, Q the G x T[1] fp32 rows of the widest GEMM output
    if ((int64_t)G * T[0] > p_rows(G, T) || (int64_t)G * T[1] > q_rows(G, T)) fail("layer mode's rows exceed P or Q");
    for (int g0 = 0; g0 < n; g0 += gstep) {
        const int g = std::min(gstep, n - g0);
        if (g > G) fail("a window group exceeds the slots of a pass");
        int64_t M[7] = {}, sum = 0;
        for (int w = g0; w < g0 + g; ++w) {
            int Tw[7];
            frames7(R.len[w], Tw);
            for (int i = 1; i < 7; ++i) M[i] += Tw[i] + 1;
        }
        for (int i = 1; i < 7; ++i) {
            // the input space of conv i (2 M_i rows and the junk row's reach) lives in P (i odd) or Q (i even)
            const int64_t have = (i & 1) ? p_rows(G, T) : q_rows(G, T);
            if (2 * M[i] + 1 > have) fail("conv" + std::to_string(i) + ": 2 M + 1 = " + std::to_string(2 * M[i] + 1) + " rows exceed the buffer's " + std::to_string(have));
            if (packed_tab_base(G, T, i) + M[i] > packed_tab_base(G, T, i + 1)) fail("row table of conv" + std::to_string(i) + " runs into the next");
            sum += M[i];
        }
        if (sum > packed_tab_base(G, T, 7)) fail("the row tables exceed t_crow");      // t_crow holds 2 packed_tab_base(G, T, 7) ints
    }
}

static void check_rag(const std::vector<int>& len, const Rag& R) {
    expect(R.n, (int64_t)len.size(), "Rag.n");
    expect(R.maxlen, len[0], "Rag.maxlen");
    int64_t rows = 0;
    std::vector<std::pair<int, int>> runs;
    for (size_t w = 0; w < len.size(); ++w) {
        int T[7];
        frames7(len[w], T);
        expect(R.row0[w], rows, "Rag.row0[" + std::to_string(w) + "]");
        expect(R.T6[w], T[6], "Rag.T6");
        if (w == 0) for (int i = 0; i < 7; ++i) expect(R.Tmax[i], T[i], "Rag.Tmax[" + std::to_string(i) + "]");
        int Tp[7] = {};
        if (w > 0) frames7(len[w - 1], Tp);
        if (w == 0 || Tp[6] != T[6]) runs.push_back({(int)w, (int)w + 1});
        else runs.back().second = (int)w + 1;
        rows += T[6];
    }
    expect(R.row0[len.size()], rows, "Rag.row0[n]");
    expect(R.rows, rows, "Rag.rows");
    expect((int64_t)R.tgroups.size(), (int64_t)runs.size(), "Rag.tgroups");
    for (size_t i = 0; i < runs.size(); ++i) {
        expect(R.tgroups[i].first, runs[i].first, "Rag.tgroups.begin");
        expect(R.tgroups[i].second, runs[i].second, "Rag.tgroups.end");
    }
}

static void check_lds(const Cfg& c, int Tt, const Want& want) {
    const int cg = c.Hd / c.PG, nt = cg / 16;
    const int64_t KiB160 = 160 * 1024;
    // attention: two blocks of 128 keys x 64 halfs x 2 planes
    expect((int64_t)AttnLds::bytes(), 2 * 2 * 128 * 64 * 2, "AttnLds.bytes");
    expect((int64_t)AttnLds::bytes(), 65536, "AttnLds.bytes");
    check_spans("AttnLds", {{"block0", 2 * AttnLds::BLOCK0, 2 * 2 * AttnLds::PLANE}, {"block1", 2 * AttnLds::BLOCK1, 2 * 2 * AttnLds::PLANE}},
                (int64_t)AttnLds::bytes(), 16);
    if (nt < 1) return;                                      // the two positional kernels need group widths of 16 NT
    for (int split = 1; split <= 2; ++split) {
        const PosconvLds p = PosconvLds::make(cg, c.PK, split);
        const int64_t rows_alloc = (512 / split + c.PK - 1 + 31) & ~31;
        expect(p.rows_alloc, rows_alloc, "PosconvLds.rows_alloc");
        expect((int64_t)p.bytes(), (2 * (cg / 16) * rows_alloc * 16 + (int64_t)4 * split * 4 * cg * 16) * 2, "PosconvLds.bytes");
        if (512 / split + c.PK - 1 > p.rows_alloc) fail("PosconvLds: the image rows do not hold a tile and its taps");
        std::vector<Span> s;
        for (int pl = 0; pl < 2; ++pl)
            for (int q = 0; q < nt; ++q)
                s.push_back({"image", 2 * (int64_t)((pl * nt + q) * p.a_panel()), 2 * (int64_t)p.a_panel()});
        for (int slot = 0; slot < 4; ++slot)
            for (int kh = 0; kh < split; ++kh)
                s.push_back({"stage", 2 * (int64_t)(p.ring() + p.stage(slot, kh)), 2 * (int64_t)PosconvLds::stage_elems(nt)});
        check_spans("PosconvLds", s, (int64_t)p.bytes(), 16);
        if (split == 2) {                                    // the exchange takes the image's place: inside it, groups disjoint
            std::vector<Span> x;
            for (int grp = 0; grp < 8 / split; ++grp) x.push_back({"exchange", 4 * (int64_t)p.exchange(grp), 4 * (int64_t)(4 * nt * 4 * 64)});
            check_spans("PosconvLds", x, 2 * (int64_t)p.ring(), 16);
        }
    }
    if (want.on_f16x3 && want.resident && (int64_t)PosconvLds::make(cg, c.PK, want.split).bytes() > KiB160) fail("PosconvLds above 160 KiB where the kernel runs");
    if (nt <= 4) {
        const PosstackLds p = PosstackLds::make(cg, c.PK);
        expect(p.rows_alloc, 256 + c.PK - 1, "PosstackLds.rows_alloc");
        expect((int64_t)p.bytes(), (int64_t)2 * cg * (256 + c.PK - 1) * 2, "PosstackLds.bytes");
        std::vector<Span> s;
        for (int pl = 0; pl < 2; ++pl)
            for (int q = 0; q < nt; ++q) s.push_back({"panel", 2 * (int64_t)p.panel(pl, q), 2 * (int64_t)p.a_panel()});
        check_spans("PosstackLds", s, (int64_t)p.bytes(), 16);
        if (want.stack_mfma && (int64_t)p.bytes() > KiB160) fail("PosstackLds above 160 KiB where the kernel runs");
    }
    (void)Tt;
}

// ---- regime runs of a ragged call (`w2v2_layout_replay regimes`) -------------------------------------------------------------
// A call whose windows span regimes is run as one sub-call per regime run in the caller's workspace.  Over every
// non-increasing list of one to four windows with frame counts either side of 256, 512 and 513, at head widths 64 and 16,
// with and without POS_CONV_STACK: the runs partition the list in order, each run is uniform under the predicates that pick
// a path at its geometry (fused_attention always; posconv_resident, and posconv_split where resident, on the f16x3
// positional path without a stack), neighbouring runs differ in one of them, and a run's workspace is no larger than the call's.
struct PathPick { int fused, resident, split; };
static PathPick path_pick(const Cfg& c, int Tt) {
    const bool lds_path = c.pos_depth() == 0 && posconv_on_f16x3(c);
    const bool res = lds_path && posconv_resident(c, Tt);
    return {fused_attention(c, Tt), res, res ? posconv_split(Tt) : 0};
}
static bool same_pick(const PathPick& a, const PathPick& b) { return a.fused == b.fused && a.resident == b.resident && a.split == b.split; }

static int64_t check_regime_runs(const Cfg& c, const std::vector<int>& frames) {
    std::vector<int> len;
    for (int T : frames) len.push_back(400 + 320 * (T - 1));
    Rag R;
    if (const char* msg = make_rag(len.data(), (int)len.size(), 0, R)) fail(std::string("make_rag: ") + msg);
    for (size_t w = 0; w < frames.size(); ++w) expect(R.T6[w], frames[w], "frames of a window");
    const std::vector<std::pair<int, int>> runs = regime_runs(c, R);
    const int64_t call_total = make_ws(c, R).total;
    int next = 0;
    for (size_t r = 0; r < runs.size(); ++r) {
        expect(runs[r].first, next, "a run begins where the last one ended");
        if (runs[r].second <= runs[r].first) fail("an empty run");
        next = runs[r].second;
        const PathPick first = path_pick(c, R.T6[runs[r].first]);
        for (int w = runs[r].first; w < runs[r].second; ++w)
            if (!same_pick(path_pick(c, R.T6[w]), first)) fail("a run mixes paths at T = " + std::to_string(R.T6[w]));
        if (r > 0 && same_pick(path_pick(c, R.T6[runs[r - 1].first]), first)) fail("two neighbouring runs take the same paths");
        const Regime g = window_regime(c, R.T6[runs[r].first]);
        expect(g.fused, first.fused, "Regime.fused");
        expect(g.posconv, first.split, "Regime.posconv");
        Rag Rr;
        if (const char* msg = make_rag(len.data() + runs[r].first, runs[r].second - runs[r].first, 0, Rr)) fail(std::string("make_rag(run): ") + msg);
        expect(Rr.rows, R.row0[runs[r].second] - R.row0[runs[r].first], "rows of a run");
        const int64_t run_total = make_ws(c, Rr).total;
        if (run_total > call_total)
            fail("a run needs " + std::to_string(run_total) + " floats of workspace, the call has " + std::to_string(call_total));
    }
    expect(next, R.n, "the runs end at the last window");
    return (int64_t)runs.size();
}

static int regimes_main() {
    const int stack = F_LAYER_FEAT_NORM | F_POS_CONV_STACK | (5 << RSAF_W2V2_POS_DEPTH_SHIFT);
    struct Row { const char* name; Cfg c; int max_runs; };
    const Row rows[] = {
        {"hd64-cg16", {32, 128, 1, 2, 128, 16, 8, 1e-5f, 0}, 3},              // tests/test_w2v2_long_windows_gpu.py, main geometry
        {"hd64-cg16-wavlm", {32, 128, 1, 2, 128, 16, 8, 1e-5f, F_REL_POS_BIAS}, 3},
        {"hd64-base", {512, 768, 12, 12, 3072, 128, 16, 1e-5f, 0}, 3},
        {"hd64-large-stable", {512, 1024, 24, 16, 4096, 128, 16, 1e-5f, 7}, 2},   // group width 64: 512 rows and 127 taps exceed the LDS
        {"hd16-cg8", {32, 64, 2, 4, 128, 16, 8, 1e-5f, 0}, 1},                // no regimes: exact-fp32 convolution, three launches
        {"hd16-cg16", {32, 64, 2, 4, 128, 16, 4, 1e-5f, F_REL_POS_BIAS}, 3},   // the positional kernel alone has regimes
        {"hd64-stack", {512, 768, 12, 12, 3072, 19, 16, 1e-5f, stack}, 2},     // the stack picks nothing by T; the attention does
        {"hd16-stack", {32, 64, 2, 4, 128, 19, 4, 1e-5f, stack}, 1}};
    const int F[] = {1025, 514, 513, 512, 511, 499, 258, 257, 256, 255, 249, 120, 2};   // descending
    const int nF = (int)(sizeof(F) / sizeof(F[0]));
    for (const Row& row : rows) {
        g_row = std::string("regimes ") + row.name;
        if (const char* msg = check_cfg(row.c)) fail(std::string("check_cfg: ") + msg);
        int64_t lists = 0, most = 0;
        for (int a = 0; a < nF; ++a)
            for (int b = a; b <= nF; ++b)
                for (int d = (b < nF ? b : nF); d <= nF; ++d)
                    for (int e = (d < nF ? d : nF); e <= nF; ++e) {
                        std::vector<int> frames = {F[a]};
                        for (int i : {b, d, e}) if (i < nF) frames.push_back(F[i]);
                        most = std::max(most, check_regime_runs(row.c, frames));
                        ++lists;
                    }
        expect(most, row.max_runs, "most runs of a list");
        // the list of the GPU test: 1025, 513 | 512, 499, 257 | 256 .. 2 at the main geometry
        if (check_regime_runs(row.c, {1025, 513, 512, 499, 257, 256, 249, 120, 33, 2}) != row.max_runs) fail("runs of the ten-window list");
        // many equal windows and a tail: the feature encoder's group buffers and the score buffer are sized by the call
        std::vector<int> many(600, 499);
        many.insert(many.end(), 40, 249);
        many.push_back(2);
        check_regime_runs(row.c, many);
        std::printf("ok %s (%lld lists)\n", g_row.c_str(), (long long)lists);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "regimes") return regimes_main();
    const std::vector<WinSet> sets = window_sets();
    const int n_geoms = (int)(sizeof(GEOMS) / sizeof(GEOMS[0]));
    for (int gi = 0; gi < n_geoms; ++gi)
        for (size_t wi = 0; wi < sets.size(); ++wi) {
            const Geom& g = GEOMS[gi];
            const Want& want = WANT[gi][wi];
            g_row = std::string(g.name) + " / " + sets[wi].name;
            if (const char* msg = check_cfg(g.c)) fail(std::string("check_cfg: ") + msg);
            check_weights(g);
            Rag R;
            if (const char* msg = make_rag(sets[wi].len.data(), (int)sets[wi].len.size(), 0, R)) fail(std::string("make_rag: ") + msg);
            check_rag(sets[wi].len, R);
            check_workspace(g.c, R, make_ws(g.c, R), want.ws_bytes);
            check_packed_rows(R);
            const int Tt = R.Tmax[6];
            expect(fused_attention(g.c, Tt), want.fused, "fused_attention");
            expect(posconv_on_f16x3(g.c), want.on_f16x3, "posconv_on_f16x3");
            expect(posstack_on_mfma(g.c), want.stack_mfma, "posstack_on_mfma");
            expect(posconv_split(Tt), want.split, "posconv_split");
            expect(posconv_resident(g.c, Tt), want.resident, "posconv_resident");
            check_lds(g.c, Tt, want);
            std::printf("ok %s\n", g_row.c_str());
        }
    // equal windows given by count and length, and the two refusals of make_rag
    Rag E;
    g_row = "make_rag";
    if (make_rag(nullptr, 3, 80000, E) || E.rows != 3 * 249 || E.tgroups.size() != 1) fail("equal windows");
    const int up[2] = {400, 800}, tiny[1] = {399};
    Rag U, S;
    const char* mu = make_rag(up, 2, 0, U);
    const char* ms = make_rag(tiny, 1, 0, S);
    if (!mu || std::string(mu) != "window lengths must be non-increasing") fail("increasing lengths accepted");
    if (!ms || std::string(ms) != "chunk shorter than the receptive field of the feature encoder") fail("short chunk accepted");
    std::printf("ok make_rag\n");
    return 0;
}
