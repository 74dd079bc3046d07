// Layouts of the Wav2Vec2 forward (w2v2*.hip), each stated once for the kernels that carve the memory and the host code that
// sizes it: the packed weights, the workspace, the window geometry of a call, the predicates that pick a path, and the
// dynamic LDS of the three kernels that request it.  Plain C++ (no HIP include): tests/test_w2v2_layout_host.py compiles it
// with g++ and checks sizes, bounds, overlap and alignment at the published geometries (tests/host/w2v2_layout_replay.cpp).
// check_cfg and make_rag return the message of the first condition that fails, or NULL; the entry points turn it into
// rsaf_last_error (w2v2.hip: arg_error).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "rsaf.h"

#if defined(__HIPCC__)
#define WL_HD __host__ __device__ __forceinline__
#else
#define WL_HD inline
#endif

namespace rsaf {
namespace w2v2 {

// flags: the forward variants of the _ex entry points (include/rsaf.h)
constexpr int F_LAYER_FEAT_NORM = RSAF_W2V2_LAYER_FEAT_NORM, F_CONV_BIAS = RSAF_W2V2_CONV_BIAS, F_PRE_LN = RSAF_W2V2_PRE_LN,
              F_NO_INPUT_NORM = RSAF_W2V2_NO_INPUT_NORM, F_NO_FEAT_PROJ_LN = RSAF_W2V2_NO_FEAT_PROJ_LN,
              F_REL_POS_BIAS = RSAF_W2V2_REL_POS_BIAS, F_POS_CONV_STACK = RSAF_W2V2_POS_CONV_STACK,
              F_POS_DEPTH_MASK = RSAF_W2V2_POS_DEPTH_MASK,
              F_ALL = 15 | F_NO_FEAT_PROJ_LN | F_REL_POS_BIAS | F_POS_CONV_STACK | F_POS_DEPTH_MASK;
constexpr int REL_SPAN = RSAF_W2V2_REL_SPAN, REL_TAB = 2 * REL_SPAN - 1;    // the distance table of a head: |k - q| < REL_SPAN

struct Cfg {
    int C, Hd, L, NH, I, PK, PG;
    float eps;
    int flags = 0;
    // POS_CONV_STACK: convolutions of the positional stack (0: the single weight-normed convolution)
    int pos_depth() const { return (flags & F_POS_CONV_STACK) ? (flags & F_POS_DEPTH_MASK) >> RSAF_W2V2_POS_DEPTH_SHIFT : 0; }
};

inline int64_t pad4(int64_t n) { return (n + 3) & ~int64_t(3); }

// taps and strides of the seven feature-encoder convolutions (host code and w2v2_tables_kernel)
constexpr int KERN[7] = {10, 3, 3, 3, 3, 2, 2};
constexpr int STRD[7] = {5, 2, 2, 2, 2, 2, 2};

struct LayerOff {
    int64_t wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
};
struct Layout {
    int64_t conv0, gng, gnb, conv[6], fplg, fplb, fpw, fpb, posw, posb, elng, elnb;
    std::vector<LayerOff> layers;
    int64_t cb = -1, cln = -1;       // appended segments: conv biases [7][C] (CONV_BIAS), conv LayerNorms [7][2][C] (LAYER_FEAT_NORM)
    // REL_POS_BIAS: per layer the gate's two summed weight rows ga / gb [hd], {ba, bb} and gru_rel_pos_const [NH]; the table
    std::vector<int64_t> ga, gb, gbias, gconst;
    int64_t reltab = -1;             // [NH][REL_TAB]
    std::vector<int64_t> stackw, stackb;   // POS_CONV_STACK: kernel and bias of the stack's layers 1..D-1 (layer 0: posw / posb)
    int64_t total;
};

inline Layout make_layout(const Cfg& c) {
    Layout L;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t s = o; o += pad4(n); return s; };
    L.conv0 = take((int64_t)c.C * 10); L.gng = take(c.C); L.gnb = take(c.C);
    for (int i = 0; i < 6; ++i) L.conv[i] = take((int64_t)c.C * KERN[i + 1] * c.C);
    L.fplg = take(c.C); L.fplb = take(c.C); L.fpw = take((int64_t)c.Hd * c.C); L.fpb = take(c.Hd);
    const int cg = c.Hd / c.PG;
    L.posw = take((int64_t)c.PG * cg * c.PK * cg); L.posb = take(c.Hd);
    L.elng = take(c.Hd); L.elnb = take(c.Hd);
    for (int l = 0; l < c.L; ++l) {
        LayerOff lo;
        lo.wqkv = take((int64_t)3 * c.Hd * c.Hd); lo.bqkv = take(3 * c.Hd);
        lo.wo = take((int64_t)c.Hd * c.Hd); lo.bo = take(c.Hd);
        lo.ln1g = take(c.Hd); lo.ln1b = take(c.Hd);
        lo.w1 = take((int64_t)c.I * c.Hd); lo.b1 = take(c.I);
        lo.w2 = take((int64_t)c.Hd * c.I); lo.b2 = take(c.Hd);
        lo.ln2g = take(c.Hd); lo.ln2b = take(c.Hd);
        L.layers.push_back(lo);
    }
    if (c.flags & F_CONV_BIAS) L.cb = take((int64_t)7 * c.C);
    if (c.flags & F_LAYER_FEAT_NORM) L.cln = take((int64_t)14 * c.C);
    if (c.flags & F_REL_POS_BIAS) {
        for (int l = 0; l < c.L; ++l) {
            L.ga.push_back(take(c.Hd / c.NH)); L.gb.push_back(take(c.Hd / c.NH));
            L.gbias.push_back(take(2)); L.gconst.push_back(take(c.NH));
        }
        L.reltab = take((int64_t)c.NH * REL_TAB);
    }
    for (int i = 1; i < c.pos_depth(); ++i) {
        L.stackw.push_back(take((int64_t)c.Hd * c.PK * cg)); L.stackb.push_back(take(c.Hd));
    }
    L.total = o;
    return L;
}

// a condition of check_cfg / make_rag: its message goes back to the caller when it fails
#define W2V2_REQUIRE(cond, msg) do { if (!(cond)) return msg; } while (0)

inline const char* check_cfg(const Cfg& c) {
    W2V2_REQUIRE(c.C >= 32 && c.C <= 1024 && c.C % 32 == 0 && (c.C <= 256 || c.C % 256 == 0),
                 "conv_dim must be a multiple of 32 (<= 256) or of 256 (<= 1024)");
    W2V2_REQUIRE(c.Hd >= 16 && c.Hd <= 1024 && c.Hd % 16 == 0, "hidden_size must be a multiple of 16, <= 1024");
    W2V2_REQUIRE(c.I >= 16 && c.I % 16 == 0, "intermediate_size must be a multiple of 16");
    W2V2_REQUIRE(c.L >= 1 && c.L <= 64, "num_hidden_layers out of range");
    W2V2_REQUIRE(c.NH >= 1 && c.Hd % c.NH == 0 && (c.Hd / c.NH) % 4 == 0, "head_dim must be a multiple of 4");
    W2V2_REQUIRE((c.flags & ~F_ALL) == 0, "unknown RSAF_W2V2_* flag bits");
    W2V2_REQUIRE(c.PG >= 1 && c.Hd % c.PG == 0 && (c.Hd / c.PG) % 4 == 0, "positional conv: channels/group multiple of 4");
    if (c.flags & F_POS_CONV_STACK) {
        W2V2_REQUIRE(c.flags & F_POS_DEPTH_MASK, "RSAF_W2V2_POS_CONV_STACK needs its depth in flags bits 12..15");
        W2V2_REQUIRE(c.PK >= 1 && c.PK <= 64, "positional conv stack: kernel must lie in 1..64");
        W2V2_REQUIRE(!(c.flags & (F_PRE_LN | F_REL_POS_BIAS | F_NO_FEAT_PROJ_LN)),
                     "RSAF_W2V2_POS_CONV_STACK with PRE_LN, REL_POS_BIAS or NO_FEAT_PROJ_LN is not built");
        W2V2_REQUIRE(c.flags & F_LAYER_FEAT_NORM, "RSAF_W2V2_POS_CONV_STACK needs RSAF_W2V2_LAYER_FEAT_NORM");
    } else {
        W2V2_REQUIRE(!(c.flags & F_POS_DEPTH_MASK), "depth bits without RSAF_W2V2_POS_CONV_STACK");
        W2V2_REQUIRE(c.PK >= 2 && c.PK % 2 == 0, "positional conv: even kernel");
    }
    W2V2_REQUIRE(!((c.flags & F_NO_FEAT_PROJ_LN) && (c.flags & F_LAYER_FEAT_NORM)),
                 "RSAF_W2V2_NO_FEAT_PROJ_LN with RSAF_W2V2_LAYER_FEAT_NORM is not built");
    return nullptr;
}

inline void chunk_lengths(int len, int T[7]) {
    int n = len;
    for (int i = 0; i < 7; ++i) {
        n = n >= KERN[i] ? (n - KERN[i]) / STRD[i] + 1 : 0;
        T[i] = n;
    }
}

// The dense GEMMs run on rsaf's fp32-accurate f16x3 kernel (gemm_f16x3.hip): their operands live as two fp16 planes,
// scaled per row (encoder activations, weights) or per window (feature-encoder activations) by a power of two.
// Offsets are in floats; a planes buffer of N elements takes 2 N uint16 = N floats.
struct Workspace {
    int64_t xn, part, ab, P, Q, c6, lnfp, x, xp, y, att, attp, xg, qkv, S, ffnp, wp, total;
    int64_t wp_conv[6], wp_fp, wp_pos;
    std::vector<int64_t> wp_qkv, wp_o, wp_1, wp_2;
    // scales of the weight rows, and per weight matrix two words {max row norm, max |w|} (bit patterns, atomicMax)
    int64_t ws_conv[6], ws_fp, ws_pos, wstat;            // wstat: [6 + 2 + 4 L][2] (+ [L][2] for the ffn1 biases)
    std::vector<int64_t> ws_qkv, ws_o, ws_1, ws_2;
    // scales of the activations: per window of the current conv group (conv_scale[7][G], conv_amax[7][G]), per window of
    // the call (pos_scale, fp_amax, win_norm; wlen: the length table of an equal-window call) and per frame (ln / ffn / qkv scales)
    int64_t conv_scale, conv_amax, pos_scale, fp_amax, wlen, win_norm, s_lnfp, s_x, s_ffn, s_att, s_qkv;
    int64_t cb_max;                                      // CONV_BIAS: max |bias| of conv1..5 (appended after the tables)
    int64_t gate;                                        // REL_POS_BIAS: the bias gates [rows][NH] of the current layer (appended)
    std::vector<int64_t> wp_stack, ws_stack;             // POS_CONV_STACK on the matrix pipe: planes and row scales of layers 1..D-1 (appended)
    int64_t t_Tw, t_row0, t_ztab, t_rowwin;              // window tables (int32 / int64 views of the float workspace)
    int64_t t_coff, t_crow;                              // packed conv row spaces of the current group (see packed_in_rows)
};
constexpr int STAT_SLAB = 512;
constexpr int CONV_GROUP = 512;      // windows per pass of the feature encoder (its ping-pong buffers are the big ones)

// What sizes the workspace and picks the forward's path with it (make_ws and Forward read the same three):
inline int conv_group(int n) { return n < CONV_GROUP ? n : CONV_GROUP; }                  // window slots of a feature-encoder pass
inline bool fused_attention(const Cfg& c, int Tt) { return c.Hd / c.NH == 64 && Tt <= 256; }   // else three launches and the score buffer
inline bool posconv_on_f16x3(const Cfg& c) { return (c.Hd / c.PG) % 16 == 0; }             // else the exact-fp32 GEMM
// the positional stack's MFMA kernel holds a group's channels of a row tile in LDS: group widths of 16, 32, 48 and 64
inline bool posstack_on_mfma(const Cfg& c) { return c.pos_depth() > 0 && (c.Hd / c.PG) % 16 == 0 && c.Hd / c.PG <= 64; }

inline int64_t planes_floats(int64_t n) { return pad4(n); }

// Packed row spaces of the feature encoder (group-norm mode).  Conv i (1..6) of a group of windows is ONE GEMM whose rows
// are the windows' frames back to back: in the OUTPUT row space of layer i window w owns T_i[w] + 1 rows from off_i[w] (the
// extra row is junk: it absorbs the last tap reaching one input row further), and the layer's INPUT row space, the
// channels-last planes of layer i - 1, starts the window at row 2 off_i[w] (T_{i-1} <= 2 T_i + 2, so it fits; GEMM row R
// reads K = k C contiguous elements at lda = 2 C).  Gap rows of the input space are read by junk rows only.
// Rows a buffer needs to hold the input space of layer i for G windows of at most Ti frames: the last junk row reads one
// row past the 2 M_i rows of the space.
inline int64_t packed_in_rows(int G, int Ti) { return 2 * (int64_t)G * (Ti + 1) + 1; }
// the P buffer holds the inputs of conv1 / 3 / 5 (and layer mode's G x T[0] rows), Q those of conv2 / 4 / 6 (layer mode:
// G x T[1] fp32 rows); T_{i-1} <= 2 T_i + 2 makes the packed sizes the larger ones
inline int64_t p_rows(int G, const int* T) { return packed_in_rows(G, T[1]); }
inline int64_t q_rows(int G, const int* T) { return packed_in_rows(G, T[2]); }
// first entry of layer i's row table (i = 1..6): G (T[j] + 1) rows per earlier layer j
inline int64_t packed_tab_base(int G, const int* T, int i) {
    int64_t b = 0;
    for (int j = 1; j < i; ++j) b += (int64_t)G * (T[j] + 1);
    return b;
}

// index of a weight matrix in the wstat table
inline int wstat_conv(int i) { return i; }                              // i = 0..5 (conv1..6)
constexpr int WSTAT_FP = 6, WSTAT_POS = 7, WSTAT_LAYER0 = 8, WSTAT_PER_LAYER = 6;   // layer l: qkv, o, ffn1, ffn2, ffn1 bias, qkv bias

// Window geometry of one call (host side): lengths are NON-INCREASING (the caller sorts), so windows of equal frame count
// are contiguous and a group of CONV_GROUP consecutive windows wastes few tile rows.
struct Rag {
    int n = 0, maxlen = 0, Tmax[7] = {};
    int64_t rows = 0;                                    // frames of all windows (rows of the encoder)
    std::vector<int> len;
    std::vector<int64_t> row0;                           // [n + 1] first encoder row of each window
    std::vector<std::pair<int, int>> tgroups;            // [begin, end) of windows with equal T[6]
    std::vector<int> T6;
};

// len_host NULL: n windows of `len` samples each
inline const char* make_rag(const int* len_host, int n, int len, Rag& R) {
    R.n = n;
    if (len_host) R.len.assign(len_host, len_host + n);
    else R.len.assign((size_t)n, len);
    R.row0.assign(n + 1, 0);
    R.T6.resize(n);
    for (int w = 0; w < n; ++w) {
        W2V2_REQUIRE(w == 0 || R.len[w] <= R.len[w - 1], "window lengths must be non-increasing");
        int T[7];
        chunk_lengths(R.len[w], T);
        W2V2_REQUIRE(T[6] >= 1, "chunk shorter than the receptive field of the feature encoder");
        R.T6[w] = T[6];
        R.row0[w + 1] = R.row0[w] + T[6];
        if (w == 0) { R.maxlen = R.len[0]; for (int i = 0; i < 7; ++i) R.Tmax[i] = T[i]; }
        if (w == 0 || T[6] != R.T6[w - 1]) R.tgroups.emplace_back(w, w + 1);
        else R.tgroups.back().second = w + 1;
    }
    R.rows = R.row0[n];
    return nullptr;
}
#undef W2V2_REQUIRE

inline Workspace make_ws(const Cfg& c, const Rag& R) {
    const int n = R.n;
    const int* T = R.Tmax;
    Workspace w{};
    int64_t o = 0;
    auto take = [&](int64_t k) { int64_t s = o; o += pad4(k); return s; };
    const int Tt = T[6];
    const int64_t rows = R.rows;
    const int G = conv_group(n), slabs = (T[0] + STAT_SLAB - 1) / STAT_SLAB;
    w.xn = take((int64_t)G * R.maxlen);
    w.part = take((int64_t)G * slabs * 3 * c.C);
    w.ab = take((int64_t)G * 2 * c.C);
    w.P = take(planes_floats(p_rows(G, T) * c.C));
    w.Q = take(planes_floats(q_rows(G, T) * c.C));
    w.c6 = take(rows * c.C);
    w.lnfp = take(planes_floats(rows * c.C));
    w.x = take(rows * c.Hd);
    w.xp = take(planes_floats(rows * c.Hd));
    w.y = take(rows * c.Hd);
    w.att = take(rows * c.Hd);
    w.attp = take(planes_floats(rows * c.Hd));
    w.xg = take((int64_t)n * (Tt + c.PK - 1) * c.Hd);                     // fp32 or two fp16 planes (same size)
    w.qkv = take(rows * 3 * c.Hd);
    w.S = take(fused_attention(c, Tt) ? 4 : (int64_t)n * c.NH * Tt * pad4(Tt));   // scores: only the three-launch attention
    w.ffnp = take(planes_floats(rows * c.I));
    // weight planes and row scales (built once per forward call)
    for (int i = 0; i < 6; ++i) {
        w.wp_conv[i] = take(planes_floats((int64_t)c.C * KERN[i + 1] * c.C));
        w.ws_conv[i] = take(c.C);
    }
    w.wp_fp = take(planes_floats((int64_t)c.Hd * c.C)); w.ws_fp = take(c.Hd);
    w.wp_pos = take(planes_floats((int64_t)c.Hd * c.PK * (c.Hd / c.PG))); w.ws_pos = take(c.Hd);
    for (int l = 0; l < c.L; ++l) {
        w.wp_qkv.push_back(take(planes_floats((int64_t)3 * c.Hd * c.Hd))); w.ws_qkv.push_back(take(3 * c.Hd));
        w.wp_o.push_back(take(planes_floats((int64_t)c.Hd * c.Hd))); w.ws_o.push_back(take(c.Hd));
        w.wp_1.push_back(take(planes_floats((int64_t)c.I * c.Hd))); w.ws_1.push_back(take(c.I));
        w.wp_2.push_back(take(planes_floats((int64_t)c.Hd * c.I))); w.ws_2.push_back(take(c.Hd));
    }
    w.wstat = take((int64_t)(WSTAT_LAYER0 + WSTAT_PER_LAYER * c.L) * 2);
    w.conv_scale = take((int64_t)7 * G);
    w.conv_amax = take((int64_t)7 * G);
    w.pos_scale = take(n); w.fp_amax = take(n); w.wlen = take(n); w.win_norm = take(n);
    w.s_lnfp = take(rows); w.s_x = take(rows); w.s_ffn = take(rows); w.s_att = take(rows); w.s_qkv = take(rows);
    // window tables (device): Tw[7][n] frames per layer, row0[n + 1] (int64), ztab[7][n][2] (int64: the GEMM's per-batch
    // {rows, output offset} of conv1..6 and of the positional conv), rowwin[rows] window of every encoder row
    w.t_Tw = take((int64_t)7 * n); w.t_row0 = take(2 * ((int64_t)n + 1)); w.t_ztab = take((int64_t)7 * n * 2 * 2);
    w.t_rowwin = take(rows);
    // packed conv row spaces of a group: off[7][G + 1] (int32) and per layer and row {window slot, destination row} (int32 x 2)
    w.t_coff = take((int64_t)7 * (G + 1)); w.t_crow = take(2 * packed_tab_base(G, T, 7));
    w.cb_max = (c.flags & F_CONV_BIAS) ? take(8) : -1;
    w.gate = (c.flags & F_REL_POS_BIAS) ? take(rows * c.NH) : -1;
    if (posstack_on_mfma(c))
        for (int i = 1; i < c.pos_depth(); ++i) {
            w.wp_stack.push_back(take(planes_floats((int64_t)c.Hd * c.PK * (c.Hd / c.PG)))); w.ws_stack.push_back(take(c.Hd));
        }
    w.total = o;
    return w;
}

// ---- dynamic LDS -----------------------------------------------------------------------------------------------------------
// Each layout is built from the kernel's geometry; its accessors return where an array starts, counted in elements of the
// array's type from the start of the dynamic LDS (fp16 bit patterns unless it says floats), and bytes() is what the launch
// requests.  (Offsets, not pointers, and constants where the geometry is fixed: the kernels add them to their own
// __shared__ array, which keeps the instruction streams they were tuned with.)

// attn_f16x3_kernel: two staged blocks of KB keys x HD halfs x 2 planes (K or V of one head)
struct AttnLds {
    static constexpr int HD = 64, KB = 128;             // head width, keys per staged block
    static constexpr int PLANE = KB * HD, TILE = 2 * PLANE;   // halfs of one plane of a block, of a block
    static constexpr int BLOCK0 = 0, BLOCK1 = TILE;     // where the two blocks start
    static constexpr size_t bytes() { return (size_t)2 * TILE * sizeof(unsigned short); }
};

constexpr int PC_ROWS = 512;                     // posconv_f16x3_kernel: output rows per workgroup with SPLIT = 1 (8 waves x 4 row tiles of 16)
constexpr int PS_ROWS = 256;                     // posstack_conv_kernel: output frames per workgroup (4 waves x 4 row tiles of 16)

// posconv_f16x3_kernel<NT, SPLIT>: the window's image [plane][NT panels][rows_alloc][16], then the weight ring of four
// iterations x SPLIT stages of [unit in pair][plane][16 NT rows][16]; SPLIT = 2: the exchange of the odd steps' sums, four
// row groups of [4][NT][4][64] floats, takes the image's place once the image is dead
struct PosconvLds {
    int nt, split, rows_alloc;                   // rows_alloc: image rows, a multiple of the 32 rows one DMA instruction moves
    static WL_HD PosconvLds make(int cg, int PK, int split) { return PosconvLds{cg / 16, split, (PC_ROWS / split + PK - 1 + 31) & ~31}; }
    // each array as a function of the tile counts, which a kernel instance passes as its template arguments (a member read
    // in their place changed the instruction streams the kernel was tuned with)
    static WL_HD int ring_at(int nt, int a_panel) { return 2 * nt * a_panel; }
    static constexpr int stage_elems(int nt) { return 4 * 16 * nt * 16; }  // [unit in pair][plane][16 NT rows][16]
    static WL_HD int stage_at(int nt, int split, int slot, int kh) { return (slot * split + kh) * stage_elems(nt); }
    static WL_HD int exchange_at(int nt, int row_group) { return row_group * (4 * nt * 4 * 64); }
    WL_HD int a_panel() const { return rows_alloc * 16; }                  // elements per (plane, panel); the image starts the LDS
    WL_HD int ring() const { return ring_at(nt, a_panel()); }
    WL_HD int stage(int slot, int kh) const { return stage_at(nt, split, slot, kh); }      // from ring(); slot 0..3, kh 0..split-1
    WL_HD int exchange(int row_group) const { return exchange_at(nt, row_group); }         // in floats; row_group 0..8/split-1
    WL_HD size_t bytes() const { return ((size_t)ring() + (size_t)4 * split * stage_elems(nt)) * sizeof(unsigned short); }
};
// the row split of a window in posconv_f16x3_kernel, and whether the window's image fits
inline int posconv_split(int Tt) { return Tt <= PC_ROWS / 2 ? 2 : 1; }
inline bool posconv_resident(const Cfg& c, int Tt) {
    const int cg = c.Hd / c.PG, split = posconv_split(Tt);
    return cg <= 64 && Tt <= PC_ROWS && (c.PK * (cg / 16)) % (4 * split) == 0 && PosconvLds::make(cg, c.PK, split).bytes() <= 160 * 1024;
}

// The regime of a window of Tt frames: what the three frame-count predicates pick for it, stated once for Forward (which
// reads it at the call's longest window) and for the ragged entry points (which read it per window).  Two windows of one
// regime run the same kernels in the same summation order whichever call they share; a call whose windows span several
// regimes is run as one sub-call per regime run (regime_runs), so a window's values never depend on its neighbours.
// posconv: 0 where the frame count picks nothing (the positional stack, group widths off the f16x3 path) or the batched
// GEMM, else the row split of posconv_f16x3_kernel.
struct Regime {
    bool fused;
    int posconv;
    bool operator==(const Regime& o) const { return fused == o.fused && posconv == o.posconv; }
    bool operator!=(const Regime& o) const { return !(*this == o); }
};
inline Regime window_regime(const Cfg& c, int Tt) {
    const bool lds = c.pos_depth() == 0 && posconv_on_f16x3(c) && posconv_resident(c, Tt);
    return Regime{fused_attention(c, Tt), lds ? posconv_split(Tt) : 0};
}
// [begin, end) of the maximal runs of consecutive windows of one regime (lengths are non-increasing: a regime's windows are contiguous)
inline std::vector<std::pair<int, int>> regime_runs(const Cfg& c, const Rag& R) {
    std::vector<std::pair<int, int>> runs;
    for (int w = 0; w < R.n; ++w) {
        if (w == 0 || window_regime(c, R.T6[w]) != window_regime(c, R.T6[w - 1])) runs.emplace_back(w, w + 1);
        else runs.back().second = w + 1;
    }
    return runs;
}

// posstack_conv_kernel<NT>: the row tile's image [plane][NT panels][rows_alloc][16], PK - 1 halo rows included
struct PosstackLds {
    int nt, rows_alloc;
    static WL_HD PosstackLds make(int cg, int PK) { return PosstackLds{cg / 16, PS_ROWS + PK - 1}; }
    WL_HD int a_panel() const { return rows_alloc * 16; }                  // elements per (plane, panel)
    WL_HD int panel(int plane, int p) const { return (plane * nt + p) * a_panel(); }
    WL_HD size_t bytes() const { return (size_t)2 * nt * a_panel() * sizeof(unsigned short); }
};

}  // namespace w2v2
}  // namespace rsaf
