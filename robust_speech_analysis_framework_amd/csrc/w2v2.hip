// Wav2Vec2 frame-embedding forward for gfx950 (fp32 end to end).
//
// Replaces, for a batch of equal-length chunks, what the reference runs per chunk at batch 1
// (src/foundation_model_extractor.py:113-116): HF Wav2Vec2FeatureExtractor normalisation
// (feature_extraction_wav2vec2.py:95) + transformers' Wav2Vec2Model.forward in eval mode
// (modeling_wav2vec2.py:254-323 conv stack, :422-434 projection, :326-379 positional conv,
// :575-608 post-LN encoder layers).  Chunking (80 000-sample windows every 64 000, per-chunk
// normalisation, duplicated overlap) stays on the host side exactly as the reference does it.
//
// Every dense contraction runs on the fp32-accurate fp16-split GEMM (gemm_f16x3.hip: operands as two fp16 planes with
// power-of-two scales, three MFMA products per term):
//   conv1..6  : channels-last activations make a k-tap/stride-2 conv a GEMM with lda = 2*C, K = k*C
//   pos-conv  : activations regrouped to [chunk][group][T+K-1 (zero padded)][C/G], one batched GEMM
//               (data2vec-audio, RSAF_W2V2_POS_CONV_STACK: a stack of convolution + LayerNorm + GELU layers, posstack_* below)
//   attention : S = QK^T/sqrt(d) and O = PV as (chunk, head)-batched GEMMs on the packed qkv buffer
// conv0 (Cin = 1) + GroupNorm + GELU is recomputed in two passes (stats, apply) instead of
// materialising the un-normalised 15 999 x 512 activation; LayerNorm / softmax are one wave per row.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "gemm_f32.h"
#include "gemm_f16x3.h"

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

static inline int64_t pad4(int64_t n) { return (n + 3) & ~int64_t(3); }

static const int KERN[7] = {10, 3, 3, 3, 3, 2, 2};
static const int STRD[7] = {5, 2, 2, 2, 2, 2, 2};

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

static Layout make_layout(const Cfg& c) {
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

static int check_cfg(const Cfg& c) {
    RSAF_CHECK_ARG(c.C >= 32 && c.C <= 1024 && c.C % 32 == 0 && (c.C <= 256 || c.C % 256 == 0),
                   "conv_dim must be a multiple of 32 (<= 256) or of 256 (<= 1024)");
    RSAF_CHECK_ARG(c.Hd >= 16 && c.Hd <= 1024 && c.Hd % 16 == 0, "hidden_size must be a multiple of 16, <= 1024");
    RSAF_CHECK_ARG(c.I >= 16 && c.I % 16 == 0, "intermediate_size must be a multiple of 16");
    RSAF_CHECK_ARG(c.L >= 1 && c.L <= 64, "num_hidden_layers out of range");
    RSAF_CHECK_ARG(c.NH >= 1 && c.Hd % c.NH == 0 && (c.Hd / c.NH) % 4 == 0, "head_dim must be a multiple of 4");
    RSAF_CHECK_ARG((c.flags & ~F_ALL) == 0, "unknown RSAF_W2V2_* flag bits");
    RSAF_CHECK_ARG(c.PG >= 1 && c.Hd % c.PG == 0 && (c.Hd / c.PG) % 4 == 0, "positional conv: channels/group multiple of 4");
    if (c.flags & F_POS_CONV_STACK) {
        RSAF_CHECK_ARG(c.flags & F_POS_DEPTH_MASK, "RSAF_W2V2_POS_CONV_STACK needs its depth in flags bits 12..15");
        RSAF_CHECK_ARG(c.PK >= 1 && c.PK <= 64, "positional conv stack: kernel must lie in 1..64");
        RSAF_CHECK_ARG(!(c.flags & (F_PRE_LN | F_REL_POS_BIAS | F_NO_FEAT_PROJ_LN)),
                       "RSAF_W2V2_POS_CONV_STACK with PRE_LN, REL_POS_BIAS or NO_FEAT_PROJ_LN is not built");
        RSAF_CHECK_ARG(c.flags & F_LAYER_FEAT_NORM, "RSAF_W2V2_POS_CONV_STACK needs RSAF_W2V2_LAYER_FEAT_NORM");
    } else {
        RSAF_CHECK_ARG(!(c.flags & F_POS_DEPTH_MASK), "depth bits without RSAF_W2V2_POS_CONV_STACK");
        RSAF_CHECK_ARG(c.PK >= 2 && c.PK % 2 == 0, "positional conv: even kernel");
    }
    RSAF_CHECK_ARG(!((c.flags & F_NO_FEAT_PROJ_LN) && (c.flags & F_LAYER_FEAT_NORM)),
                   "RSAF_W2V2_NO_FEAT_PROJ_LN with RSAF_W2V2_LAYER_FEAT_NORM is not built");
    return RSAF_OK;
}

static void chunk_lengths(int len, int T[7]) {
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
static inline int conv_group(int n) { return n < CONV_GROUP ? n : CONV_GROUP; }                  // window slots of a feature-encoder pass
static inline bool fused_attention(const Cfg& c, int Tt) { return c.Hd / c.NH == 64 && Tt <= 256; }   // else three launches and the score buffer
static inline bool posconv_on_f16x3(const Cfg& c) { return (c.Hd / c.PG) % 16 == 0; }             // else the exact-fp32 GEMM
// the positional stack's MFMA kernel holds a group's channels of a row tile in LDS: group widths of 16, 32, 48 and 64
static inline bool posstack_on_mfma(const Cfg& c) { return c.pos_depth() > 0 && (c.Hd / c.PG) % 16 == 0 && c.Hd / c.PG <= 64; }

static inline int64_t planes_floats(int64_t n) { return pad4(n); }

// Packed row spaces of the feature encoder (group-norm mode).  Conv i (1..6) of a group of windows is ONE GEMM whose rows
// are the windows' frames back to back: in the OUTPUT row space of layer i window w owns T_i[w] + 1 rows from off_i[w] (the
// extra row is junk: it absorbs the last tap reaching one input row further), and the layer's INPUT row space, the
// channels-last planes of layer i - 1, starts the window at row 2 off_i[w] (T_{i-1} <= 2 T_i + 2, so it fits; GEMM row R
// reads K = k C contiguous elements at lda = 2 C).  Gap rows of the input space are read by junk rows only.
// Rows a buffer needs to hold the input space of layer i for G windows of at most Ti frames: the last junk row reads one
// row past the 2 M_i rows of the space.
static inline int64_t packed_in_rows(int G, int Ti) { return 2 * (int64_t)G * (Ti + 1) + 1; }
// the P buffer holds the inputs of conv1 / 3 / 5 (and layer mode's G x T[0] rows), Q those of conv2 / 4 / 6 (layer mode:
// G x T[1] fp32 rows); T_{i-1} <= 2 T_i + 2 makes the packed sizes the larger ones
static inline int64_t p_rows(int G, const int* T) { return packed_in_rows(G, T[1]); }
static inline int64_t q_rows(int G, const int* T) { return packed_in_rows(G, T[2]); }
// first entry of layer i's row table (i = 1..6): G (T[j] + 1) rows per earlier layer j
static inline int64_t packed_tab_base(int G, const int* T, int i) {
    int64_t b = 0;
    for (int j = 1; j < i; ++j) b += (int64_t)G * (T[j] + 1);
    return b;
}

// index of a weight matrix in the wstat table
static inline int wstat_conv(int i) { return i; }                       // i = 0..5 (conv1..6)
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
static int make_rag(const int* len_host, int n, int len, Rag& R) {
    R.n = n;
    if (len_host) R.len.assign(len_host, len_host + n);
    else R.len.assign((size_t)n, len);
    R.row0.assign(n + 1, 0);
    R.T6.resize(n);
    for (int w = 0; w < n; ++w) {
        RSAF_CHECK_ARG(w == 0 || R.len[w] <= R.len[w - 1], "window lengths must be non-increasing");
        int T[7];
        chunk_lengths(R.len[w], T);
        RSAF_CHECK_ARG(T[6] >= 1, "chunk shorter than the receptive field of the feature encoder");
        R.T6[w] = T[6];
        R.row0[w + 1] = R.row0[w] + T[6];
        if (w == 0) { R.maxlen = R.len[0]; for (int i = 0; i < 7; ++i) R.Tmax[i] = T[i]; }
        if (w == 0 || T[6] != R.T6[w - 1]) R.tgroups.emplace_back(w, w + 1);
        else R.tgroups.back().second = w + 1;
    }
    R.rows = R.row0[n];
    return RSAF_OK;
}

static Workspace make_ws(const Cfg& c, const Rag& R) {
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

// Tw[i][w], row0, the packed-output offsets and the row -> window map from the device copy of the lengths
__global__ __launch_bounds__(256) void w2v2_tables_kernel(const int* __restrict__ len, int n, int C, int Hd, int* __restrict__ Tw,
                                                          int64_t* __restrict__ row0, int64_t* __restrict__ ztab) {
    const int KERN_[7] = {10, 3, 3, 3, 3, 2, 2}, STRD_[7] = {5, 2, 2, 2, 2, 2, 2};
    for (int w = threadIdx.x; w < n; w += 256) {
        int m = len[w];
        for (int i = 0; i < 7; ++i) { m = m >= KERN_[i] ? (m - KERN_[i]) / STRD_[i] + 1 : 0; Tw[(int64_t)i * n + w] = m; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t r = 0;
        for (int w = 0; w < n; ++w) { row0[w] = r; r += Tw[(int64_t)6 * n + w]; }
        row0[n] = r;
    }
    __syncthreads();
    // ztab[j][w] = {rows of window w, element offset of its fp32 output or -1}: j = 0..4 conv1..5 (plane outputs at the batch
    // stride), j = 5 conv6 (packed rows of C floats), j = 6 positional conv (packed rows of Hd floats)
    for (int w = threadIdx.x; w < n; w += 256) {
        for (int j = 0; j < 5; ++j) { ztab[((int64_t)j * n + w) * 2] = Tw[(int64_t)(j + 1) * n + w]; ztab[((int64_t)j * n + w) * 2 + 1] = -1; }
        ztab[((int64_t)5 * n + w) * 2] = Tw[(int64_t)6 * n + w]; ztab[((int64_t)5 * n + w) * 2 + 1] = row0[w] * C;
        ztab[((int64_t)6 * n + w) * 2] = Tw[(int64_t)6 * n + w]; ztab[((int64_t)6 * n + w) * 2 + 1] = row0[w] * Hd;
    }
}
// Packed conv row spaces of the windows of one group (Tw, row0: already at the group's first window): off[i][w] = first row
// of window w in the output row space of conv i, off[i][g] = M_i, the rows of that layer's GEMM
__global__ __launch_bounds__(64) void w2v2_pack_offsets_kernel(const int* __restrict__ Tw, int n, int g, int G, int* __restrict__ off) {
    const int i = threadIdx.x + 1;
    if (i > 6) return;
    int r = 0;
    for (int w = 0; w < g; ++w) { off[(int64_t)i * (G + 1) + w] = r; r += Tw[(int64_t)i * n + w] + 1; }
    off[(int64_t)i * (G + 1) + g] = r;
}
// the row table of conv i = blockIdx.y + 1, window blockIdx.x: {slot, destination} of its T_i + 1 rows.  Frame t goes to
// row 2 off_{i+1}[w] + t of the next layer's input space (conv6: to the call's packed row row0[w] + t); the junk row to -1
struct PackBases { int64_t b[7]; };
__global__ __launch_bounds__(256) void w2v2_pack_rows_kernel(const int* __restrict__ Tw, int n, int G, const int* __restrict__ off,
                                                             const int64_t* __restrict__ row0, int* __restrict__ tab, PackBases bases) {
    const int w = blockIdx.x, i = blockIdx.y + 1;
    const int Ti = Tw[(int64_t)i * n + w];
    const int dst0 = i < 6 ? 2 * off[(int64_t)(i + 1) * (G + 1) + w] : (int)row0[w];
    int2* t2 = reinterpret_cast<int2*>(tab) + bases.b[i] + off[(int64_t)i * (G + 1) + w];
    for (int t = threadIdx.x; t <= Ti; t += 256) t2[t] = make_int2(w, t < Ti ? dst0 + t : -1);
}
__global__ __launch_bounds__(256) void w2v2_rowwin_kernel(const int64_t* __restrict__ row0, int* __restrict__ rowwin) {
    const int w = blockIdx.x;
    const int64_t a = row0[w], b = row0[w + 1];
    for (int64_t r = a + threadIdx.x; r < b; r += 256) rowwin[r] = w;
}
__global__ __launch_bounds__(256) void fill_i32_kernel(int* __restrict__ p, int n, int v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- per-chunk zero-mean / unit-variance normalisation -------------------------------------------
// NORM = false (RSAF_W2V2_NO_INPUT_NORM, HF do_normalize=False): the window's samples go to conv0 as they are
template <bool NORM>
__global__ __launch_bounds__(256) void normalize_kernel(const float* __restrict__ wav,
                                                        const int64_t* __restrict__ starts, const int* __restrict__ wlen,
                                                        int maxlen, float* __restrict__ xn) {
    __shared__ double red[4];
    __shared__ double bc;
    const float* x = wav + starts[blockIdx.x];
    const int len = wlen[blockIdx.x];                        // every window is normalised over its own samples
    float* o = xn + (int64_t)blockIdx.x * maxlen;
    if (!NORM) {
        for (int i = threadIdx.x; i < len; i += 256) o[i] = x[i];
        return;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double s = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) s += (double)x[i];
    s = wave_sum_f64(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) bc = (red[0] + red[1] + red[2] + red[3]) / len;
    __syncthreads();
    const double mean = bc;
    double v = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) { const double d = (double)x[i] - mean; v += d * d; }
    v = wave_sum_f64(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    const float var = (float)((red[0] + red[1] + red[2] + red[3]) / len);
    const float mu = (float)mean;
    const float sd = sqrtf(var + 1e-7f);
    for (int i = threadIdx.x; i < len; i += 256) o[i] = (x[i] - mu) / sd;
}

// ---- conv0 (1 -> C, k = 10, s = 5) + GroupNorm(C groups) + GELU, two passes ----------------------
__device__ __forceinline__ unsigned short f16_bits_w(_Float16 h) { return __builtin_bit_cast(unsigned short, h); }
// xs = hi + lo (+ 2^-22 |xs|): the two fp16 planes of a value that already carries its power-of-two scale (gemm_f16x3.hip)
__device__ __forceinline__ void split2_w(float xs, unsigned short& h, unsigned short& l) {
    const _Float16 hh = (_Float16)xs;
    h = f16_bits_w(hh);
    l = f16_bits_w((_Float16)(xs - (float)hh));
}

// thread <-> channel(s); the 10 samples of a frame are wave-uniform (scalar loads).  Statistics pass: per slab and channel
// the sum, the sum of squares and the largest |y| (the bound behind the window's plane scale).  Apply pass: the output
// goes out as the two fp16 planes of GELU(a y + b) * scale[window] (A operand of conv1).
// BIAS (RSAF_W2V2_CONV_BIAS): the conv bias joins y before the statistics, as in the checkpoint's Conv1d
template <int CPT, bool APPLY, bool BIAS>
__global__ __launch_bounds__(256) void conv0_kernel(const float* __restrict__ xn, const float* __restrict__ w0,
                                                    const float* __restrict__ cb, float* __restrict__ part, const float* __restrict__ ab,
                                                    const float* __restrict__ scale,
                                                    unsigned short* __restrict__ outp, int64_t plane, int len,
                                                    const int* __restrict__ T0w, const int* __restrict__ out_off, int C, int slab,
                                                    int slabs) {
    // len: the longest window's samples (stride of xn); T0w: frames of every window; out_off[w]: HALF the first output row of
    // window w (its first row in conv1's packed output row space)
    const int chunk = blockIdx.y, sl = blockIdx.x;
    const int t0 = sl * slab, t1 = min(T0w[chunk], t0 + slab);
    const float* __restrict__ x = xn + (int64_t)chunk * len;
    float wr[CPT][10], a[CPT], b[CPT], s[CPT], q[CPT], mx[CPT], bi[CPT];
    int ch[CPT];
    const float sc = APPLY ? scale[chunk] : 1.0f;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        ch[k] = CPT * threadIdx.x + k;                      // adjacent channels: the planes go out as packed pairs
#pragma unroll
        for (int j = 0; j < 10; ++j) wr[k][j] = w0[ch[k] * 10 + j];
        bi[k] = BIAS ? cb[ch[k]] : 0.f;
        s[k] = 0.f; q[k] = 0.f; mx[k] = 0.f;
        if (APPLY) { a[k] = ab[((int64_t)chunk * 2 + 0) * C + ch[k]]; b[k] = ab[((int64_t)chunk * 2 + 1) * C + ch[k]]; }
    }
    for (int t = t0; t < t1; ++t) {
        float xv[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) xv[j] = x[5 * t + j];
        unsigned short hh[CPT], ll[CPT];
        float gv[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            float y = 0.f;
#pragma unroll
            for (int j = 0; j < 10; ++j) y = fmaf(wr[k][j], xv[j], y);
            if (BIAS) y += bi[k];
            if (APPLY) {
                gv[k] = fmaf(y, a[k], b[k]);
            } else {
                s[k] += y; q[k] += y * y; mx[k] = fmaxf(mx[k], fabsf(y));
            }
        }
        if (APPLY) {                                        // GELU two channels per packed instruction (gemm_f16x3.h)
#pragma unroll
            for (int k = 0; k < CPT; k += 2) {
                if (k + 1 < CPT) {
                    const gelu_f32x2 g2 = gelu_pair(gelu_f32x2{gv[k], gv[k + 1]});
                    split2_w(g2.x * sc, hh[k], ll[k]);
                    split2_w(g2.y * sc, hh[k + 1], ll[k + 1]);
                } else {
                    const gelu_f32x2 g2 = gelu_pair(gelu_f32x2{gv[k], gv[k]});
                    split2_w(g2.x * sc, hh[k], ll[k]);
                }
            }
        }
        if (APPLY) {
            const int64_t o = (2 * (int64_t)out_off[chunk] + t) * C + ch[0];
            if (CPT % 2 == 0) {                             // 4-byte stores of channel pairs (C and ch[0] are even)
#pragma unroll
                for (int k = 0; k < CPT; k += 2) {
                    *reinterpret_cast<unsigned*>(outp + o + k) = hh[k] | ((unsigned)hh[k + 1] << 16);
                    *reinterpret_cast<unsigned*>(outp + plane + o + k) = ll[k] | ((unsigned)ll[k + 1] << 16);
                }
            } else {
#pragma unroll
                for (int k = 0; k < CPT; ++k) { outp[o + k] = hh[k]; outp[plane + o + k] = ll[k]; }
            }
        }
    }
    if (!APPLY) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            part[(((int64_t)chunk * slabs + sl) * 3 + 0) * C + ch[k]] = s[k];
            part[(((int64_t)chunk * slabs + sl) * 3 + 1) * C + ch[k]] = q[k];
            part[(((int64_t)chunk * slabs + sl) * 3 + 2) * C + ch[k]] = mx[k];
        }
    }
}

// ---- layer-norm feature encoder (RSAF_W2V2_LAYER_FEAT_NORM): conv -> LayerNorm over the C channels of a frame -> GELU --------
// The conv GEMMs read their A operand through a strided, overlapping row view (lda = stride C), so the planes of a conv layer's
// output carry one power of two per window.  A bound that needs no pass over the data: a normalised element is at most
// sqrt(C - 1) in magnitude, so |GELU(g n + b)| <= max(max|g| sqrt(C) + max|b|, 0.17) (GELU >= -0.17).  It depends on the
// weights only: one scale per layer, the same for every window (about 23x loose at C = 512, which the three-product
// arithmetic absorbs: tests/test_gemm_gpu.py runs scales 4 096x too loose at fp32 accuracy).
// Wave i < 6 writes layer i's scale into scale[i * G + w] for every window slot w of a group.
__global__ __launch_bounds__(384) void lnconv_scale_kernel(const float* __restrict__ cln, int C, int G, float* __restrict__ scale) {
    const int i = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* g = cln + (int64_t)2 * i * C;
    const float* b = g + C;
    float mg = 0.f, mb = 0.f;
    for (int c = lane; c < C; c += 64) { mg = fmaxf(mg, fabsf(g[c])); mb = fmaxf(mb, fabsf(b[c])); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { mg = fmaxf(mg, __shfl_xor(mg, o, 64)); mb = fmaxf(mb, __shfl_xor(mb, o, 64)); }
    const float bound = fmaxf(mg * sqrtf((float)C) * 1.0001f + mb, 0.17f) * 1.0001f;
    const float sc = f16x2_scale_for_bound(bound);
    for (int w = lane; w < G; w += 64) scale[(int64_t)i * G + w] = sc;
}

// max |bias| of conv1..5 (RSAF_W2V2_CONV_BIAS, group mode): the additive term of the bound behind each layer's plane scale
__global__ __launch_bounds__(64) void conv_bias_max_kernel(const float* __restrict__ cb, int C, float* __restrict__ out) {
    for (int i = 1; i < 6; ++i) {
        float m = 0.f;
        for (int c = threadIdx.x; c < C; c += 64) m = fmaxf(m, fabsf(cb[(int64_t)i * C + c]));
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (threadIdx.x == 0) out[i] = m * 1.000001f;
    }
}

// the LayerNorm (eps 1e-5: nn.LayerNorm's default, not layer_norm_eps) of C values spread as CPT per lane over one wave
template <int CPT>
__device__ __forceinline__ void conv_ln_gelu_lanes(float (&y)[CPT], const bool (&ok)[CPT], const float (&g)[CPT],
                                                   const float (&b)[CPT], int C) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CPT; ++k) s += ok[k] ? y[k] : 0.f;
    const float mean = wave_sum(s) / C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < CPT; ++k) { const float d = y[k] - mean; q += ok[k] ? d * d : 0.f; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / C + 1e-5f);
#pragma unroll
    for (int k = 0; k < CPT; ++k) y[k] = (y[k] - mean) * rstd * g[k] + b[k];
#pragma unroll
    for (int k = 0; k < CPT; k += 2) {
        const gelu_f32x2 g2 = gelu_pair(gelu_f32x2{y[k], y[k + 1 < CPT ? k + 1 : k]});
        y[k] = g2.x;
        if (k + 1 < CPT) y[k + 1] = g2.y;
    }
}

// conv0 (1 -> C, k 10, s 5, optional bias) + LayerNorm over the channels + GELU in one pass: one wave per frame, lane l holds
// channels CPT l .. CPT l + CPT - 1; the output goes out as the two fp16 planes of conv1's A under the window's scale
template <int CPT>
__global__ __launch_bounds__(256) void conv0_ln_kernel(const float* __restrict__ xn, const float* __restrict__ w0,
                                                       const float* __restrict__ cb, const float* __restrict__ lg,
                                                       const float* __restrict__ lb, const float* __restrict__ scale,
                                                       unsigned short* __restrict__ outp, int64_t plane, int len,
                                                       const int* __restrict__ T0w, int T0, int C, int frames) {
    const int chunk = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int t0 = blockIdx.x * frames, t1 = min(T0w[chunk], t0 + frames);
    const float* __restrict__ x = xn + (int64_t)chunk * len;
    float wr[CPT][10], bi[CPT], g[CPT], b[CPT];
    bool ok[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int c = CPT * lane + k;
        ok[k] = c < C;
        const int cc = ok[k] ? c : 0;
#pragma unroll
        for (int j = 0; j < 10; ++j) wr[k][j] = w0[cc * 10 + j];
        bi[k] = cb ? cb[cc] : 0.f;
        g[k] = lg[cc];
        b[k] = lb[cc];
    }
    const float sc = scale[chunk];
    for (int t = t0 + wv; t < t1; t += 4) {
        float xv[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) xv[j] = x[5 * t + j];
        float y[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < 10; ++j) v = fmaf(wr[k][j], xv[j], v);
            y[k] = v + bi[k];
        }
        conv_ln_gelu_lanes<CPT>(y, ok, g, b, C);
        unsigned short hh[CPT], ll[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) split2_w(y[k] * sc, hh[k], ll[k]);
        const int64_t o = ((int64_t)chunk * T0 + t) * C + CPT * lane;
        if (CPT % 2 == 0) {                                 // 4-byte stores of channel pairs (ok[k] implies ok[k + 1]: C even)
#pragma unroll
            for (int k = 0; k < CPT; k += 2)
                if (ok[k]) {
                    *reinterpret_cast<unsigned*>(outp + o + k) = hh[k] | ((unsigned)hh[k + 1 < CPT ? k + 1 : k] << 16);
                    *reinterpret_cast<unsigned*>(outp + plane + o + k) = ll[k] | ((unsigned)ll[k + 1 < CPT ? k + 1 : k] << 16);
                }
        } else {
#pragma unroll
            for (int k = 0; k < CPT; ++k)
                if (ok[k]) { outp[o + k] = hh[k]; outp[plane + o + k] = ll[k]; }
        }
    }
}

// conv1..5 in layer mode: the GEMM wrote fp32 rows (window w's frame t at row w Ti + t); LayerNorm -> GELU -> the planes of the
// next conv's A under the window's scale.  One wave per row (C <= 1024); rows past a window's own frame count are skipped.
__global__ __launch_bounds__(256) void conv_ln_gelu_kernel(const float* __restrict__ src, const float* __restrict__ lg,
                                                           const float* __restrict__ lb, const float* __restrict__ scale,
                                                           unsigned short* __restrict__ outp, int64_t plane, int64_t rows,
                                                           int Ti, const int* __restrict__ Tiw, int C) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int w = (int)(row / Ti);
    if (row - (int64_t)w * Ti >= Tiw[w]) return;
    const int lane = threadIdx.x & 63, C4 = C >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src + row * C);
    const float4* g4 = reinterpret_cast<const float4*>(lg);
    const float4* b4 = reinterpret_cast<const float4*>(lb);
    float y[16], g[16], b[16];
    bool ok[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = lane + 64 * i;
        const bool v = idx < C4;
        const float4 a = v ? s4[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 gg = v ? g4[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 bb = v ? b4[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
        y[4 * i] = a.x; y[4 * i + 1] = a.y; y[4 * i + 2] = a.z; y[4 * i + 3] = a.w;
        g[4 * i] = gg.x; g[4 * i + 1] = gg.y; g[4 * i + 2] = gg.z; g[4 * i + 3] = gg.w;
        b[4 * i] = bb.x; b[4 * i + 1] = bb.y; b[4 * i + 2] = bb.z; b[4 * i + 3] = bb.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) ok[4 * i + k] = v;
    }
    conv_ln_gelu_lanes<16>(y, ok, g, b, C);
    const float sc = scale[w];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = lane + 64 * i;
        if (idx < C4) {
            unsigned short hh[4], ll[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) split2_w(y[4 * i + k] * sc, hh[k], ll[k]);
            unsigned short* pp = outp + row * C + 4 * idx;
            *reinterpret_cast<uint2*>(pp) = make_uint2(hh[0] | ((unsigned)hh[1] << 16), hh[2] | ((unsigned)hh[3] << 16));
            *reinterpret_cast<uint2*>(pp + plane) = make_uint2(ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16));
        }
    }
}

// GroupNorm coefficients per (window, channel) and the window's bound: |GELU(a y + b)| <= |a| max|y| + |b|
__global__ __launch_bounds__(256) void gn_finalize_kernel(const float* __restrict__ part, const float* __restrict__ g,
                                                          const float* __restrict__ be, float* __restrict__ ab,
                                                          unsigned* __restrict__ amax, int n, int C, int slabs,
                                                          const int* __restrict__ T0w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * C) return;
    const int chunk = (int)(i / C), c = (int)(i % C);
    const int T0 = T0w[chunk];
    double s = 0.0, q = 0.0;
    float mx = 0.f;
    for (int sl = 0; sl < slabs; ++sl) {
        s += (double)part[(((int64_t)chunk * slabs + sl) * 3 + 0) * C + c];
        q += (double)part[(((int64_t)chunk * slabs + sl) * 3 + 1) * C + c];
        mx = fmaxf(mx, part[(((int64_t)chunk * slabs + sl) * 3 + 2) * C + c]);
    }
    const double mean = s / T0;
    double var = q / T0 - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + 1e-5);
    const double a = (double)g[c] * rstd;
    const float af = (float)a, bf = (float)((double)be[c] - mean * a);
    ab[((int64_t)chunk * 2 + 0) * C + c] = af;
    ab[((int64_t)chunk * 2 + 1) * C + c] = bf;
    atomicMax(amax + chunk, __float_as_uint((fabsf(af) * mx + fabsf(bf)) * 1.000001f));
}

// ---- LayerNorm over the last dim (optionally of x + r), one wave per row, D <= 1024 -----------------
// Optional outputs for the GEMM that reads the result: the row as two fp16 planes times the power of two that puts the
// row's largest magnitude into [2^14, 2^15) (scale_out[row]: exact, the wave holds the whole row), and the scale the NEXT
// GEMM's plane output may use for this row (bound_scale_out): |GELU(y W^T + b)| <= |y|_2 max_n |w_n|_2 + max |b|.
// VAR 1 (stable-layer-norm encoder): the un-normalised sum x + r also goes to aux (the fp32 residual stream).
// VAR 2 (conv6 of the layer-norm feature encoder): the row first takes its conv LayerNorm (pg, pb, eps 1e-5) and GELU.
// VAR 3 (NO_FEAT_PROJ_LN): identity, y = x (+ r); g, b and eps are not read.  The row only changes its form: planes and scales.
// TAP (hidden-state extraction): the row also goes to `tap`, at row tap_row_start[w] + t (or row `row` when that table is
// NULL): TAP 1 the normalised output y, TAP 2 the un-normalised input v = x (+ r).  TAP 0 never reads the two trailing
// arguments, so the untapped instances keep their code.
template <int VAR, int TAP = 0>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ r,
                                                        const float* __restrict__ g, const float* __restrict__ b,
                                                        float* __restrict__ out, int64_t rows, int D, float eps,
                                                        const int64_t* __restrict__ out_row_start, const int* __restrict__ rowwin,
                                                        const int64_t* __restrict__ row0,
                                                        unsigned short* __restrict__ planes, int64_t plane, int panel,
                                                        float* __restrict__ scale_out, const unsigned* __restrict__ bound_w,
                                                        const unsigned* __restrict__ bound_b, float* __restrict__ bound_scale_out,
                                                        unsigned* __restrict__ win_norm, const float* __restrict__ pg,
                                                        const float* __restrict__ pb, float* __restrict__ aux,
                                                        float* __restrict__ tap, const int64_t* __restrict__ tap_row_start) {
    // panel != 0: the planes go out in the k16-panel layout of `rows` rows (gemm_f16x3.h), staged through LDS so that the
    // four rows of the workgroup leave as full 128-byte lines per panel (scattering 8-byte pieces from the row layout cost
    // this kernel + 77 %)
    __shared__ __attribute__((aligned(16))) unsigned short stg[2][4][1024];
    const int64_t row_raw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool valid = row_raw < rows;
    if (!valid && !(planes && panel)) return;
    const int64_t row = valid ? row_raw : rows - 1;
    const int lane = threadIdx.x & 63;
    // optional scatter: frame t of window w lands at output row out_row_start[w] + t (vstack order)
    int64_t orow = row;
    if (out_row_start) { const int w = rowwin[row]; orow = out_row_start[w] + (row - row0[w]); }
    const int D4 = D >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + row * D);
    const float4* r4 = r ? reinterpret_cast<const float4*>(r + row * D) : nullptr;
    float4* t4 = nullptr;
    if constexpr (TAP != 0) {
        int64_t trow = row;
        if (tap_row_start) { const int w = rowwin[row]; trow = tap_row_start[w] + (row - row0[w]); }
        t4 = reinterpret_cast<float4*>(tap + trow * D);
    }
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = lane + 64 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < D4) {
            v[i] = x4[idx];
            if (r4) { const float4 t = r4[idx]; v[i].x += t.x; v[i].y += t.y; v[i].z += t.z; v[i].w += t.w; }
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
            if (VAR == 1 && valid) reinterpret_cast<float4*>(aux + row * D)[idx] = v[i];
            if (TAP == 2 && valid) t4[idx] = v[i];
        }
    }
    if constexpr (VAR == 2) {
        const float m0 = wave_sum(s) / D;
        float q0 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = lane + 64 * i;
            if (idx < D4) {
                const float a = v[i].x - m0, bb = v[i].y - m0, c = v[i].z - m0, d = v[i].w - m0;
                q0 += (a * a + bb * bb) + (c * c + d * d);
            }
        }
        const float r0 = 1.0f / sqrtf(wave_sum(q0) / D + 1e-5f);
        s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = lane + 64 * i;
            if (idx < D4) {
                const float4 gg = reinterpret_cast<const float4*>(pg)[idx], bb = reinterpret_cast<const float4*>(pb)[idx];
                const gelu_f32x2 e0 = gelu_pair(gelu_f32x2{(v[i].x - m0) * r0 * gg.x + bb.x, (v[i].y - m0) * r0 * gg.y + bb.y});
                const gelu_f32x2 e1 = gelu_pair(gelu_f32x2{(v[i].z - m0) * r0 * gg.z + bb.z, (v[i].w - m0) * r0 * gg.w + bb.w});
                v[i] = make_float4(e0.x, e0.y, e1.x, e1.y);
                s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
            }
        }
    }
    float mean = 0.f, rstd = 1.f;
    if constexpr (VAR != 3) {
        mean = wave_sum(s) / D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = lane + 64 * i;
            if (idx < D4) {
                const float a = v[i].x - mean, bb = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
                q += (a * a + bb * bb) + (c * c + d * d);
            }
        }
        rstd = 1.0f / sqrtf(wave_sum(q) / D + eps);
    }
    float4* o4 = out ? reinterpret_cast<float4*>(out + orow * D) : nullptr;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    float mx = 0.f, n2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = lane + 64 * i;
        if (idx < D4) {
            float4 y = v[i];
            if constexpr (VAR != 3) {
                const float4 gg = g4[idx], bb = b4[idx];
                y = make_float4((v[i].x - mean) * rstd * gg.x + bb.x, (v[i].y - mean) * rstd * gg.y + bb.y,
                                (v[i].z - mean) * rstd * gg.z + bb.z, (v[i].w - mean) * rstd * gg.w + bb.w);
            }
            if (o4 && valid) o4[idx] = y;
            if (TAP == 1 && valid) t4[idx] = y;
            v[i] = y;
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(y.x), fabsf(y.y)), fmaxf(fabsf(y.z), fabsf(y.w))));
            n2 += (y.x * y.x + y.y * y.y) + (y.z * y.z + y.w * y.w);
        }
    }
    if (!planes) return;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float sc = f16x2_scale_for_bound(mx);
    if (valid && lane == 0) scale_out[row] = sc;
    if (bound_scale_out || win_norm) {
        const float nrm = sqrtf(wave_sum(n2)) * 1.000001f;
        if (bound_scale_out) {
            const float bound = nrm * __uint_as_float(bound_w[0]) * 1.000001f + (bound_b ? __uint_as_float(bound_b[1]) : 0.0f);
            if (valid && lane == 0) bound_scale_out[row] = f16x2_scale_for_bound(bound);
        }
        // the largest row norm of the window (behind the per-window scale of the next q / k / v projection's plane output)
        if (win_norm && valid && lane == 0) atomicMax(win_norm + rowwin[row], __float_as_uint(nrm));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = lane + 64 * i;
        if (idx < D4) {                                    // the same values as two fp16 planes (A operand of the next GEMM)
            const float yy[4] = {v[i].x * sc, v[i].y * sc, v[i].z * sc, v[i].w * sc};
            unsigned short hh[4], ll[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) split2_w(yy[k], hh[k], ll[k]);
            const uint2 ph = make_uint2(hh[0] | ((unsigned)hh[1] << 16), hh[2] | ((unsigned)hh[3] << 16));
            const uint2 pl = make_uint2(ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16));
            if (panel) {
                const int wq = threadIdx.x >> 6;
                *reinterpret_cast<uint2*>(&stg[0][wq][4 * idx]) = ph;
                *reinterpret_cast<uint2*>(&stg[1][wq][4 * idx]) = pl;
            } else if (valid) {
                unsigned short* pp = planes + row * D + 4 * idx;
                *reinterpret_cast<uint2*>(pp) = ph;
                *reinterpret_cast<uint2*>(pp + plane) = pl;
            }
        }
    }
    if (panel) {
        __syncthreads();
        const int64_t row0 = (int64_t)blockIdx.x * 4;
        const int chunks = D >> 1;                          // 16-byte pieces per plane: D / 16 panels x 4 rows x 2 halves
        for (int c = threadIdx.x; c < chunks; c += 256) {
            const int pn = c >> 3, rr = (c & 7) >> 1, hf = c & 1;
            if (row0 + rr < rows) {
#pragma unroll
                for (int p2 = 0; p2 < 2; ++p2)
                    *reinterpret_cast<uint4*>(planes + p2 * plane + (int64_t)pn * (rows * 16) + (row0 + rr) * 16 + 8 * hf) =
                        *reinterpret_cast<const uint4*>(&stg[p2][rr][16 * pn + 8 * hf]);
            }
        }
    }
}

using af32x16 = __attribute__((ext_vector_type(16))) float;

typedef __attribute__((address_space(3))) void* attn_lds_ptr;
typedef const __attribute__((address_space(1))) void* attn_glb_ptr;

// ---- fused attention on the fp16 matrix pipe (two-way fp16 splits, three products: gemm_f16x3.hip's arithmetic) --------
// For windows of at most 256 frames (every Wav2Vec2 window: T <= 249).  One workgroup = 128 queries of one (window, head);
// wave = 32 queries.  S^T = K Q^T: keys are the MFMA rows, queries the columns, so a lane holds ONE query's scores for 16 keys
// per tile: the softmax over keys is in-lane plus one exchange with lane ^ 32, and no score or probability ever goes to memory;
// all 256 scores of a query stay in registers, so the softmax is the plain two-pass form, not an online rescaling.  K and V are
// staged in blocks of 128 keys by LDS-DMA (two 32 KB buffers, the next block in flight during the multiply).
// (Rounds 1-3 ran this on the fp32 matrix pipe, v_mfma_f32_32x32x2_f32: 78 TFLOP/s; now 161.)  Every product runs on
// v_mfma_f32_32x32x16_f16:
//   * q, k, v arrive as the fp16 plane pair the q/k/v projection's epilogue wrote, scaled by ONE power of two per window
//     (s_w: the bound |x|_2 max|w_n|_2 + max|b| over the window's rows), so S = acc / s_w^2 and the value scale factors out
//     of the sum over keys; no conversion work in this kernel except for the probabilities;
//   * K blocks of 128 keys x 64 halfs x 2 planes (32 KB) by LDS-DMA, 16-byte chunks XOR-swizzled on the source address
//     (chunk ^ ((row >> 1) & 7): the ds_read_b128 fragment reads of 16 consecutive rows cover all 64 banks);
//   * the score tile's register layout is the A operand of P V (element j of lane half h = key 16 s + 8 (j >> 2) + 4 h + (j & 3)),
//     P = p * 2^14 split into hi + lo; the V fragment (B operand, the same key order) comes out of row-major V by two
//     ds_read_b64_tr_b16 (4 keys x 16 columns per 16-lane group, delivered column-major), V chunks swizzled by
//     ((row >> 1) & 1) << 2 so that the four rows of a transposed read sit on disjoint banks;
//   * O = acc 2^-14 is already in the window's scale: it leaves as the plane pair of the out-projection's A operand.
// Matrix cycles: 192 MFMAs of 32 cycles per wave against 512 of 64 on the fp32 pipe.
// RELPOS (WavLM, REL_POS_BIAS): score(q, key) += gate[q][head] * tab[head][key - q].  The head's table over |key - q| <= 255
// (511 floats of reltab, 2 KB of static LDS beside the 64 KB of K / V blocks: still two workgroups per CU) is staged once per
// workgroup; a lane loads its query's gate once and reads tab at (255 - q) + key: the keys of a lane are compile-time
// offsets, and the 32 queries of a half-wave read 32 consecutive words (no bank conflict).  The plain instance reads neither
// of the two trailing arguments and keeps its code.
using ah8 = __attribute__((ext_vector_type(8))) _Float16;
typedef short atr4 __attribute__((__vector_size__(4 * sizeof(short))));

template <bool RELPOS>
__global__ __launch_bounds__(256, 2) void attn_f16x3_kernel(const unsigned short* __restrict__ qkvp, int64_t in_plane,
                                                            unsigned short* __restrict__ planes, int64_t plane_stride,
                                                            int64_t n_rows, const int* __restrict__ Tw,
                                                            const int64_t* __restrict__ row0, int NH, int Hd, float scale,
                                                            const float* __restrict__ row_scale,
                                                            const float* __restrict__ gate, const float* __restrict__ reltab) {
    constexpr int HD = 64, KB = 128, PLANE = KB * HD, TILE = 2 * PLANE;          // one staged block: 2 planes x 16 KB (halfs)
    extern __shared__ __attribute__((aligned(1024))) unsigned short kvh[];      // two blocks
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int win = blockIdx.x / NH, head = blockIdx.x - win * NH;
    const int T = Tw[win];
    if (blockIdx.y * 128 >= T) return;                                          // (workgroup-uniform)
    const int64_t wrow0 = row0[win];
    const int64_t ld = 3 * (int64_t)Hd;                                         // halfs per row of a plane
    const unsigned short* base = qkvp + wrow0 * ld + (int64_t)head * HD;       // q of this window and head, plane 0
    const int q0 = blockIdx.y * 128 + wv * 32;
    const int nblk = (T + KB - 1) / KB;                                         // 1 or 2 key blocks
    const float sw = row_scale[wrow0];                                          // the window's power of two
    const float sinv = pow2_inverse(sw);
    float qgate = 0.0f;                                                         // RELPOS: this lane's query
    const float* qtab = nullptr;                                                //         tab[key - q] = qtab[key]
    if constexpr (RELPOS) {
        __shared__ float tabs[512];
        for (int i = tid; i < 511; i += 256) tabs[i] = reltab[(int64_t)head * REL_TAB + (REL_SPAN - 256) + i];   // d = i - 255
        const int q = blockIdx.y * 128 + wv * 32 + l31;                         // <= 255 (published by the first drain())
        qgate = gate[(wrow0 + (q < T ? q : T - 1)) * NH + head];
        qtab = tabs + (255 - q);
    }

    // Q fragments (B operand of S^T = K Q^T): lane (query l31, half h) holds d = 16 s + 8 h + j, both planes
    ah8 qh[4], ql[4];
    {
        const int q = q0 + l31 < T ? q0 + l31 : T - 1;
        const unsigned short* qp = base + (int64_t)q * ld + 8 * h;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            qh[s4] = *reinterpret_cast<const ah8*>(qp + 16 * s4);
            ql[s4] = *reinterpret_cast<const ah8*>(qp + in_plane + 16 * s4);
        }
    }
    af32x16 sc[8];
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) sc[kt][e] = 0.0f;

    // LDS-DMA staging of a 128-key block of K (col0 = Hd) or V (col0 = 2 Hd): one wave-instruction writes 8 rows of 128 B of
    // one plane linearly; chunk c' of row r is fetched from source chunk c' ^ f(r).  Rows past the window re-read its last row.
    auto stage = [&](int col0, int key0, unsigned short* dst, bool is_v) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ins = wv * 8 + i;                                         // 32 wave-instructions per block
            const int pl = ins >> 4, r = 8 * (ins & 15) + (lane >> 3), pc = lane & 7;
            const int key = key0 + r < T ? key0 + r : T - 1;
            const int c = pc ^ (is_v ? (((r >> 1) & 1) << 2) : ((r >> 1) & 7));
            __builtin_amdgcn_global_load_lds((attn_glb_ptr)(base + col0 + pl * in_plane + (int64_t)key * ld + 8 * c),
                                             (attn_lds_ptr)(dst + ins * 512), 16, 0, 0);
        }
    };
    auto drain = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };
    unsigned short* buf0 = kvh;
    unsigned short* buf1 = kvh + TILE;

    // ---- scores: block b of K lives in buf[b]; the next block (K1, then V0) is in flight during the multiply ----
    stage(Hd, 0, buf0, false);
    drain();
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (b < nblk) {
            const unsigned short* cur = b == 0 ? buf0 : buf1;
            if (b + 1 < nblk) stage(Hd, KB * (b + 1), buf1, false);            // K1 -> buf1 while K0 is multiplied
            else stage(2 * Hd, 0, b == 0 ? buf1 : buf0, true);                 // last K block: V0 -> the other buffer
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) {
                const int kt = 4 * b + t4;
                const int row = 32 * t4 + l31;
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    const int off = row * HD + 8 * ((2 * s4 + h) ^ ((row >> 1) & 7));
                    const ah8 kh = *reinterpret_cast<const ah8*>(cur + off);
                    const ah8 kl = *reinterpret_cast<const ah8*>(cur + PLANE + off);
                    sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[s4], sc[kt], 0, 0, 0);
                    sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[s4], sc[kt], 0, 0, 0);
                    sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[s4], sc[kt], 0, 0, 0);
                }
            }
            drain();
        }
    }
    // V0 now sits in buf1 (one key block) or buf0 (two key blocks)
    // ---- softmax over the keys of this lane's query: key = 32 kt + (e & 3) + 8 (e >> 2) + 4 h ----
    const float sscale = scale * sinv * sinv;                                   // q and k both carry s_w
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = 32 * kt + (e & 3) + 8 * (e >> 2) + 4 * h;
            float v;
            if constexpr (RELPOS) {                                             // (the table read is unconditional: in bounds for every key)
                const float sv = fmaf(qgate, qtab[key], sc[kt][e] * sscale);
                v = key < T ? sv : -INFINITY;
            } else {
                v = key < T ? sc[kt][e] * sscale : -INFINITY;
            }
            sc[kt][e] = v;
            m = fmaxf(m, v);
        }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.0f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float ev = expf(sc[kt][e] - m);                               // exp(-inf) = 0 for the padded keys
            sc[kt][e] = ev;
            sum += ev;
        }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 16384.0f / sum;                                           // probabilities travel as p * 2^14 (hi + lo)

    // ---- O = P V ----
    af32x16 o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.0f; o1[e] = 0.0f; }
    // transposed-read addressing: 16-lane group gq covers columns 16 (gq & 1) .. + 15 of a column tile and the 4 keys of lane
    // half h = gq >> 1; lane 4 q + p of the group supplies row q, columns 4 p .. 4 p + 3
    const int gq = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (b < nblk) {
            // V block b: V0 is where the score phase left it, V1 goes to the other buffer while V0 is multiplied
            unsigned short* v0buf = nblk == 1 ? buf1 : buf0;
            const unsigned short* cur = b == 0 ? v0buf : (v0buf == buf0 ? buf1 : buf0);
            if (b == 0 && nblk > 1) stage(2 * Hd, KB, v0buf == buf0 ? buf1 : buf0, true);
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) {
                const int kt = 4 * b + t4;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    ah8 ph, pl;                                                 // A operand: this lane's query, keys of k-step s2
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float pn = sc[kt][8 * s2 + j] * inv;
                        const _Float16 hi = (_Float16)pn;
                        ph[j] = hi;
                        pl[j] = (_Float16)(pn - (float)hi);
                    }
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        // (volatile asm with a memory clobber: the reads stay behind the barrier that publishes the staged
                        // block, the wait for the four results is explicit and tied to them)
                        atr4 th0, th1, tl0, tl1;
                        {
                            const int rowa = 32 * t4 + 16 * s2 + 4 * (gq >> 1) + tq, rowb = rowa + 8;      // keys within the staged block
                            const int cha = (4 * ct + 2 * (gq & 1) + (tp >> 1)) ^ (((rowa >> 1) & 1) << 2);
                            const int chb = (4 * ct + 2 * (gq & 1) + (tp >> 1)) ^ (((rowb >> 1) & 1) << 2);
                            const unsigned a0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const unsigned short*)(cur + rowa * HD + 8 * cha + 4 * (tp & 1));
                            const unsigned a1 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const unsigned short*)(cur + rowb * HD + 8 * chb + 4 * (tp & 1));
                            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(th0) : "v"(a0) : "memory");
                            asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(th1) : "v"(a1) : "memory");
                            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(tl0) : "v"(a0), "n"(2 * PLANE) : "memory");
                            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(tl1) : "v"(a1), "n"(2 * PLANE) : "memory");
                            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(th0), "+v"(th1), "+v"(tl0), "+v"(tl1) : : "memory");
                        }
                        // (whole-vector moves: rebuilding the fragments element by element from the 4-element results,
                        // `vh[j] = bit_cast(th0[j])`, came out of hipcc 7.2 as a broadcast of element 0)
                        typedef short atr8 __attribute__((__vector_size__(8 * sizeof(short))));
                        const ah8 vh = __builtin_bit_cast(ah8, __builtin_shufflevector(th0, th1, 0, 1, 2, 3, 4, 5, 6, 7));
                        const ah8 vl = __builtin_bit_cast(ah8, __builtin_shufflevector(tl0, tl1, 0, 1, 2, 3, 4, 5, 6, 7));
                        if (ct == 0) {
                            o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(pl, vh, o0, 0, 0, 0);
                            o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, vl, o0, 0, 0, 0);
                            o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, vh, o0, 0, 0, 0);
                        } else {
                            o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(pl, vh, o1, 0, 0, 0);
                            o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, vl, o1, 0, 0, 0);
                            o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, vh, o1, 0, 0, 0);
                        }
                    }
                }
            }
            if (b == 0 && nblk > 1) drain();
        }
    }
    // C layout: column = lane & 31 (d), row = (e & 3) + 8 (e >> 2) + 4 h (query within the wave's 32).  acc * 2^-14 = o * s_w:
    // already the out-projection's A operand in the window's scale (|o| <= max |v| of the window, and v * s_w < 2^15).
    // k16 panels of n_rows rows (gemm_f16x3.h): column head * 64 + 32 u + l31 -> panel 4 head + 2 u + (l31 >> 4), k = l31 & 15
    const int64_t panel_sz = n_rows * 16;
    unsigned short* op = planes + ((int64_t)(head * 4) + (l31 >> 4)) * panel_sz + wrow0 * 16 + (l31 & 15);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int q = q0 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (q < T) {
            unsigned short* d0 = op + (int64_t)q * 16;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float x = (u == 0 ? o0[e] : o1[e]) * (1.0f / 16384.0f);
                unsigned short a2, b2;
                split2_w(x, a2, b2);
                d0[2 * u * panel_sz] = a2;
                d0[plane_stride + 2 * u * panel_sz] = b2;
            }
        }
    }
}

// one power of two per window for the q / k / v projection's plane output: the bound of the window's rows,
// max_rows |y|_2 * max_n |w_n|_2 + max |b|, written per row (the GEMM's c_scale / the attention's scale / the out-projection's a_scale)
__global__ __launch_bounds__(256) void qkv_scale_kernel(const unsigned* __restrict__ win_norm, const int* __restrict__ rowwin,
                                                        int64_t rows, const unsigned* __restrict__ wst, const unsigned* __restrict__ bst,
                                                        float* __restrict__ row_scale) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float bound = __uint_as_float(win_norm[rowwin[r]]) * __uint_as_float(wst[0]) * 1.000001f + __uint_as_float(bst[1]);
    row_scale[r] = f16x2_scale_for_bound(bound);
}

// ---- WavLM's bias gate (REL_POS_BIAS): gate[row][head] = a (b const[head] - 1) + 2, a = sigmoid(x . ga + ba), b = sigmoid(x . gb + bb)
// over the head's hd values of the fp32 row the q/k/v projection reads.  16 lanes per (row, head): a wave instruction reads
// four whole 64-wide heads (1 KB contiguous); the two weight rows sit in LDS.
__global__ __launch_bounds__(256) void relpos_gate_kernel(const float* __restrict__ x, int64_t items, int NH, int hd,
                                                          const float* __restrict__ ga, const float* __restrict__ gb,
                                                          const float* __restrict__ gbias, const float* __restrict__ gconst,
                                                          float* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(16))) float gw[];                  // ga[hd] | gb[hd]
    for (int i = threadIdx.x; i < 2 * hd; i += 256) gw[i] = i < hd ? ga[i] : gb[i - hd];
    __syncthreads();
    const int sub = threadIdx.x & 15;
    const int64_t raw = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int64_t item = raw < items ? raw : items - 1;                         // = row * NH + head; its values start at item * hd
    const float4* xp = reinterpret_cast<const float4*>(x + item * hd);
    const float4* a4 = reinterpret_cast<const float4*>(gw);
    const float4* b4 = reinterpret_cast<const float4*>(gw + hd);
    float a = 0.0f, b = 0.0f;
    for (int k = sub; k < (hd >> 2); k += 16) {
        const float4 v = xp[k], wa = a4[k], wb = b4[k];
        a += (v.x * wa.x + v.y * wa.y) + (v.z * wa.z + v.w * wa.w);
        b += (v.x * wb.x + v.y * wb.y) + (v.z * wb.z + v.w * wb.w);
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if (sub == 0 && raw < items) {
        const float sa = 1.0f / (1.0f + expf(-(a + gbias[0]))), sb = 1.0f / (1.0f + expf(-(b + gbias[1])));
        gate[item] = sa * (sb * gconst[item % NH] - 1.0f) + 2.0f;
    }
}

// ---- row softmax in place, one wave per row of length T (row stride Tp, pad columns zeroed) ---------
// Tp <= 256 (every Wav2Vec2 window: T <= 249): the row lives in one float4 per lane, one load + one store
// RELPOS (REL_POS_BIAS): row = (window, head, q) of a run of equal windows whose first encoder row is xrow0; the row takes
// + gate[q][head] * tab[head][c - q] while it is read (c - q clamped to the table: exact, see rsaf.h).  The plain instances
// never read the four trailing arguments.
template <bool SMALL, bool RELPOS = false>
__global__ __launch_bounds__(256) void softmax_kernel(float* __restrict__ S, int64_t rows, int T, int Tp,
                                                      const float* __restrict__ gate, const float* __restrict__ reltab, int NH,
                                                      int64_t xrow0) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    float* p = S + row * Tp;
    float g = 0.0f;
    const float* tab = nullptr;                               // the head's table, tab[0] = distance 0
    int q = 0;
    if constexpr (RELPOS) {
        const int64_t wh = row / T;
        q = (int)(row - wh * T);
        const int head = (int)(wh % NH);
        g = gate[(xrow0 + (wh / NH) * T + q) * NH + head];
        tab = reltab + (int64_t)head * REL_TAB + (REL_SPAN - 1);
    }
    auto bias = [&](int c) {                                  // key c of this row's query
        const int d = c - q;
        return g * tab[d < -(REL_SPAN - 1) ? -(REL_SPAN - 1) : (d > REL_SPAN - 1 ? REL_SPAN - 1 : d)];
    };
    if (SMALL) {
        const int c0 = 4 * lane;
        float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (c0 < Tp) v = reinterpret_cast<const float4*>(p)[lane];
        float e[4] = {v.x, v.y, v.z, v.w};
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (RELPOS) { if (c0 + i < T) e[i] += bias(c0 + i); }
            if (c0 + i >= T) e[i] = -INFINITY;
            m = fmaxf(m, e[i]);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { e[i] = (c0 + i < T) ? expf(e[i] - m) : 0.f; s += e[i]; }
        s = wave_sum(s);
        const float inv = 1.0f / s;
        if (c0 < Tp) reinterpret_cast<float4*>(p)[lane] = make_float4(e[0] * inv, e[1] * inv, e[2] * inv, e[3] * inv);
        return;
    }
    float m = -INFINITY;
    for (int c = lane; c < T; c += 64) {
        if constexpr (RELPOS) p[c] += bias(c);
        m = fmaxf(m, p[c]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.f;
    for (int c = lane; c < T; c += 64) { const float e = expf(p[c] - m); p[c] = e; s += e; }
    s = wave_sum(s);
    const float inv = 1.0f / s;
    for (int c = lane; c < Tp; c += 64) p[c] = c < T ? p[c] * inv : 0.0f;
}

// ---- regroup for the grouped positional conv: xg[chunk][g][tt][ci], zero padded in time -----------
__global__ __launch_bounds__(256) void regroup_kernel(const float4* __restrict__ x, float4* __restrict__ xg, int n,
                                                      int T, int Hd4, int G, int K) {
    const int cg4 = Hd4 / G;
    const int TT = T + K - 1;
    const int64_t total = (int64_t)n * G * TT * cg4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ci = (int)(i % cg4);
        int64_t r = i / cg4;
        const int tt = (int)(r % TT); r /= TT;
        const int g = (int)(r % G);
        const int64_t chunk = r / G;
        const int t = tt - K / 2;
        xg[i] = (t >= 0 && t < T) ? x[(chunk * T + t) * Hd4 + g * cg4 + ci] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// the same regrouping as two fp16 planes (A operand of the positional convolution on the f16x3 GEMM), scaled per window by
// the power of two that the window's largest |x| (reported by the feature projection's epilogue) asks for
__global__ __launch_bounds__(256) void regroup_planes_kernel(const float4* __restrict__ x, unsigned short* __restrict__ xg,
                                                             int64_t plane, int n, int Tmax, int Hd4, int G, int K,
                                                             const int* __restrict__ Tw, const int64_t* __restrict__ row0,
                                                             const unsigned* __restrict__ amax, float* __restrict__ win_scale) {
    // destination per (window, group): Tmax + K - 1 rows of cg channels, frame t of window w at tt = t + K / 2, zeros around its T_w frames
    const int cg4 = Hd4 / G;
    const int TT = Tmax + K - 1;
    const int64_t total = (int64_t)n * G * TT * cg4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ci = (int)(i % cg4);
        int64_t r = i / cg4;
        const int tt = (int)(r % TT); r /= TT;
        const int g = (int)(r % G);
        const int64_t chunk = r / G;
        const int t = tt - K / 2;
        const float sc = f16x2_scale_for_bound(__uint_as_float(amax[chunk]));
        if (g == 0 && tt == 0 && ci == 0) win_scale[chunk] = sc;
        const float4 v = (t >= 0 && t < Tw[chunk]) ? x[(row0[chunk] + t) * Hd4 + g * cg4 + ci] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float vv[4] = {v.x * sc, v.y * sc, v.z * sc, v.w * sc};
        unsigned short hh[4], ll[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) split2_w(vv[k], hh[k], ll[k]);
        // k16 panels per (window, group): [cg / 16][TT][16] - tap k of output frame t is panel row t + k, so the GEMM's DMA
        // moves 32 consecutive rows of a panel as one contiguous KiB (a_tap_panels = cg / 16)
        unsigned short* pp = xg + ((((chunk * G + g) * (cg4 / 4) + (ci >> 2)) * TT + tt) * 16 + (ci & 3) * 4);
        *reinterpret_cast<uint2*>(pp) = make_uint2(hh[0] | ((unsigned)hh[1] << 16), hh[2] | ((unsigned)hh[3] << 16));
        *reinterpret_cast<uint2*>(pp + plane) = make_uint2(ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16));
    }
}

// ---- positional convolution: the window's panel image stays in LDS -----------------------------------------------------------
// As a batched GEMM (gemm_f16x3, 256 x 64 tiles) every k-tile of the 128-tap convolution re-reads its A tile from L2 although
// consecutive taps differ by ONE ROW: 6.3 MB of DMA per tile, 755 GB per 1 000 clips, 6.7 TB/s - the kernel sat on the L2 -> LDS
// path at 125 TFLOP/s-equivalent whatever the tile shape.  Here a workgroup owns one (window, group): the group's cg channels of
// the zero-padded window ([cg / 16 panels][T_w + PK - 1 rows][16], both fp16 planes: 120 KB at base geometry) are fetched ONCE,
// tap k of output row t is LDS row t + k, and only the weights stream (6 KB per step of two k16 units, four stages).  Eight
// waves x 64 rows; v_mfma_f32_16x16x32_f16 so that the 48 output channels are three full column tiles; the arithmetic is the
// GEMM's (a_l b_h + a_h b_l + a_h b_h, fp32 accumulation, power-of-two scales undone in the epilogue, bias, GELU).
// Rows and halves are stored with the GEMM's swizzle (16-byte half h of row r in slot h ^ ((r >> 3) & 1)): lanes r and r + 8 of a
// fragment read then hit different banks for any tap offset.
typedef _Float16 pc_f16x8 __attribute__((ext_vector_type(8)));
typedef float pc_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* pc_lds_ptr;
typedef const __attribute__((address_space(1))) void* pc_glb_ptr;
constexpr int PC_ROWS = 512;                     // output rows per workgroup with SPLIT = 1 (8 waves x 4 row tiles of 16)

// SPLIT = 2 (windows of at most 256 frames - the 5 s windows of the extractor give 249): 256 rows per workgroup, waves 0-3 take
// the even steps and waves 4-7 the odd ones (split K; the halves meet through LDS in front of the epilogue), so that all eight
// waves have rows to work on and each weight step is read from LDS by four waves instead of eight.
template <int NT, int SPLIT>
__global__ __launch_bounds__(512, 1) void posconv_f16x3_kernel(const unsigned short* __restrict__ xg, int64_t a_plane,
                                                               const unsigned short* __restrict__ wp, int64_t b_plane, int Hd,
                                                               const float* __restrict__ a_scale, const float* __restrict__ b_scale,
                                                               const float* __restrict__ bias, const int* __restrict__ Tw,
                                                               const int64_t* __restrict__ row0, float* __restrict__ y, int G, int TT,
                                                               int PK, int rows_alloc) {
    extern __shared__ __attribute__((aligned(1024))) unsigned short pc_sm[];
    constexpr int cg = 16 * NT, B_SEG = cg * 16, B_STAGE = 4 * B_SEG, B_INSTR = cg / 8, RGRPS = 8 / SPLIT;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = blockIdx.x / G, g = blockIdx.x - w * G;
    const int a_panel = rows_alloc * 16;                                   // elements per (plane, panel)
    unsigned short* sA = pc_sm;
    unsigned short* sB = pc_sm + 2 * NT * a_panel;
    // the window's image -> LDS: instruction ii = (plane, panel, block of 32 rows), 1 KiB each
    {
        const int blocks = rows_alloc / 32, total = 2 * NT * blocks;
        const int r_in = lane >> 1, slot = lane & 1;
        for (int ii = wave; ii < total; ii += 8) {
            const int pp = ii / blocks, rb = ii - pp * blocks;             // pp = plane * NT + panel
            const int pl = pp / NT, panel = pp - pl * NT;
            const int row = rb * 32 + r_in;
            const int srow = row < TT ? row : TT - 1;
            const int chunk = slot ^ ((row >> 3) & 1);
            const unsigned short* src = xg + pl * a_plane + ((((int64_t)w * G + g) * NT + panel) * TT + srow) * 16 + chunk * 8;
            __builtin_amdgcn_global_load_lds((pc_glb_ptr)src, (pc_lds_ptr)(sA + pp * a_panel + rb * 512), 16, 0, 0);
        }
    }
    // weights: step j = units 2 j, 2 j + 1 (a unit = 16 k of one tap); stage layout [unit in pair][plane][cg rows][16].
    // Iteration i = steps SPLIT i .. SPLIT i + SPLIT - 1, ring of four iterations.
    const int nit = PK * NT / 2 / SPLIT;
    int64_t boff = 0;
    if (wave < B_INSTR) {
        const int c = wave * 64 + lane;                                    // 16-byte chunk of the stage
        const int seg = c / (2 * cg), within = c - seg * (2 * cg);
        const int row = within >> 1, slot = within & 1;
        boff = (int64_t)(seg & 1) * b_plane + ((int64_t)(seg >> 1) * Hd + (g * cg + row)) * 16 + (slot ^ ((row >> 3) & 1)) * 8;
    }
    auto b_dma = [&](int i) {
        if (wave < B_INSTR) {
#pragma unroll
            for (int kh = 0; kh < SPLIT; ++kh)
                __builtin_amdgcn_global_load_lds((pc_glb_ptr)(wp + boff + (int64_t)(SPLIT * i + kh) * 2 * Hd * 16),
                                                 (pc_lds_ptr)(sB + ((i & 3) * SPLIT + kh) * B_STAGE + wave * 512), 16, 0, 0);
        }
    };
    b_dma(0);
    if (nit > 1) b_dma(1);
    if (nit > 2) b_dma(2);
    pc_f32x4 acc[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = pc_f32x4{0.f, 0.f, 0.f, 0.f};
    const int r16 = lane & 15, q = lane >> 4, hlf = q & 1, upair = q >> 1;
    const int khalf = wave / RGRPS, m_base = (wave - khalf * RGRPS) * 64;
    // fragments of a step: B from its stage of the ring, A from the resident image at the step's tap
    struct Frag { pc_f16x8 ah[4], al[4], bh[NT], bl[NT]; };
    auto fetch = [&](int i, Frag& F) {
        const int unit = 2 * (SPLIT * i + khalf) + upair;
        const int tap = unit / NT, panel = unit - tap * NT;
        const unsigned short* bst = sB + ((i & 3) * SPLIT + khalf) * B_STAGE + upair * 2 * B_SEG;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int brow = 16 * nt + r16;
            const int off = brow * 16 + ((hlf ^ ((brow >> 3) & 1)) << 3);
            F.bh[nt] = *reinterpret_cast<const pc_f16x8*>(bst + off);
            F.bl[nt] = *reinterpret_cast<const pc_f16x8*>(bst + B_SEG + off);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int row = m_base + 16 * mt + r16 + tap;
            const int off = panel * a_panel + row * 16 + ((hlf ^ ((row >> 3) & 1)) << 3);
            F.ah[mt] = *reinterpret_cast<const pc_f16x8*>(sA + off);
            F.al[mt] = *reinterpret_cast<const pc_f16x8*>(sA + NT * a_panel + off);
        }
    };
    auto mfmas = [&](const Frag& F) {                                     // product by product: 4 NT independent accumulators
#pragma unroll                                                             // between two instructions on the same one
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F.al[mt], F.bh[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F.ah[mt], F.bl[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F.ah[mt], F.bh[nt], acc[mt][nt], 0, 0, 0);
    };
    // Software pipeline: at the top of iteration i the fragments of iteration i are in registers; the wave waits for its share
    // of iteration i + 1's weights (issued two iterations ago), the barrier publishes everybody's and frees the ring slot of
    // iteration i + 3 (read as fragments during iteration i - 2), the DMA of iteration i + 3 goes out, the fragments of
    // iteration i + 1 are requested and the 36 MFMAs of this iteration run while they arrive.
    Frag F0, F1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the image and the first three weight iterations
    __syncthreads();
    fetch(0, F0);
    auto step = [&](int i, const Frag& cur, Frag& nxt) {
        if (i >= 1) {
            if (i + 2 < nit) { if constexpr (SPLIT == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); }
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        if (i + 3 < nit) b_dma(i + 3);
        if (i + 1 < nit) fetch(i + 1, nxt);
        mfmas(cur);
    };
    for (int i = 0; i < nit; i += 2) {                                     // nit is even (launcher)
        step(i, F0, F1);
        step(i + 1, F1, F0);
    }
    if constexpr (SPLIT == 2) {                                            // the odd steps' sums join the even steps' through LDS
        __syncthreads();                                                   // (the image is dead)
        float* red = reinterpret_cast<float*>(pc_sm) + (wave - khalf * RGRPS) * (4 * NT * 4 * 64);
        if (khalf == 1) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int v = 0; v < 4; ++v) red[((mt * NT + nt) * 4 + v) * 64 + lane] = acc[mt][nt][v];
        }
        __syncthreads();
        if (khalf == 1) return;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[mt][nt][v] += red[((mt * NT + nt) * 4 + v) * 64 + lane];
    }
    // epilogue: D of the 16 x 16 tile: lane (q, r16), register v = row 4 q + v, column r16
    const int Tv = Tw[w];
    const int64_t r0 = row0[w];
    const float sa_inv = pow2_inverse(a_scale[w]);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = g * cg + 16 * nt + r16;
        const float inv = sa_inv * pow2_inverse(b_scale[col]);
        const float bs = bias[col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int v = 0; v < 4; v += 2) {
                const int m = m_base + 16 * mt + 4 * q + v;
                const gelu_f32x2 g2 = gelu_pair(gelu_f32x2{acc[mt][nt][v] * inv + bs, acc[mt][nt][v + 1] * inv + bs});
                if (m < Tv) y[(r0 + m) * Hd + col] = g2.x;
                if (m + 1 < Tv) y[(r0 + m + 1) * Hd + col] = g2.y;
            }
    }
}

// ---- positional convolution STACK (RSAF_W2V2_POS_CONV_STACK: data2vec-audio) ---------------------------------------------------
// D layers of p <- GELU(LN(conv(p))): grouped convolution of PK taps with bias, LayerNorm over all Hd channels of a frame
// without weight or bias (eps 1e-5), GELU.  The LayerNorm couples the groups of a frame, so a layer is two launches:
//   posstack_conv_kernel  one workgroup = PS_ROWS frames of one (window, group): the pre-LN values (+ bias) as fp32 rows
//   posstack_rows_kernel  one wave per frame: LayerNorm + GELU over the Hd channels, out as the fp16 plane pair the next
//                         layer's convolution multiplies (or, after the last layer, as fp32 rows for encoder.layer_norm)
// The planes are plain packed rows [rows][Hd]; the convolution zero-fills the frames outside [0, T_w) of ITS window while it
// copies its row tile (+ PK - 1 halo rows) into LDS, so no halo ever reads a neighbouring window's rows and a ragged call
// computes what the per-window calls compute.  From layer 1 on |p| <= sqrt(Hd - 1) (GELU of a normalised row), so the A
// planes' power-of-two scale is a constant of the geometry; layer 0 reads x under the window's scale (W.fp_amax).
// The convolution is the f16x3 arithmetic of posconv_f16x3_kernel (a_l b_h + a_h b_l + a_h b_h on v_mfma_f32_16x16x32_f16, fp32
// accumulation), with the same LDS image layout ([plane][cg / 16 panels][rows][16], 16-byte halves swizzled by (row >> 3) & 1)
// and the same weight panels; PK cg / 16 may be odd (19 x 3 = 57 units of 16 k): the last MFMA's upper half multiplies zeros.
// Four waves x 64 rows; a wave reads its weight fragments from global memory (panel layout: 512 contiguous bytes per 16 lanes),
// one step ahead of the MFMAs that consume them.
constexpr int PS_ROWS = 256;                     // output frames per workgroup (4 waves x 4 row tiles of 16)
static int posstack_rows_alloc(int PK) { return PS_ROWS + PK - 1; }
static size_t posstack_lds_bytes(int cg, int PK) { return (size_t)2 * cg * posstack_rows_alloc(PK) * sizeof(unsigned short); }

template <int NT>
__global__ __launch_bounds__(256) void posstack_conv_kernel(const unsigned short* __restrict__ ap, int64_t a_plane,
                                                            const unsigned short* __restrict__ wp, int64_t b_plane, int Hd,
                                                            const float* __restrict__ a_scale, float a_scale_const,
                                                            const float* __restrict__ b_scale, const float* __restrict__ bias,
                                                            const int* __restrict__ Tw, const int64_t* __restrict__ row0,
                                                            float* __restrict__ pre, int PK, int tiles, int rows_alloc) {
    extern __shared__ __attribute__((aligned(16))) unsigned short ps_sm[];
    constexpr int cg = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = blockIdx.x / tiles, tile = blockIdx.x - w * tiles, g = blockIdx.y;
    const int Tv = Tw[w], t0 = tile * PS_ROWS;
    if (t0 >= Tv) return;                                                  // the whole workgroup: a window shorter than the longest
    const int64_t r0 = row0[w];
    const int a_panel = rows_alloc * 16;                                   // elements per (plane, panel)
    // the tile's image: LDS row lr = frame t0 - PK / 2 + lr of THIS window, zeros outside [0, T_w)
    {
        constexpr int chunks = 2 * NT;                                     // 16-byte pieces of a row's cg channels
        const int total = 2 * rows_alloc * chunks;
        for (int i = tid; i < total; i += 256) {
            const int ch = i % chunks, r = i / chunks;
            const int pl = r / rows_alloc, lr = r - pl * rows_alloc;
            const int t = t0 - PK / 2 + lr;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (t >= 0 && t < Tv) v = *reinterpret_cast<const uint4*>(ap + pl * a_plane + (r0 + t) * Hd + g * cg + ch * 8);
            *reinterpret_cast<uint4*>(ps_sm + (pl * NT + (ch >> 1)) * a_panel + lr * 16 + (((ch & 1) ^ ((lr >> 3) & 1)) << 3)) = v;
        }
    }
    __syncthreads();
    const int nunits = PK * NT, nsteps = (nunits + 1) / 2;                 // a unit = 16 k of one tap; a step = one MFMA depth of 32
    const int r16 = lane & 15, q = lane >> 4, hlf = q & 1, upair = q >> 1;
    const int m_base = wave * 64;
    pc_f32x4 acc[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = pc_f32x4{0.f, 0.f, 0.f, 0.f};
    struct BFrag { pc_f16x8 h[NT], l[NT]; };
    const pc_f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    // this lane's unit of step j (the upper half of an odd count's last step has none: its weights read as zeros)
    auto fetch_b = [&](int j, BFrag& B) {
        const int unit = 2 * j + upair;
        const bool ok = unit < nunits;
        const unsigned short* src = wp + ((int64_t)(ok ? unit : 0) * Hd + g * cg + r16) * 16 + hlf * 8;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            B.h[nt] = ok ? *reinterpret_cast<const pc_f16x8*>(src + nt * 256) : zero8;
            B.l[nt] = ok ? *reinterpret_cast<const pc_f16x8*>(src + b_plane + nt * 256) : zero8;
        }
    };
    auto mfmas = [&](int j, const BFrag& B) {
        const int unit = 2 * j + upair;
        const int u = unit < nunits ? unit : 0;
        const int tap = u / NT, panel = u - tap * NT;
        pc_f16x8 ah[4], al[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int row = m_base + 16 * mt + r16 + tap;
            const int off = panel * a_panel + row * 16 + ((hlf ^ ((row >> 3) & 1)) << 3);
            ah[mt] = *reinterpret_cast<const pc_f16x8*>(ps_sm + off);
            al[mt] = *reinterpret_cast<const pc_f16x8*>(ps_sm + NT * a_panel + off);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[mt], B.h[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], B.l[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], B.h[nt], acc[mt][nt], 0, 0, 0);
    };
    BFrag B0, B1;
    fetch_b(0, B0);
    for (int j = 0; j < nsteps; j += 2) {
        if (j + 1 < nsteps) fetch_b(j + 1, B1);
        mfmas(j, B0);
        if (j + 1 < nsteps) {
            if (j + 2 < nsteps) fetch_b(j + 2, B0);
            mfmas(j + 1, B1);
        }
    }
    // epilogue: lane (q, r16), register v = row 4 q + v, column r16 of a 16 x 16 tile: the pre-LN value, scales undone, + bias
    const float sa_inv = pow2_inverse(a_scale ? a_scale[w] : a_scale_const);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = g * cg + 16 * nt + r16;
        const float inv = sa_inv * pow2_inverse(b_scale[col]);
        const float bs = bias[col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int m = t0 + m_base + 16 * mt + 4 * q + v;
                if (m < Tv) pre[(r0 + m) * Hd + col] = acc[mt][nt][v] * inv + bs;
            }
    }
}

// One wave per frame of D <= 1024 channels.  MODE 0: the row as it is (layer 0's input x) -> planes under its window's scale
// (from the largest |x| of the window, which also goes to win_scale).  MODE 1: LayerNorm without weight or bias (eps 1e-5)
// + GELU -> planes under the constant scale.  MODE 2: the same -> fp32 rows of `out` (which may be `src`: the wave holds the row).
template <int MODE>
__global__ __launch_bounds__(256) void posstack_rows_kernel(const float* src, int64_t rows, int D, const int* __restrict__ rowwin,
                                                            const unsigned* __restrict__ amax, float* __restrict__ win_scale,
                                                            float const_scale, unsigned short* __restrict__ planes, int64_t plane,
                                                            float* out) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int D4 = D >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(src + row * D);
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = lane + 64 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < D4) { v[i] = x4[idx]; s += (v[i].x + v[i].y) + (v[i].z + v[i].w); }
    }
    float sc = const_scale;
    if constexpr (MODE == 0) {
        const int w = rowwin[row];
        sc = f16x2_scale_for_bound(__uint_as_float(amax[w]));
        if (lane == 0) win_scale[w] = sc;                                  // every row of the window writes the same value
    } else {
        const float mean = wave_sum(s) / D;
        float qq = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = lane + 64 * i;
            if (idx < D4) {
                const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
                qq += (a * a + b * b) + (c * c + d * d);
            }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(qq) / D + 1e-5f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const gelu_f32x2 e0 = gelu_pair(gelu_f32x2{(v[i].x - mean) * rstd, (v[i].y - mean) * rstd});
            const gelu_f32x2 e1 = gelu_pair(gelu_f32x2{(v[i].z - mean) * rstd, (v[i].w - mean) * rstd});
            v[i] = make_float4(e0.x, e0.y, e1.x, e1.y);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = lane + 64 * i;
        if (idx >= D4) continue;
        if constexpr (MODE == 2) {
            reinterpret_cast<float4*>(out + row * D)[idx] = v[i];
        } else {
            const float yy[4] = {v[i].x * sc, v[i].y * sc, v[i].z * sc, v[i].w * sc};
            unsigned short hh[4], ll[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) split2_w(yy[k], hh[k], ll[k]);
            unsigned short* pp = planes + row * D + 4 * idx;
            *reinterpret_cast<uint2*>(pp) = make_uint2(hh[0] | ((unsigned)hh[1] << 16), hh[2] | ((unsigned)hh[3] << 16));
            *reinterpret_cast<uint2*>(pp + plane) = make_uint2(ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16));
        }
    }
}

// a step of a sequence that ends at the first error
#define RSAF_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

static int posconv_rows_alloc(int split, int PK) { return (PC_ROWS / split + PK - 1 + 31) & ~31; }
static size_t posconv_lds_bytes(int cg, int PK, int split) {
    return ((size_t)2 * (cg / 16) * posconv_rows_alloc(split, PK) * 16 + (size_t)4 * split * 4 * cg * 16) * sizeof(unsigned short);
}
// posconv_f16x3_kernel keeps a window's regrouped image in LDS: the row split of a window, and whether the image fits
static int posconv_split(int Tt) { return Tt <= PC_ROWS / 2 ? 2 : 1; }
static bool posconv_resident(const Cfg& c, int Tt) {
    const int cg = c.Hd / c.PG, split = posconv_split(Tt);
    return cg <= 64 && Tt <= PC_ROWS && (c.PK * (cg / 16)) % (4 * split) == 0 && posconv_lds_bytes(cg, c.PK, split) <= 160 * 1024;
}

// Operands of one layernorm_kernel launch (every pointer optional unless its group says otherwise)
struct LnArgs {
    // input and residual: the row is x (+ r)
    const float *x = nullptr, *r = nullptr;
    // affine
    const float *g = nullptr, *b = nullptr;
    // fp32 output; with out_row_start, frame t of window w lands at row out_row_start[w] + t.  rowwin / row0: the row -> window
    // map and the windows' first rows, which out_row_start, win_norm and tap_row_start read
    float* out = nullptr;
    const int64_t* out_row_start = nullptr;
    const int* rowwin = nullptr;
    const int64_t* row0 = nullptr;
    // planes output (A of the next GEMM; panel: its k16-panel layout) and the exact row scales that go with it
    unsigned short* planes = nullptr;
    bool panel = false;
    float* scale_out = nullptr;
    // bound inputs {max row norm, max |bias|} of the next GEMM's weights, and the scale of that GEMM's plane output per row
    const unsigned *bound_w = nullptr, *bound_b = nullptr;
    float* bound_scale_out = nullptr;
    // largest row norm per window (bit patterns, atomicMax): behind the scale of the fused attention's q / k / v
    unsigned* win_norm = nullptr;
    // variant (layernorm_kernel's VAR) and its operands: 1 writes x + r to aux, 2 applies the conv LayerNorm pg / pb first
    int var = 0;
    const float *pg = nullptr, *pb = nullptr;
    float* aux = nullptr;
    // hidden-state tap: mode 1 the output, mode 2 the un-normalised x (+ r); rows mapped like out_row_start
    float* tap = nullptr;
    int tap_mode = 0;
    const int64_t* tap_row_start = nullptr;
};

static int ln(const LnArgs& a, int64_t rows, int D, float eps, hipStream_t s) {
    const int64_t blocks = (rows + 3) / 4;
    RSAF_CHECK_ARG(blocks <= 0x7fffffffLL, "too many rows");
    RSAF_CHECK_ARG(!a.planes || a.scale_out, "planes need their scale array");
    RSAF_CHECK_ARG(!a.win_norm || a.rowwin, "the per-window norm needs the row -> window map");
    RSAF_CHECK_ARG((a.var != 1 || a.aux) && (a.var != 2 || (a.pg && a.pb)), "layernorm variant without its operands");
    RSAF_CHECK_ARG(!a.tap || ((a.tap_mode == 1 && a.var == 0) || (a.tap_mode == 2 && a.var < 2)), "layernorm tap mode not built");
    RSAF_CHECK_ARG(!a.tap_row_start || (a.rowwin && a.row0), "the tap row map needs the row -> window map");
    ProfScope prof(a.tap ? "w2v2_layernorm_tap" : "w2v2_layernorm", s, 0.0,
                   (double)rows * D * (4 * (a.r ? 2 : 1) + (a.out ? 4 : 0) + (a.planes ? 4 : 0) + (a.aux ? 4 : 0) + (a.tap ? 4 : 0)));
#define RSAF_LN(...)                                                                                                       \
    hipLaunchKernelGGL((layernorm_kernel<__VA_ARGS__>), dim3((unsigned)blocks), dim3(256), 0, s, a.x, a.r, a.g, a.b, a.out, rows, D, eps, \
                       a.out_row_start, a.rowwin, a.row0, a.planes, rows * D, a.panel ? 1 : 0, a.scale_out, a.bound_w, a.bound_b,   \
                       a.bound_scale_out, a.win_norm, a.pg, a.pb, a.aux, a.tap, a.tap_row_start)
    if (a.tap) {                                             // hidden-state taps: post-LN outputs, pre-LN residual streams
        if (a.tap_mode == 1) RSAF_LN(0, 1);
        else if (a.var == 1) RSAF_LN(1, 2);
        else RSAF_LN(0, 2);
    } else if (a.var == 1) RSAF_LN(1);
    else if (a.var == 2) RSAF_LN(2);
    else if (a.var == 3) RSAF_LN(3);
    else RSAF_LN(0);
#undef RSAF_LN
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// cb: the conv bias (RSAF_W2V2_CONV_BIAS) or NULL
template <bool APPLY>
static int conv0_launch(const Cfg& c, const float* xn, const float* w0, const float* cb, float* part, const float* ab, const float* scale,
                        unsigned short* outp, int64_t plane, int n, int len, const int* T0w, const int* out_off, int T0, int slab, int slabs,
                        hipStream_t s) {
    const int threads = c.C <= 256 ? c.C : 256;
    const int cpt = c.C / threads;
    dim3 grid((unsigned)slabs, (unsigned)n);
    // HBM-bound: the apply pass writes C channels x T0 frames per window as two fp16 planes (4 B per element: 33 MB per
    // 5 s window at C = 512) and reads the window once; the statistics pass only reads the window (both recompute the
    // 10-tap convolution: Cin = 1, 0.16 GFLOP per window)
    ProfScope prof(APPLY ? "w2v2_conv0_apply" : "w2v2_conv0_stats", s, 0.0,
                   APPLY ? (double)n * ((double)c.C * T0 * 4.0 + 4.0 * (5.0 * T0 + 5.0)) : (double)n * 4.0 * (5.0 * T0 + 5.0));
#define RSAF_C0K(CPT, BIAS)                                                                                \
    hipLaunchKernelGGL((conv0_kernel<CPT, APPLY, BIAS>), grid, dim3(threads), 0, s, xn, w0, cb, part, ab, scale, outp, plane, len, T0w, \
                       out_off, c.C, slab, slabs)
#define RSAF_C0(BIAS)                                                                                      \
    switch (cpt) {                                                                                         \
        case 1: RSAF_C0K(1, BIAS); break;                                                                  \
        case 2: RSAF_C0K(2, BIAS); break;                                                                  \
        case 3: RSAF_C0K(3, BIAS); break;                                                                  \
        case 4: RSAF_C0K(4, BIAS); break;                                                                  \
        default: set_error("conv0: unsupported conv_dim"); return RSAF_ERR_ARG;                            \
    }
    if (cb) { RSAF_C0(true) } else { RSAF_C0(false) }
#undef RSAF_C0
#undef RSAF_C0K
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// conv0 + LayerNorm + GELU of the layer-norm feature encoder (one pass, 64 frames per workgroup)
static int conv0_ln_launch(const Cfg& c, const float* xn, const float* w0, const float* cb, const float* lg, const float* lb,
                           const float* scale, unsigned short* outp, int64_t plane, int n, int len, const int* T0w, int T0,
                           int T0g, hipStream_t s) {
    constexpr int FR = 64;
    dim3 grid((unsigned)((T0g + FR - 1) / FR), (unsigned)n);
    ProfScope prof("w2v2_conv0_ln", s, 0.0, (double)n * ((double)c.C * T0g * 4.0 + 4.0 * (5.0 * T0g + 5.0)));
    const int cpt = (c.C + 63) / 64;
#define RSAF_C0L(CPT)                                                                                                      \
    hipLaunchKernelGGL((conv0_ln_kernel<CPT>), grid, dim3(256), 0, s, xn, w0, cb, lg, lb, scale, outp, plane, len, T0w, T0, \
                       c.C, FR)
    switch (cpt) {
        case 1: RSAF_C0L(1); break;
        case 2: RSAF_C0L(2); break;
        case 3: RSAF_C0L(3); break;
        case 4: RSAF_C0L(4); break;
        case 8: RSAF_C0L(8); break;
        case 12: RSAF_C0L(12); break;
        case 16: RSAF_C0L(16); break;
        default: set_error("conv0: unsupported conv_dim"); return RSAF_ERR_ARG;
    }
#undef RSAF_C0L
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// Operands of one f16x3 GEMM, C = act(A B^T + bias (+ R)): A and B as fp16 plane pairs with their power-of-two scales
struct GemmA {
    const uint16_t* planes = nullptr;
    int64_t plane = 0, lda = 0, sA = 0;                      // plane stride, row stride, batch stride
    const float* scale = nullptr;
    int scale_zs = 0, scale_ms = 0;                          // stride of the scale per batch / per row
    bool panel = false;                                      // k16-panel layout (lda, sA unused)
};
struct GemmB {                                               // weights: k16 panels of N rows, one scale per row
    const uint16_t* planes = nullptr;
    const float* scale = nullptr;
};
// the epilogue: what joins the product, where it goes (fp32 rows Cf and / or the planes Cp under c_scale), and the largest
// |output| it reports (amax: per batch at stride amax_zs, or per row slot; columns from amax_col_min on)
struct Out {
    const float* bias = nullptr;
    const float* R = nullptr;                                // residual, laid out like Cf
    int act = ACT_NONE;
    float* Cf = nullptr;
    int64_t sC = 0;
    uint16_t* Cp = nullptr;
    int64_t c_plane = 0, sCp = 0;
    const float* c_scale = nullptr;
    int cs_zs = 0, cs_ms = 0;
    bool cp_panel = false;
    unsigned* amax = nullptr;
    int amax_zs = 0;
    const int* amax_row_slot = nullptr;
    int amax_col_min = 0;
    const int* row_tab = nullptr;                            // packed windows: {slot, destination} per row (GemmH3Params::row_tab)
};

// One forward call: its geometry, buffers and device tables, and one member function per phase (forward_impl runs them in order)
struct Forward {
    const Cfg& c;
    const Rag& R;
    const Layout L;
    const Workspace& W;
    const float* Wt;
    float* ws;
    hipStream_t s;
    // the call's input and outputs.  taps (NULL: no hidden states): taps[k], k = 0..L, receives hidden_states[k] in the row
    // layout of `out`, or is NULL
    const float* wav = nullptr;
    const int64_t* chunk_start = nullptr;
    float* out = nullptr;
    const int64_t* out_row_start = nullptr;
    float* const* taps = nullptr;
    // geometry.  T: frames of the LONGEST window per layer (strides, grids); G: window slots of a feature-encoder pass
    const int n, C, Hd, Tt, G, hd;
    const int* T;
    const int64_t rows;
    const float scale;
    // fused: attention on the fp16 matrix pipe, q / k / v as plane pairs.  relpos (REL_POS_BIAS): the gates come from the fp32
    // rows the q/k/v projection reads: x (post-LN), or LN1(h), which the stable-layer-norm LayerNorms then also write in fp32
    // into the att buffer (free until the attention writes it)
    const bool fused, relpos, pre_ln, layer_norm, conv_bias;
    // window tables on the device (every window has its own length: the reference's tail windows)
    int* Tw;                                                 // [7][n]
    int64_t* row0;
    int64_t* ztab;                                           // [7][n][2]
    int* rowwin;
    int* coff;                                               // [7][G + 1] packed conv row spaces of the current group
    int* crow;                                               // per conv layer and packed row {slot, destination}
    const int* wlen = nullptr;
    // feature encoder: scale of layer i's plane output per window of the group, largest |output| of layer i (layer 0: its
    // bound), the conv biases [7][C], the conv LayerNorms [7][2][C] (layer mode), max |bias| of conv1..5 at 1..5
    float* cscale;                                           // [7][G]
    unsigned* camax;                                         // [7][G]
    const float* cbias;
    const float* cln;
    float* cb_max;                                           // [8]
    float* x;                                                // the encoder's fp32 rows (post-LN: LN outputs; PRE_LN: the residual stream)

    Forward(const Cfg& c_, const Rag& R_, const Workspace& W_, const float* weights, void* workspace, hipStream_t s_)
        : c(c_), R(R_), L(make_layout(c_)), W(W_), Wt(weights), ws(static_cast<float*>(workspace)), s(s_), n(R_.n), C(c_.C), Hd(c_.Hd),
          Tt(R_.Tmax[6]), G(conv_group(R_.n)), hd(c_.Hd / c_.NH), T(R_.Tmax), rows(R_.rows), scale(1.0f / sqrtf((float)hd)),
          fused(fused_attention(c_, Tt)), relpos(c_.flags & F_REL_POS_BIAS), pre_ln(c_.flags & F_PRE_LN),
          layer_norm(c_.flags & F_LAYER_FEAT_NORM), conv_bias(c_.flags & F_CONV_BIAS),
          Tw(reinterpret_cast<int*>(ws + W.t_Tw)), row0(reinterpret_cast<int64_t*>(ws + W.t_row0)),
          ztab(reinterpret_cast<int64_t*>(ws + W.t_ztab)), rowwin(reinterpret_cast<int*>(ws + W.t_rowwin)),
          coff(reinterpret_cast<int*>(ws + W.t_coff)), crow(reinterpret_cast<int*>(ws + W.t_crow)),
          cscale(ws + W.conv_scale), camax(bits_at(W.conv_amax)), cbias(conv_bias ? Wt + L.cb : nullptr), cln(Wt + L.cln),
          cb_max(conv_bias ? ws + W.cb_max : nullptr), x(ws + W.x) {}

    uint16_t* planes_at(int64_t off) const { return reinterpret_cast<uint16_t*>(ws + off); }
    unsigned* bits_at(int64_t off) const { return reinterpret_cast<unsigned*>(ws + off); }
    unsigned* wstat(int idx) const { return bits_at(W.wstat) + 2 * idx; }   // {max row norm, max |element|} of matrix idx
    float* tap(int k) const { return taps ? taps[k] : nullptr; }
    float* gate_rows() const { return relpos ? ws + W.att : nullptr; }     // PRE_LN: where LN1(h) goes in fp32 for the gates
    float* gate() const { return relpos ? ws + W.gate : nullptr; }
    const float* reltab() const { return relpos ? Wt + L.reltab : nullptr; }

    int gemm3(const GemmA& A, const GemmB& B, const Out& o, int M, int N, int K, int nz = 1, const int64_t* zt = nullptr) {
        GemmH3Params p{};
        p.a_panel = A.panel; p.b_panel = 1; p.cp_panel = o.cp_panel;
        p.A = A.planes; p.a_plane = A.plane; p.lda = A.lda; p.sA = A.sA; p.a_scale = A.scale; p.a_scale_zs = A.scale_zs; p.a_scale_ms = A.scale_ms;
        p.B = B.planes; p.b_plane = (int64_t)N * K; p.ldb = 16; p.b_scale = B.scale;
        p.C = o.Cf; p.ldc = N; p.sC = o.sC;
        p.Cp = o.Cp; p.c_plane = o.c_plane; p.ldcp = N; p.sCp = o.sCp; p.c_scale = o.c_scale; p.c_scale_zs = o.cs_zs; p.c_scale_ms = o.cs_ms;
        p.amax_out = o.amax; p.amax_zs = o.amax_zs; p.amax_row_slot = o.amax_row_slot; p.amax_col_min = o.amax_col_min;
        p.bias = o.bias; p.R = o.R; p.ldr = N; p.sR = o.sC;
        p.M = M; p.N = N; p.K = K; p.nz = nz; p.ztab = zt; p.row_tab = o.row_tab; p.act = o.act; p.alpha = 1.0f; p.group_m = 0;
        return launch_gemm_f16x3(p, s, "w2v2_gemm");
    }
    // A = all `rows` encoder rows of K columns as panels, each row with its own scale
    GemmA rows_a(int64_t planes_off, int K, const float* row_scale) const {
        GemmA A;
        A.planes = planes_at(planes_off); A.plane = rows * K; A.lda = K; A.scale = row_scale; A.scale_ms = 1; A.panel = true;
        return A;
    }
    // A of conv i: the channels-last output of layer i - 1, one batch and one scale per window; tap k of a frame = a row shift
    GemmA conv_a(const uint16_t* planes, int i) const {
        GemmA A;
        A.planes = planes; A.plane = (int64_t)G * T[i - 1] * C; A.lda = (int64_t)STRD[i] * C; A.sA = (int64_t)T[i - 1] * C;
        A.scale = cscale + (int64_t)(i - 1) * G; A.scale_zs = 1;
        return A;
    }
    // A of conv i over the packed row space: row R of the GEMM starts at plane row 2 R; the scale comes by the row's window slot
    GemmA conv_a_packed(const uint16_t* planes, int64_t plane, int i) const {
        GemmA A;
        A.planes = planes; A.plane = plane; A.lda = (int64_t)STRD[i] * C;
        A.scale = cscale + (int64_t)(i - 1) * G;
        return A;
    }
    GemmB weights_b(int64_t planes_off, int64_t scale_off) const { return GemmB{planes_at(planes_off), ws + scale_off}; }

    // window tables; len_dev NULL (equal windows): the length table is filled here
    int window_tables(const int* len_dev) {
        wlen = len_dev;
        if (!wlen) {
            int* wl = reinterpret_cast<int*>(ws + W.wlen);
            hipLaunchKernelGGL(fill_i32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, wl, n, R.maxlen);
            wlen = wl;
        }
        hipLaunchKernelGGL(w2v2_tables_kernel, dim3(1), dim3(256), 0, s, wlen, n, C, Hd, Tw, row0, ztab);
        hipLaunchKernelGGL(w2v2_rowwin_kernel, dim3(n), dim3(256), 0, s, row0, rowwin);
        RSAF_CHECK_HIP(hipGetLastError());
        return RSAF_OK;
    }

    int split_wp(int64_t src_off, int64_t nrows, int K, int64_t dst_off, int64_t scale_off, int stat_idx) {
        RSAF_TRY(launch_f16x2_row_scales(Wt + src_off, nrows, K, K, ws + scale_off, nullptr, wstat(stat_idx), s));
        return launch_split_f16x2(Wt + src_off, nrows, K, K, ws + scale_off, 1, planes_at(dst_off), nrows * K, 1, s);
    }
    // 0. weights of the dense layers as fp16 plane pairs in the k16-panel layout, each row with its own power-of-two scale
    //    (once per call: 0.4 GB at base geometry, < 1 ms), and per matrix the largest row norm: the Cauchy-Schwarz factor of
    //    the bound behind the scale of a GEMM's PLANE output (conv1..5, ffn1)
    int weight_planes() {
        RSAF_CHECK_HIP(hipMemsetAsync(ws + W.wstat, 0, sizeof(float) * 2 * (WSTAT_LAYER0 + WSTAT_PER_LAYER * c.L), s));
        for (int i = 0; i < 6; ++i)
            RSAF_TRY(split_wp(L.conv[i], C, KERN[i + 1] * C, W.wp_conv[i], W.ws_conv[i], wstat_conv(i)));
        RSAF_TRY(split_wp(L.fpw, Hd, C, W.wp_fp, W.ws_fp, WSTAT_FP));
        if (c.pos_depth() ? posstack_on_mfma(c) : posconv_on_f16x3(c)) {   // [G cg][PK cg] as panels of Hd rows
            RSAF_TRY(split_wp(L.posw, Hd, c.PK * (Hd / c.PG), W.wp_pos, W.ws_pos, WSTAT_POS));
        }
        for (size_t i = 0; i < W.wp_stack.size(); ++i) {     // POS_CONV_STACK: the stack's layers 1..D-1 (no bound reads their statistics)
            const int K = c.PK * (Hd / c.PG);
            RSAF_TRY(launch_f16x2_row_scales(Wt + L.stackw[i], Hd, K, K, ws + W.ws_stack[i], nullptr, nullptr, s));
            RSAF_TRY(launch_split_f16x2(Wt + L.stackw[i], Hd, K, K, ws + W.ws_stack[i], 1, planes_at(W.wp_stack[i]), (int64_t)Hd * K, 1, s));
        }
        for (int l = 0; l < c.L; ++l) {
            const LayerOff& lo = L.layers[l];
            const int b0 = WSTAT_LAYER0 + WSTAT_PER_LAYER * l;
            RSAF_TRY(split_wp(lo.wqkv, 3 * Hd, Hd, W.wp_qkv[l], W.ws_qkv[l], b0));
            RSAF_TRY(split_wp(lo.wo, Hd, Hd, W.wp_o[l], W.ws_o[l], b0 + 1));
            RSAF_TRY(split_wp(lo.w1, c.I, Hd, W.wp_1[l], W.ws_1[l], b0 + 2));
            RSAF_TRY(split_wp(lo.w2, Hd, c.I, W.wp_2[l], W.ws_2[l], b0 + 3));
            // max |b1| (word 1 of the statistics of the bias seen as one row); the scale it writes goes to a scratch slot
            RSAF_TRY(launch_f16x2_row_scales(Wt + lo.b1, 1, c.I, c.I, ws + W.pos_scale, nullptr, wstat(b0 + 4), s));
            RSAF_TRY(launch_f16x2_row_scales(Wt + lo.bqkv, 1, 3 * Hd, 3 * Hd, ws + W.pos_scale, nullptr, wstat(b0 + 5), s));
        }
        return RSAF_OK;
    }

    // 1-3. feature encoder, G windows at a time (its activations are the large ones: 15 999 x 512 per window)
    int feature_encoder() {
        // window groups of (almost) equal size: ceil(n / G) groups instead of full ones and a small remainder
        const int n_groups = (n + G - 1) / G, gstep = (n + n_groups - 1) / n_groups;
        if (layer_norm) {                                    // layer mode: the planes' scales depend on the weights only
            hipLaunchKernelGGL(lnconv_scale_kernel, dim3(1), dim3(384), 0, s, cln, C, G, cscale);
            RSAF_CHECK_HIP(hipGetLastError());
        } else if (conv_bias) {
            hipLaunchKernelGGL(conv_bias_max_kernel, dim3(1), dim3(64), 0, s, cbias, C, cb_max);
            RSAF_CHECK_HIP(hipGetLastError());
        }
        for (int g0 = 0; g0 < n; g0 += gstep) {
            const int g = std::min(gstep, n - g0);
            // the group's longest window is its first (lengths are non-increasing): its frame counts size the group's launches
            int Tg[7];
            chunk_lengths(R.len[g0], Tg);
            if (!layer_norm) RSAF_CHECK_HIP(hipMemsetAsync(camax, 0, sizeof(unsigned) * 7 * G, s));
            // 1. per-chunk normalisation (HF feature extractor; NO_INPUT_NORM: do_normalize=False, a copy)
            {
                ProfScope prof("w2v2_normalize", s, 0.0, (double)g * R.len[g0] * 4 * 3);
                if (c.flags & F_NO_INPUT_NORM)
                    hipLaunchKernelGGL(normalize_kernel<false>, dim3(g), dim3(256), 0, s, wav, chunk_start + g0, wlen + g0, R.maxlen, ws + W.xn);
                else
                    hipLaunchKernelGGL(normalize_kernel<true>, dim3(g), dim3(256), 0, s, wav, chunk_start + g0, wlen + g0, R.maxlen, ws + W.xn);
                RSAF_CHECK_HIP(hipGetLastError());
            }
            RSAF_TRY(layer_norm ? convs_layer_norm(g0, g, Tg) : convs_group_norm(g0, g, Tg));
        }
        return RSAF_OK;
    }
    // layer mode: conv i of the windows g0 .. g0 + g - 1, one batch per window: every window keeps the longest window's row allotment (batch stride T[i] rows)
    // and has its own row count (ztab); the last layer writes its rows packed (window w at row row0[w])
    int conv_gemm(int i, const uint16_t* a_planes, Out& o, int g0, int g, const int* Tg) {
        if (i == 6) { o.Cf = ws + W.c6; o.sC = 0; }
        o.bias = conv_bias ? cbias + (int64_t)i * C : nullptr;
        return gemm3(conv_a(a_planes, i), weights_b(W.wp_conv[i - 1], W.ws_conv[i - 1]), o, Tg[i], C, KERN[i] * C, g,
                     ztab + ((int64_t)(i - 1) * n + g0) * 2);
    }
    // 2-3 (layer mode). conv0 + LayerNorm + GELU in one pass; conv1..6 as GEMMs writing fp32 rows (+ bias) into the Q buffer,
    // then LayerNorm -> GELU -> planes back into P (the GEMM has consumed them); conv6 writes its packed rows, and its
    // LayerNorm + GELU join the feature projection's LayerNorm (step 4)
    int convs_layer_norm(int g0, int g, const int* Tg) {
        RSAF_TRY(conv0_ln_launch(c, ws + W.xn, Wt + L.conv0, cbias, cln, cln + C, cscale, planes_at(W.P), (int64_t)G * T[0] * C,
                                  g, R.maxlen, Tw + g0, T[0], Tg[0], s));
        for (int i = 1; i < 7; ++i) {
            Out o;
            o.Cf = ws + W.Q; o.sC = (int64_t)T[i] * C;
            RSAF_TRY(conv_gemm(i, planes_at(W.P), o, g0, g, Tg));
            if (i < 6) {
                const int64_t lrows = (int64_t)g * T[i];
                ProfScope prof("w2v2_conv_ln", s, 0.0, (double)lrows * C * 8.0);
                hipLaunchKernelGGL(conv_ln_gelu_kernel, dim3((unsigned)((lrows + 3) / 4)), dim3(256), 0, s, ws + W.Q,
                                   cln + (int64_t)2 * i * C, cln + (int64_t)(2 * i + 1) * C, cscale + (int64_t)i * G,
                                   planes_at(W.P), (int64_t)G * T[i] * C, lrows, T[i], Tw + (int64_t)i * n + g0, C);
                RSAF_CHECK_HIP(hipGetLastError());
            }
        }
        return RSAF_OK;
    }
    // 2-3 (group mode): the windows of the group packed along M (packed_in_rows above)
    int convs_group_norm(int g0, int g, const int* Tg) {
        // rows of every layer's GEMM, and the tables behind them
        int64_t M[7] = {};
        for (int w = g0; w < g0 + g; ++w) {
            int Tw_[7];
            chunk_lengths(R.len[w], Tw_);
            for (int i = 1; i < 7; ++i) M[i] += Tw_[i] + 1;
        }
        RSAF_CHECK_ARG(2 * M[1] + 1 < 0x7fffffffLL && rows < 0x7fffffffLL, "too many conv rows in one group");
        PackBases bases{};
        for (int i = 1; i < 7; ++i) bases.b[i] = packed_tab_base(G, T, i);
        hipLaunchKernelGGL(w2v2_pack_offsets_kernel, dim3(1), dim3(64), 0, s, Tw + g0, n, g, G, coff);
        hipLaunchKernelGGL(w2v2_pack_rows_kernel, dim3(g, 6), dim3(256), 0, s, Tw + g0, n, G, coff, row0 + g0, crow, bases);
        RSAF_CHECK_HIP(hipGetLastError());
        // 2. conv0 + GroupNorm + GELU (stats pass, finalize, apply pass); the apply pass writes fp16 plane pairs
        const int slabs_g = (Tg[0] + STAT_SLAB - 1) / STAT_SLAB;
        RSAF_TRY(conv0_launch<false>(c, ws + W.xn, Wt + L.conv0, cbias, ws + W.part, nullptr, nullptr, nullptr, 0, g, R.maxlen, Tw + g0,
                                      nullptr, T[0], STAT_SLAB, slabs_g, s));
        const int64_t tot = (int64_t)g * C;
        hipLaunchKernelGGL(gn_finalize_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, ws + W.part,
                           Wt + L.gng, Wt + L.gnb, ws + W.ab, camax, g, C, slabs_g, Tw + g0);
        RSAF_CHECK_HIP(hipGetLastError());
        RSAF_TRY(launch_scale_from_bound(camax, g, nullptr, 1.0f, nullptr, cscale, s));
        const int slab = 128;
        const int64_t plane_p = p_rows(G, T) * C, plane_q = q_rows(G, T) * C;
        RSAF_TRY(conv0_launch<true>(c, ws + W.xn, Wt + L.conv0, cbias, nullptr, ws + W.ab, cscale, planes_at(W.P), plane_p, g,
                                     R.maxlen, Tw + g0, coff + (G + 1), T[0], slab, (Tg[0] + slab - 1) / slab, s));
        // 3. conv1..6 as GEMMs over the channels-last sequence (lda = stride * C, K = taps * C) with fused GELU;
        //    the output goes out as planes (the next layer's A), the last one as fp32 rows for the LayerNorm.
        //    Scale of layer i's output, per window: |GELU(x)| <= |x| <= |a|_2 |w|_2 <= sqrt(K) max|a| max_n |w_n|_2 with
        //    max|a| = the largest |output| of layer i - 1, which that layer's epilogue reported (layer 0: the GroupNorm bound).
        uint16_t* cur = planes_at(W.P);
        uint16_t* nxt = planes_at(W.Q);
        int64_t plane_cur = plane_p, plane_nxt = plane_q;
        for (int i = 1; i < 7; ++i) {
            Out o;
            o.act = ACT_GELU;
            o.row_tab = crow + 2 * bases.b[i];
            if (i < 6) {
                // (CONV_BIAS: + max |bias| of layer i)
                RSAF_TRY(launch_scale_from_bound(camax + (int64_t)(i - 1) * G, g, reinterpret_cast<const float*>(wstat(wstat_conv(i - 1))),
                                                  sqrtf((float)(KERN[i] * C)) * 1.00001f, conv_bias ? cb_max + i : nullptr,
                                                  cscale + (int64_t)i * G, s));
                o.Cp = nxt; o.c_plane = plane_nxt;
                o.c_scale = cscale + (int64_t)i * G;
                o.amax = camax + (int64_t)i * G;
            } else {
                o.Cf = ws + W.c6;
            }
            o.bias = conv_bias ? cbias + (int64_t)i * C : nullptr;
            RSAF_TRY(gemm3(conv_a_packed(cur, plane_cur, i), weights_b(W.wp_conv[i - 1], W.ws_conv[i - 1]), o, (int)M[i], C, KERN[i] * C));
            std::swap(cur, nxt);
            std::swap(plane_cur, plane_nxt);
        }
        return RSAF_OK;
    }

    // 4. feature projection: LayerNorm (-> planes, exact row scales) + Linear; its epilogue reports max |x| per window
    int feature_projection() {
        RSAF_CHECK_HIP(hipMemsetAsync(ws + W.fp_amax, 0, sizeof(unsigned) * n, s));
        LnArgs a;
        a.x = ws + W.c6; a.g = Wt + L.fplg; a.b = Wt + L.fplb;
        a.planes = planes_at(W.lnfp); a.panel = true; a.scale_out = ws + W.s_lnfp;
        if (layer_norm) {                                    // conv6's LayerNorm (eps 1e-5) + GELU first, in the same row pass
            a.var = 2; a.pg = cln + (int64_t)12 * C; a.pb = cln + (int64_t)13 * C;
        } else if (c.flags & F_NO_FEAT_PROJ_LN) {            // the conv output itself, as planes
            a.var = 3;
        }
        RSAF_TRY(ln(a, rows, C, c.eps, s));
        Out o;
        o.Cf = x; o.bias = Wt + L.fpb;
        o.amax = bits_at(W.fp_amax); o.amax_row_slot = rowwin;
        return gemm3(rows_a(W.lnfp, C, ws + W.s_lnfp), weights_b(W.wp_fp, W.ws_fp), o, (int)rows, Hd, C);
    }

    // 5. positional conv embedding (grouped, weight norm folded), GELU, then the first LayerNorm of the encoder: x = LN(x + pos),
    //    or, stable layer norm, h = x + pos stays un-normalised (the residual stream) and layer 0's LN1(h) goes to the planes
    int positional_conv() {
        if (posconv_on_f16x3(c)) {
            RSAF_TRY(posconv_regroup_planes());
            const bool pc_off = [] { const char* e = getenv("RSAF_W2V2_POSCONV_GEMM"); return e && e[0] == '1'; }();   // per call: the tests toggle it
            RSAF_TRY((!pc_off && posconv_resident(c, Tt)) ? posconv_lds() : posconv_batched_gemm());
        } else {
            RSAF_TRY(posconv_fp32());
        }
        if (pre_ln) return ln_to_qkv(x, ws + W.y, Wt + L.layers[0].ln1g, Wt + L.layers[0].ln1b, gate_rows(), 0, true, x);
        return ln_to_qkv(x, ws + W.y, Wt + L.elng, Wt + L.elnb, x, 0, true);
    }
    // 5 (POS_CONV_STACK). p_0 = x, p_{i+1} = GELU(LN(conv_i(p_i))), i = 0..D-1 (LN without weight or bias, eps 1e-5), then
    //    x = LN(x + p_D) as above.  The pre-LN rows of every layer go through W.y, which ends up holding p_D; the planes
    //    between the layers live in W.xg (rows x Hd elements per plane: no padding rows, the kernel pads per window)
    int positional_conv_stack() {
        const int D = c.pos_depth(), cg = Hd / c.PG;
        {
            ProfScope prof("w2v2_posconv_stack", s, 2.0 * (double)D * rows * cg * (double)c.PK * cg * c.PG, (double)D * rows * Hd * 16.0);
            RSAF_TRY(posstack_on_mfma(c) ? posstack_mfma(D) : posstack_fp32(D));
        }
        return ln_to_qkv(x, ws + W.y, Wt + L.elng, Wt + L.elnb, x, 0, true);
    }
    template <int MODE>
    int posstack_rows(const float* src, float* dst) {
        hipLaunchKernelGGL(posstack_rows_kernel<MODE>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, src, rows, Hd, rowwin,
                           bits_at(W.fp_amax), ws + W.pos_scale, f16x2_scale_for_bound(sqrtf((float)Hd)), planes_at(W.xg), rows * Hd, dst);
        RSAF_CHECK_HIP(hipGetLastError());
        return RSAF_OK;
    }
    template <int NT>
    int posstack_conv_launch(int i) {
        const int cg = Hd / c.PG, tiles = (Tt + PS_ROWS - 1) / PS_ROWS;
        const size_t lds = posstack_lds_bytes(cg, c.PK);
        RSAF_CHECK_ARG((int64_t)n * tiles <= 0x7fffffffLL, "too many row tiles");
        RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)posstack_conv_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((posstack_conv_kernel<NT>), dim3((unsigned)(n * tiles), (unsigned)c.PG), dim3(256), lds, s,
                           reinterpret_cast<const unsigned short*>(planes_at(W.xg)), rows * Hd,
                           reinterpret_cast<const unsigned short*>(planes_at(i ? W.wp_stack[i - 1] : W.wp_pos)), (int64_t)Hd * c.PK * cg, Hd,
                           i ? nullptr : ws + W.pos_scale, f16x2_scale_for_bound(sqrtf((float)Hd)), ws + (i ? W.ws_stack[i - 1] : W.ws_pos),
                           Wt + (i ? L.stackb[i - 1] : L.posb), Tw + (int64_t)6 * n, row0, ws + W.y, c.PK, tiles, posstack_rows_alloc(c.PK));
        RSAF_CHECK_HIP(hipGetLastError());
        return RSAF_OK;
    }
    int posstack_mfma(int D) {
        RSAF_TRY(posstack_rows<0>(x, nullptr));
        for (int i = 0; i < D; ++i) {
            switch (Hd / c.PG / 16) {
                case 1: RSAF_TRY(posstack_conv_launch<1>(i)); break;
                case 2: RSAF_TRY(posstack_conv_launch<2>(i)); break;
                case 3: RSAF_TRY(posstack_conv_launch<3>(i)); break;
                default: RSAF_TRY(posstack_conv_launch<4>(i)); break;
            }
            RSAF_TRY(i + 1 < D ? posstack_rows<1>(ws + W.y, nullptr) : posstack_rows<2>(ws + W.y, ws + W.y));
        }
        return RSAF_OK;
    }
    // other group widths (test geometries): regroup + the exact-fp32 GEMM per run of equal windows, rows normalised in place
    int posstack_fp32(int D) {
        const int cg = Hd / c.PG;
        for (int i = 0; i < D; ++i) {
            for (const auto& tg : R.tgroups) {
                const int nw = tg.second - tg.first, Tq = R.T6[tg.first], TTq = Tq + c.PK - 1;
                const int64_t r0 = R.row0[tg.first];
                const int64_t t4 = (int64_t)nw * TTq * (Hd / 4);
                hipLaunchKernelGGL(regroup_kernel, dim3((unsigned)std::min<int64_t>((t4 + 255) / 256, 4096)), dim3(256), 0, s,
                                   reinterpret_cast<const float4*>((i ? ws + W.y : x) + r0 * Hd), reinterpret_cast<float4*>(ws + W.xg),
                                   nw, Tq, Hd / 4, c.PG, c.PK);
                RSAF_CHECK_HIP(hipGetLastError());
                GemmParams p = gemm_params_plain(ws + W.xg, Wt + (i ? L.stackw[i - 1] : L.posw), ws + W.y + r0 * Hd, Tq, cg, c.PK * cg, cg,
                                                 (int64_t)c.PK * cg, Hd);
                p.nz = nw * c.PG; p.nz2 = c.PG;
                p.sA1 = (int64_t)c.PG * TTq * cg; p.sA2 = (int64_t)TTq * cg;
                p.sB1 = 0; p.sB2 = (int64_t)cg * c.PK * cg;
                p.sC1 = (int64_t)Tq * Hd; p.sC2 = cg;
                p.bias = Wt + (i ? L.stackb[i - 1] : L.posb); p.sBias2 = cg; p.act = ACT_NONE;
                RSAF_TRY(launch_gemm_f32(p, s, "w2v2_posstack_gemm_f32"));
            }
            RSAF_TRY(posstack_rows<2>(ws + W.y, ws + W.y));
        }
        return RSAF_OK;
    }
    // the regrouped sequence as k16 panels of T_w + PK - 1 rows per (window, group): tap k = one row down
    int posconv_regroup_planes() {
        const int TT = Tt + c.PK - 1;
        const int64_t tot4 = (int64_t)n * TT * (Hd / 4);
        ProfScope prof("w2v2_regroup", s, 0.0, (double)tot4 * 32);
        hipLaunchKernelGGL(regroup_planes_kernel, dim3((unsigned)std::min<int64_t>((tot4 + 255) / 256, 4096)), dim3(256),
                           0, s, reinterpret_cast<const float4*>(ws + W.x), reinterpret_cast<unsigned short*>(planes_at(W.xg)),
                           (int64_t)n * TT * Hd, n, Tt, Hd / 4, c.PG, c.PK, Tw + (int64_t)6 * n, row0, bits_at(W.fp_amax), ws + W.pos_scale);
        RSAF_CHECK_HIP(hipGetLastError());
        return RSAF_OK;
    }
    template <int NT, int SP>
    int posconv_lds_launch() {
        const int cg = Hd / c.PG, TT = Tt + c.PK - 1;
        const size_t lds = posconv_lds_bytes(cg, c.PK, SP);
        RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)posconv_f16x3_kernel<NT, SP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((posconv_f16x3_kernel<NT, SP>), dim3((unsigned)(n * c.PG)), dim3(512), lds, s,
                           reinterpret_cast<const unsigned short*>(planes_at(W.xg)), (int64_t)n * TT * Hd,
                           reinterpret_cast<const unsigned short*>(planes_at(W.wp_pos)), (int64_t)Hd * c.PK * cg, Hd,
                           ws + W.pos_scale, ws + W.ws_pos, Wt + L.posb, Tw + (int64_t)6 * n, row0, ws + W.y, c.PG, TT, c.PK,
                           posconv_rows_alloc(SP, c.PK));
        RSAF_CHECK_HIP(hipGetLastError());
        return RSAF_OK;
    }
    template <int SP>
    int posconv_lds_launch_nt() {
        switch (Hd / c.PG / 16) {
            case 1: return posconv_lds_launch<1, SP>();
            case 2: return posconv_lds_launch<2, SP>();
            case 3: return posconv_lds_launch<3, SP>();
            default: return posconv_lds_launch<4, SP>();
        }
    }
    // the window's image stays in LDS (posconv_f16x3_kernel); RSAF_W2V2_POSCONV_GEMM=1: the batched GEMM below (A/B)
    int posconv_lds() {
        const int cg = Hd / c.PG;
        ProfScope prof("w2v2_posconv_gemm", s, 2.0 * (double)rows * cg * (double)c.PK * cg * c.PG, 0.0);
        return posconv_split(Tt) == 2 ? posconv_lds_launch_nt<2>() : posconv_lds_launch_nt<1>();
    }
    // grouped conv as a two-level batched GEMM on the f16x3 kernel's 256 x 64 tile: batch (window, group), M = T_w rows,
    // N = cg output channels, K = PK cg
    int posconv_batched_gemm() {
        const int cg = Hd / c.PG, TT = Tt + c.PK - 1;
        GemmH3Params p{};
        p.A = planes_at(W.xg); p.a_plane = (int64_t)n * TT * Hd; p.lda = 16; p.sA = (int64_t)c.PG * TT * cg; p.sA2 = (int64_t)TT * cg;
        p.a_panel = 1; p.a_panel_rows = TT; p.a_tap_panels = cg / 16;
        p.a_scale = ws + W.pos_scale; p.a_scale_zs = 1; p.a_scale_ms = 0;
        p.B = planes_at(W.wp_pos); p.b_plane = (int64_t)Hd * c.PK * cg; p.ldb = 16; p.b_panel = 1; p.b_panel_rows = Hd; p.sB2 = (int64_t)cg * 16;
        p.b_scale = ws + W.ws_pos;
        p.C = ws + W.y; p.ldc = Hd; p.sC = 0; p.sC2 = cg;
        p.bias = Wt + L.posb; p.sBias2 = cg;
        p.M = Tt; p.ztab = ztab + (int64_t)6 * n * 2; p.N = cg; p.K = c.PK * cg; p.nz = n * c.PG; p.nz2 = c.PG; p.act = ACT_GELU; p.alpha = 1.0f;
        return launch_gemm_f16x3(p, s, "w2v2_posconv_gemm");
    }
    // group widths that are no multiple of 16 (test geometries): exact-fp32 GEMM, one launch per run of equal windows
    int posconv_fp32() {
        const int cg = Hd / c.PG;
        for (const auto& tg : R.tgroups) {
            const int nw = tg.second - tg.first, Tq = R.T6[tg.first], TTq = Tq + c.PK - 1;
            const int64_t r0 = R.row0[tg.first];
            const int64_t t4 = (int64_t)nw * TTq * (Hd / 4);
            {
                ProfScope prof("w2v2_regroup", s, 0.0, (double)t4 * 32);
                hipLaunchKernelGGL(regroup_kernel, dim3((unsigned)std::min<int64_t>((t4 + 255) / 256, 4096)), dim3(256),
                                   0, s, reinterpret_cast<const float4*>(ws + W.x + r0 * Hd), reinterpret_cast<float4*>(ws + W.xg),
                                   nw, Tq, Hd / 4, c.PG, c.PK);
                RSAF_CHECK_HIP(hipGetLastError());
            }
            GemmParams p = gemm_params_plain(ws + W.xg, Wt + L.posw, ws + W.y + r0 * Hd, Tq, cg, c.PK * cg, cg, (int64_t)c.PK * cg, Hd);
            p.nz = nw * c.PG; p.nz2 = c.PG;
            p.sA1 = (int64_t)c.PG * TTq * cg; p.sA2 = (int64_t)TTq * cg;
            p.sB1 = 0; p.sB2 = (int64_t)cg * c.PK * cg;
            p.sC1 = (int64_t)Tq * Hd; p.sC2 = cg;
            p.bias = Wt + L.posb; p.sBias2 = cg; p.act = ACT_GELU;
            RSAF_TRY(launch_gemm_f32(p, s, "w2v2_posconv_gemm"));
        }
        return RSAF_OK;
    }

    // The LayerNorm between two q/k/v projections: LN(src (+ res)) under g / b, fp32 rows into dst (x, the att buffer for the
    // gates, the call's `out`, or none), hidden_states[k] into its tap.
    // next: layer k follows and reads the planes in W.xp under the scales in W.s_x (fused attention: this LayerNorm also reports
    // the window's largest row norm, behind the scale of that layer's q / k / v).  Else dst is `out`: frame t of window w at
    // row out_row_start[w] + t (or packed, window after window).
    // The tap takes this LayerNorm's output, except in the PRE_LN flow while a layer follows: there hidden_states[k] is the
    // un-normalised residual stream h that this LayerNorm reads.  sum (PRE_LN after the positional conv): src + res goes there.
    int ln_to_qkv(const float* src, const float* res, const float* g, const float* b, float* dst, int k, bool next,
                  float* sum = nullptr) {
        LnArgs a;
        a.x = src; a.r = res; a.g = g; a.b = b;
        a.out = dst; a.rowwin = rowwin; a.row0 = row0;
        if (next) {
            if (fused) RSAF_CHECK_HIP(hipMemsetAsync(ws + W.win_norm, 0, sizeof(unsigned) * n, s));
            a.planes = planes_at(W.xp); a.panel = true; a.scale_out = ws + W.s_x;
            a.win_norm = fused ? bits_at(W.win_norm) : nullptr;
        } else {
            a.out_row_start = out_row_start;
        }
        a.var = sum ? 1 : 0; a.aux = sum;
        a.tap = tap(k); a.tap_mode = (pre_ln && next) ? 2 : 1; a.tap_row_start = out_row_start;
        return ln(a, rows, Hd, c.eps, s);
    }

    // fused q,k,v projection of layer l (A = the planes the previous LayerNorm wrote beside x).  Fused attention: the output
    // leaves as the fp16 plane pair the attention kernel multiplies, under one power of two per window (the bound over its
    // rows).  REL_POS_BIAS: then the bias gates of the layer
    int qkv_projection(int l) {
        const int b0 = WSTAT_LAYER0 + WSTAT_PER_LAYER * l;
        Out o;
        o.bias = Wt + L.layers[l].bqkv;
        if (fused) {
            hipLaunchKernelGGL(qkv_scale_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, bits_at(W.win_norm), rowwin, rows,
                               wstat(b0), wstat(b0 + 5), ws + W.s_qkv);
            RSAF_CHECK_HIP(hipGetLastError());
            o.Cp = planes_at(W.qkv); o.c_plane = rows * 3 * Hd; o.c_scale = ws + W.s_qkv; o.cs_zs = 0; o.cs_ms = 1;
        } else {
            o.Cf = ws + W.qkv;
        }
        const int rc = gemm3(rows_a(W.xp, Hd, ws + W.s_x), weights_b(W.wp_qkv[l], W.ws_qkv[l]), o, (int)rows, 3 * Hd, Hd);
        if (rc || !relpos) return rc;
        const int64_t items = rows * c.NH;
        RSAF_CHECK_ARG((items + 15) / 16 <= 0x7fffffffLL, "too many rows");
        ProfScope prof("w2v2_relpos_gate", s, 0.0, (double)rows * Hd * 4 + (double)items * 4);
        hipLaunchKernelGGL(relpos_gate_kernel, dim3((unsigned)((items + 15) / 16)), dim3(256), 2 * hd * sizeof(float), s,
                           pre_ln ? ws + W.att : x, items, c.NH, hd, Wt + L.ga[l], Wt + L.gb[l], Wt + L.gbias[l], Wt + L.gconst[l], gate());
        RSAF_CHECK_HIP(hipGetLastError());
        return RSAF_OK;
    }

    // attention of a layer: the planes of its output in W.attp (scales: W.s_qkv fused, W.s_att three-launch)
    int attention() { return fused ? (relpos ? attention_fused<true>() : attention_fused<false>()) : attention_three_launch(); }
    template <bool RP>
    int attention_fused() {
        // 2 x 2 T^2 hd flops per (chunk, head)
        double att_flops = 0.0;
        for (const auto& tg : R.tgroups) att_flops += 4.0 * (tg.second - tg.first) * c.NH * (double)R.T6[tg.first] * R.T6[tg.first] * hd;
        ProfScope prof("w2v2_attn_fused", s, att_flops, 0.0);
        RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)attn_f16x3_kernel<RP>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 2 * 128 * 64 * 2));
        hipLaunchKernelGGL(attn_f16x3_kernel<RP>, dim3((unsigned)(n * c.NH), (unsigned)((Tt + 127) / 128)), dim3(256), 2 * 2 * 128 * 64 * 2, s,
                           planes_at(W.qkv), rows * 3 * Hd, planes_at(W.attp), rows * Hd, rows, Tw + (int64_t)6 * n, row0, c.NH, Hd, scale,
                           ws + W.s_qkv, gate(), reltab());
        RSAF_CHECK_HIP(hipGetLastError());
        return RSAF_OK;
    }
    // three launches per run of equal windows (head widths other than 64: test geometries), then the planes of the result
    // (the fused kernel writes them itself)
    int attention_three_launch() {
        for (const auto& tg : R.tgroups) {
            const int nw = tg.second - tg.first, Tq = R.T6[tg.first], Tpq = (int)pad4(Tq);
            const int64_t r0 = R.row0[tg.first];
            const float* qkvg = ws + W.qkv + r0 * 3 * Hd;
            {   // S = scale * Q K^T per (chunk, head)
                GemmParams p = gemm_params_plain(qkvg, qkvg + Hd, ws + W.S, Tq, Tq, hd, 3 * Hd, 3 * Hd, Tpq);
                p.nz = nw * c.NH; p.nz2 = c.NH;
                p.sA1 = (int64_t)Tq * 3 * Hd; p.sA2 = hd; p.sB1 = p.sA1; p.sB2 = hd;
                p.sC1 = (int64_t)c.NH * Tq * Tpq; p.sC2 = (int64_t)Tq * Tpq;
                p.alpha = scale;
                RSAF_TRY(launch_gemm_f32(p, s, "w2v2_attn_gemm"));
            }
            {
                const int64_t srows = (int64_t)nw * c.NH * Tq;
                ProfScope prof("w2v2_softmax", s, 0.0, (double)srows * Tpq * 8);
#define RSAF_SOFTMAX(...)                                                                                                      \
    hipLaunchKernelGGL((softmax_kernel<__VA_ARGS__>), dim3((unsigned)((srows + 3) / 4)), dim3(256), 0, s, ws + W.S, srows, Tq, Tpq, \
                       gate(), reltab(), c.NH, r0)
                if (Tpq <= 256) { if (relpos) RSAF_SOFTMAX(true, true); else RSAF_SOFTMAX(true); }
                else { if (relpos) RSAF_SOFTMAX(false, true); else RSAF_SOFTMAX(false); }
#undef RSAF_SOFTMAX
                RSAF_CHECK_HIP(hipGetLastError());
            }
            {   // O = P V per (chunk, head), V is [T, hd] with N contiguous
                GemmParams p = gemm_params_plain(ws + W.S, qkvg + 2 * Hd, ws + W.att + r0 * Hd, Tq, hd, Tq, Tpq, 3 * Hd, Hd);
                p.nz = nw * c.NH; p.nz2 = c.NH; p.b_kn = 1;
                p.sA1 = (int64_t)c.NH * Tq * Tpq; p.sA2 = (int64_t)Tq * Tpq;
                p.sB1 = (int64_t)Tq * 3 * Hd; p.sB2 = hd;
                p.sC1 = (int64_t)Tq * Hd; p.sC2 = hd;
                RSAF_TRY(launch_gemm_f32(p, s, "w2v2_attn_gemm"));
            }
        }
        RSAF_TRY(launch_f16x2_row_scales(ws + W.att, rows, Hd, Hd, ws + W.s_att, nullptr, nullptr, s));
        return launch_split_f16x2(ws + W.att, rows, Hd, Hd, ws + W.s_att, 1, planes_at(W.attp), rows * Hd, 1, s);
    }

    // y = attn Wo^T + bo + x
    int out_projection(int l) {
        Out o;
        o.Cf = ws + W.y; o.bias = Wt + L.layers[l].bo; o.R = x;
        return gemm3(rows_a(W.attp, Hd, fused ? ws + W.s_qkv : ws + W.s_att), weights_b(W.wp_o[l], W.ws_o[l]), o, (int)rows, Hd, Hd);
    }
    // LN(y) under g / b as the planes the feed forward reads, with the bound behind the scale of the ffn1 output; fp32 rows
    // into dst (or none)
    int ln_to_ffn(int l, const float* g, const float* b, float* dst) {
        const int b0 = WSTAT_LAYER0 + WSTAT_PER_LAYER * l;
        LnArgs a;
        a.x = ws + W.y; a.g = g; a.b = b; a.out = dst;
        a.planes = planes_at(W.xp); a.panel = true; a.scale_out = ws + W.s_x;
        a.bound_w = wstat(b0 + 2); a.bound_b = wstat(b0 + 4); a.bound_scale_out = ws + W.s_ffn;
        return ln(a, rows, Hd, c.eps, s);
    }
    // dst = GELU(xp W1^T + b1) W2^T + b2 + res; the GELU output only exists as planes (A of the second GEMM)
    int feed_forward(int l, float* dst, const float* res) {
        const LayerOff& lo = L.layers[l];
        Out o1;
        o1.Cp = planes_at(W.ffnp); o1.c_plane = rows * c.I; o1.c_scale = ws + W.s_ffn; o1.cs_zs = 0; o1.cs_ms = 1; o1.cp_panel = true;
        o1.bias = Wt + lo.b1; o1.act = ACT_GELU;
        RSAF_TRY(gemm3(rows_a(W.xp, Hd, ws + W.s_x), weights_b(W.wp_1[l], W.ws_1[l]), o1, (int)rows, c.I, Hd));
        Out o2;
        o2.Cf = dst; o2.bias = Wt + lo.b2; o2.R = res;
        return gemm3(rows_a(W.ffnp, c.I, ws + W.s_ffn), weights_b(W.wp_2[l], W.ws_2[l]), o2, (int)rows, Hd, c.I);
    }

    // 6. encoder layer l.  Post-LN: y = attn + x, x = LN1(y), y = ffn(x) + x, x = LN2(y): hidden_states[l + 1], which after the
    //    last layer goes into `out`
    int layer_post_ln(int l) {
        const LayerOff& lo = L.layers[l];
        const bool last = l == c.L - 1;
        RSAF_TRY(out_projection(l));
        RSAF_TRY(ln_to_ffn(l, Wt + lo.ln1g, Wt + lo.ln1b, x));
        RSAF_TRY(feed_forward(l, ws + W.y, x));
        return ln_to_qkv(ws + W.y, nullptr, Wt + lo.ln2g, Wt + lo.ln2b, last ? out : x, l + 1, !last);
    }
    //    PRE_LN (stable layer norm): the residual stream h ping-pongs between x and y: y = attn(LN1(x)) + x, x = ffn(LN2(y)) + y,
    //    and the LayerNorms write planes only: LN1 of the next layer (hidden_states[l + 1] = h), or encoder.layer_norm into `out`
    //    after the last one (= hidden_states[L])
    int layer_pre_ln(int l) {
        const LayerOff& lo = L.layers[l];
        RSAF_TRY(out_projection(l));
        RSAF_TRY(ln_to_ffn(l, Wt + lo.ln2g, Wt + lo.ln2b, nullptr));
        RSAF_TRY(feed_forward(l, x, ws + W.y));
        if (l == c.L - 1) return ln_to_qkv(x, nullptr, Wt + L.elng, Wt + L.elnb, out, l + 1, false);
        const LayerOff& nx = L.layers[l + 1];
        return ln_to_qkv(x, nullptr, Wt + nx.ln1g, Wt + nx.ln1b, gate_rows(), l + 1, true);
    }
    int encoder_layer(int l) {
        RSAF_TRY(qkv_projection(l));
        RSAF_TRY(attention());
        return pre_ln ? layer_pre_ln(l) : layer_post_ln(l);
    }
};

static int forward_impl(const float* wav, const int64_t* chunk_start, const int* len_dev_or_null, const Rag& R, const Cfg& c,
                        const float* weights, void* workspace, int64_t workspace_bytes, float* out, const int64_t* out_row_start,
                        hipStream_t s, float* const* taps = nullptr) {
    RSAF_CHECK_ARG(R.n <= 65535 / std::max(c.NH, c.PG), "too many chunks per call");
    RSAF_CHECK_ARG(wav && chunk_start && weights && workspace && out, "NULL pointer");
    const Workspace W = make_ws(c, R);
    if (workspace_bytes < W.total * (int64_t)sizeof(float)) {
        set_error("rsaf_w2v2_forward: workspace too small");
        return RSAF_ERR_WORKSPACE;
    }
    RSAF_CHECK_ARG(R.rows <= 0x7fffffffLL, "too many frames per call");
    Forward f(c, R, W, weights, workspace, s);
    f.wav = wav; f.chunk_start = chunk_start; f.out = out; f.out_row_start = out_row_start; f.taps = taps;
    RSAF_TRY(f.window_tables(len_dev_or_null));
    RSAF_TRY(f.weight_planes());
    RSAF_TRY(f.feature_encoder());
    RSAF_TRY(f.feature_projection());
    RSAF_TRY(c.pos_depth() ? f.positional_conv_stack() : f.positional_conv());
    for (int l = 0; l < c.L; ++l)
        RSAF_TRY(f.encoder_layer(l));
    return RSAF_OK;
}

// Cfg of an entry point's geometry arguments, checked
static int make_cfg(Cfg& c, int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel, int pos_groups,
                    float eps, int flags) {
    c = Cfg{conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, eps, flags};
    return check_cfg(c);
}

}  // namespace w2v2
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::w2v2;

extern "C" {

int rsaf_w2v2_frames(int chunk_len) {
    int T[7];
    chunk_lengths(chunk_len, T);
    return T[6];
}

int64_t rsaf_w2v2_weight_floats(int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                                int pos_groups) {
    return rsaf_w2v2_weight_floats_ex(conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, 0);
}

int64_t rsaf_w2v2_weight_floats_ex(int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                                   int pos_groups, int flags) {
    Cfg c;
    if (make_cfg(c, conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, 1e-5f, flags) != RSAF_OK) return -1;
    return make_layout(c).total;
}

int rsaf_w2v2_weight_offsets(int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                             int pos_groups, int64_t* offsets_host, int cap, int* n_host) {
    return rsaf_w2v2_weight_offsets_ex(conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, 0, offsets_host,
                                       cap, n_host);
}

int rsaf_w2v2_weight_offsets_ex(int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                                int pos_groups, int flags, int64_t* offsets_host, int cap, int* n_host) {
    Cfg c;
    RSAF_TRY(make_cfg(c, conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, 1e-5f, flags));
    RSAF_CHECK_ARG(offsets_host && n_host, "NULL output");
    const Layout L = make_layout(c);
    std::vector<int64_t> v = {L.conv0, L.gng, L.gnb};
    for (int i = 0; i < 6; ++i) v.push_back(L.conv[i]);
    for (int64_t o : {L.fplg, L.fplb, L.fpw, L.fpb, L.posw, L.posb, L.elng, L.elnb}) v.push_back(o);
    for (const LayerOff& lo : L.layers)
        for (int64_t o : {lo.wqkv, lo.bqkv, lo.wo, lo.bo, lo.ln1g, lo.ln1b, lo.w1, lo.b1, lo.w2, lo.b2, lo.ln2g, lo.ln2b})
            v.push_back(o);
    // appended segments, one offset per C-float row: conv biases 0..6, then {gamma, beta} of the conv LayerNorms 0..6
    if (L.cb >= 0) for (int i = 0; i < 7; ++i) v.push_back(L.cb + (int64_t)i * c.C);
    if (L.cln >= 0) for (int i = 0; i < 14; ++i) v.push_back(L.cln + (int64_t)i * c.C);
    // REL_POS_BIAS: per layer {ga, gb, {ba, bb}, gru_rel_pos_const}, then the distance table
    if (L.reltab >= 0) {
        for (int l = 0; l < c.L; ++l)
            for (int64_t o : {L.ga[l], L.gb[l], L.gbias[l], L.gconst[l]}) v.push_back(o);
        v.push_back(L.reltab);
    }
    // POS_CONV_STACK: {kernel, bias} of the stack's layers 1..D-1
    for (size_t i = 0; i < L.stackw.size(); ++i) { v.push_back(L.stackw[i]); v.push_back(L.stackb[i]); }
    RSAF_CHECK_ARG(cap >= (int)v.size(), "offsets_host too small");
    for (size_t i = 0; i < v.size(); ++i) offsets_host[i] = v[i];
    *n_host = (int)v.size();
    return RSAF_OK;
}

int64_t rsaf_w2v2_workspace_bytes(int n_chunks, int chunk_len, int conv_dim, int hidden, int layers, int heads,
                                  int intermediate, int pos_kernel, int pos_groups) {
    const std::vector<int> len((size_t)std::max(n_chunks, 1), chunk_len);
    return rsaf_w2v2_workspace_bytes_ragged_ex(len.data(), n_chunks, conv_dim, hidden, layers, heads, intermediate, pos_kernel,
                                               pos_groups, 0);
}

int64_t rsaf_w2v2_workspace_bytes_ragged(const int* chunk_len_host, int n_chunks, int conv_dim, int hidden, int layers, int heads,
                                         int intermediate, int pos_kernel, int pos_groups) {
    return rsaf_w2v2_workspace_bytes_ragged_ex(chunk_len_host, n_chunks, conv_dim, hidden, layers, heads, intermediate, pos_kernel,
                                               pos_groups, 0);
}

int64_t rsaf_w2v2_workspace_bytes_ragged_ex(const int* chunk_len_host, int n_chunks, int conv_dim, int hidden, int layers, int heads,
                                            int intermediate, int pos_kernel, int pos_groups, int flags) {
    Cfg c;
    if (make_cfg(c, conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, 1e-5f, flags) != RSAF_OK || n_chunks <= 0 ||
        !chunk_len_host) return -1;
    Rag R;
    if (make_rag(chunk_len_host, n_chunks, 0, R) != RSAF_OK) return -1;
    return make_ws(c, R).total * (int64_t)sizeof(float);
}

int rsaf_w2v2_forward(const float* wav, const int64_t* chunk_start, int n_chunks, int chunk_len, int conv_dim,
                      int hidden, int layers, int heads, int intermediate, int pos_kernel, int pos_groups,
                      float layer_norm_eps, const float* weights, void* workspace, int64_t workspace_bytes,
                      float* out, const int64_t* out_row_start, rsaf_stream_t stream) {
    Cfg c;
    RSAF_TRY(make_cfg(c, conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, layer_norm_eps, 0));
    RSAF_CHECK_ARG(n_chunks >= 0, "negative chunk count");
    if (n_chunks == 0) return RSAF_OK;
    Rag R;
    RSAF_TRY(make_rag(nullptr, n_chunks, chunk_len, R));
    return forward_impl(wav, chunk_start, nullptr, R, c, weights, workspace, workspace_bytes, out, out_row_start, (hipStream_t)stream);
}

int rsaf_w2v2_forward_ragged(const float* wav, const int64_t* chunk_start, const int* chunk_len, const int* chunk_len_host,
                             int n_chunks, int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                             int pos_groups, float layer_norm_eps, const float* weights, void* workspace,
                             int64_t workspace_bytes, float* out, const int64_t* out_row_start, rsaf_stream_t stream) {
    return rsaf_w2v2_forward_ragged_ex(wav, chunk_start, chunk_len, chunk_len_host, n_chunks, conv_dim, hidden, layers, heads,
                                       intermediate, pos_kernel, pos_groups, layer_norm_eps, 0, weights, workspace, workspace_bytes,
                                       out, out_row_start, stream);
}

int rsaf_w2v2_forward_ragged_ex(const float* wav, const int64_t* chunk_start, const int* chunk_len, const int* chunk_len_host,
                                int n_chunks, int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                                int pos_groups, float layer_norm_eps, int flags, const float* weights, void* workspace,
                                int64_t workspace_bytes, float* out, const int64_t* out_row_start, rsaf_stream_t stream) {
    Cfg c;
    RSAF_TRY(make_cfg(c, conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, layer_norm_eps, flags));
    RSAF_CHECK_ARG(n_chunks >= 0, "negative chunk count");
    if (n_chunks == 0) return RSAF_OK;
    RSAF_CHECK_ARG(chunk_len && chunk_len_host, "NULL length table");
    Rag R;
    RSAF_TRY(make_rag(chunk_len_host, n_chunks, 0, R));
    return forward_impl(wav, chunk_start, chunk_len, R, c, weights, workspace, workspace_bytes, out, out_row_start, (hipStream_t)stream);
}

int rsaf_w2v2_forward_ragged_hidden(const float* wav, const int64_t* chunk_start, const int* chunk_len, const int* chunk_len_host,
                                    int n_chunks, int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                                    int pos_groups, float layer_norm_eps, int flags, const float* weights, void* workspace,
                                    int64_t workspace_bytes, float* out, const int64_t* out_row_start, const int* hidden_index_host,
                                    int n_hidden, float* hidden_out, int64_t hidden_plane_floats, rsaf_stream_t stream) {
    Cfg c;
    RSAF_TRY(make_cfg(c, conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, layer_norm_eps, flags));
    // the taps are checked on the host before anything else: strictly increasing layer indices in [0, layers]
    RSAF_CHECK_ARG(n_hidden >= 0 && n_hidden <= layers + 1, "n_hidden out of range");
    if (n_hidden == 0)
        return rsaf_w2v2_forward_ragged_ex(wav, chunk_start, chunk_len, chunk_len_host, n_chunks, conv_dim, hidden, layers, heads,
                                           intermediate, pos_kernel, pos_groups, layer_norm_eps, flags, weights, workspace,
                                           workspace_bytes, out, out_row_start, stream);
    RSAF_CHECK_ARG(hidden_index_host && hidden_out, "NULL hidden-state index list or output");
    for (int j = 0; j < n_hidden; ++j) {
        RSAF_CHECK_ARG(hidden_index_host[j] >= 0 && hidden_index_host[j] <= layers, "hidden-state index outside [0, layers]");
        RSAF_CHECK_ARG(j == 0 || hidden_index_host[j] > hidden_index_host[j - 1], "hidden-state indices not strictly increasing");
    }
    RSAF_CHECK_ARG(hidden_plane_floats >= 0 && hidden_plane_floats % 4 == 0 && (reinterpret_cast<uintptr_t>(hidden_out) & 15) == 0,
                   "hidden-state planes must be 16-byte aligned");
    RSAF_CHECK_ARG(n_chunks >= 0, "negative chunk count");
    if (n_chunks == 0) return RSAF_OK;
    RSAF_CHECK_ARG(chunk_len && chunk_len_host, "NULL length table");
    Rag R;
    RSAF_TRY(make_rag(chunk_len_host, n_chunks, 0, R));
    RSAF_CHECK_ARG(hidden_plane_floats >= R.rows * (int64_t)hidden, "hidden_plane_floats smaller than the call's frames");
    std::vector<float*> taps((size_t)layers + 1, nullptr);
    for (int j = 0; j < n_hidden; ++j) taps[hidden_index_host[j]] = hidden_out + (int64_t)j * hidden_plane_floats;
    return forward_impl(wav, chunk_start, chunk_len, R, c, weights, workspace, workspace_bytes, out, out_row_start, (hipStream_t)stream,
                        taps.data());
}

}  // extern "C"
