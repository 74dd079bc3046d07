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
//               (data2vec-audio, RSAF_W2V2_POS_CONV_STACK: a stack of convolution + LayerNorm + GELU layers, w2v2_posconv.hip)
//   attention : S = QK^T/sqrt(d) and O = PV as (chunk, head)-batched GEMMs on the packed qkv buffer
// conv0 (Cin = 1) + GroupNorm + GELU is recomputed in two passes (stats, apply) instead of
// materialising the un-normalised 15 999 x 512 activation; LayerNorm / softmax are one wave per row.
// Files: w2v2_layout.h (layouts and path predicates, plain C++), w2v2_forward.h (Forward: one call, one member function per
// phase), w2v2_feat.hip, w2v2_posconv.hip, w2v2_encoder.hip (each stage's kernels with the phases that launch them); this
// file keeps the GEMM operands, the weight planes, the order of the phases and the entry points.
#include "w2v2_forward.h"

namespace rsaf {
namespace w2v2 {

int Forward::gemm3(const GemmA& A, const GemmB& B, const Out& o, int M, int N, int K, int nz, const int64_t* zt) {
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
GemmA Forward::rows_a(int64_t planes_off, int K, const float* row_scale) const {
    GemmA A;
    A.planes = planes_at(planes_off); A.plane = rows * K; A.lda = K; A.scale = row_scale; A.scale_ms = 1; A.panel = true;
    return A;
}
// A of conv i: the channels-last output of layer i - 1, one batch and one scale per window; tap k of a frame = a row shift
GemmA Forward::conv_a(const uint16_t* planes, int i) const {
    GemmA A;
    A.planes = planes; A.plane = (int64_t)G * T[i - 1] * C; A.lda = (int64_t)STRD[i] * C; A.sA = (int64_t)T[i - 1] * C;
    A.scale = cscale + (int64_t)(i - 1) * G; A.scale_zs = 1;
    return A;
}
// A of conv i over the packed row space: row R of the GEMM starts at plane row 2 R; the scale comes by the row's window slot
GemmA Forward::conv_a_packed(const uint16_t* planes, int64_t plane, int i) const {
    GemmA A;
    A.planes = planes; A.plane = plane; A.lda = (int64_t)STRD[i] * C;
    A.scale = cscale + (int64_t)(i - 1) * G;
    return A;
}
GemmB Forward::weights_b(int64_t planes_off, int64_t scale_off) const { return GemmB{planes_at(planes_off), ws + scale_off}; }

int Forward::split_wp(int64_t src_off, int64_t nrows, int K, int64_t dst_off, int64_t scale_off, int stat_idx) {
    RSAF_TRY(launch_f16x2_row_scales(Wt + src_off, nrows, K, K, ws + scale_off, nullptr, wstat(stat_idx), s));
    return launch_split_f16x2(Wt + src_off, nrows, K, K, ws + scale_off, 1, planes_at(dst_off), nrows * K, 1, s);
}
// 0. weights of the dense layers as fp16 plane pairs in the k16-panel layout, each row with its own power-of-two scale
//    (once per call: 0.4 GB at base geometry, < 1 ms), and per matrix the largest row norm: the Cauchy-Schwarz factor of
//    the bound behind the scale of a GEMM's PLANE output (conv1..5, ffn1)
int Forward::weight_planes() {
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

// a verdict of w2v2_layout.h (the failed condition's message, or NULL) as the error of `fn`, the function that checked it
static int arg_error(const char* fn, const char* msg) {
    if (!msg) return RSAF_OK;
    set_error(std::string(fn) + ": " + msg);
    return RSAF_ERR_ARG;
}

// Cfg of an entry point's geometry arguments, checked
static int make_cfg(Cfg& c, int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel, int pos_groups,
                    float eps, int flags) {
    c = Cfg{conv_dim, hidden, layers, heads, intermediate, pos_kernel, pos_groups, eps, flags};
    return arg_error("check_cfg", check_cfg(c));
}

// A ragged call.  Windows of one regime (w2v2_layout.h: window_regime): one forward, as ever.  Windows that span regimes: one
// forward per regime run on that run's sub-list, one after the other in the caller's workspace on the caller's stream, so
// every window takes the kernels, and returns the bits, of a call of its own.  The tables advance by the run's first
// window; packed output (out_row_start NULL) and its taps advance by the rows already written.
static int forward_runs(const float* wav, const int64_t* chunk_start, const int* len_dev, const int* len_host, const Rag& R, const Cfg& c,
                        const float* weights, void* workspace, int64_t workspace_bytes, float* out, const int64_t* out_row_start,
                        hipStream_t s, float* const* taps = nullptr) {
    const std::vector<std::pair<int, int>> runs = regime_runs(c, R);
    if (runs.size() == 1)
        return forward_impl(wav, chunk_start, len_dev, R, c, weights, workspace, workspace_bytes, out, out_row_start, s, taps);
    RSAF_CHECK_ARG(wav && chunk_start && weights && workspace && out, "NULL pointer");
    if (workspace_bytes < make_ws(c, R).total * (int64_t)sizeof(float)) {      // the size published for the call covers every run
        set_error("rsaf_w2v2_forward: workspace too small");
        return RSAF_ERR_WORKSPACE;
    }
    std::vector<float*> run_taps((size_t)c.L + 1, nullptr);
    for (const auto& run : runs) {
        const int b = run.first;
        Rag Rr;
        RSAF_TRY(arg_error("make_rag", make_rag(len_host + b, run.second - b, 0, Rr)));
        const int64_t skip = out_row_start ? 0 : R.row0[b] * (int64_t)c.Hd;
        if (taps)
            for (int k = 0; k <= c.L; ++k) run_taps[k] = taps[k] ? taps[k] + skip : nullptr;
        RSAF_TRY(forward_impl(wav, chunk_start + b, len_dev + b, Rr, c, weights, workspace, workspace_bytes, out + skip,
                              out_row_start ? out_row_start + b : nullptr, s, taps ? run_taps.data() : nullptr));
    }
    return RSAF_OK;
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
    if (arg_error("make_rag", make_rag(chunk_len_host, n_chunks, 0, R)) != RSAF_OK) return -1;
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
    RSAF_TRY(arg_error("make_rag", make_rag(nullptr, n_chunks, chunk_len, R)));
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
    RSAF_TRY(arg_error("make_rag", make_rag(chunk_len_host, n_chunks, 0, R)));
    return forward_runs(wav, chunk_start, chunk_len, chunk_len_host, R, c, weights, workspace, workspace_bytes, out, out_row_start,
                        (hipStream_t)stream);
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
    RSAF_TRY(arg_error("make_rag", make_rag(chunk_len_host, n_chunks, 0, R)));
    RSAF_CHECK_ARG(hidden_plane_floats >= R.rows * (int64_t)hidden, "hidden_plane_floats smaller than the call's frames");
    std::vector<float*> taps((size_t)layers + 1, nullptr);
    for (int j = 0; j < n_hidden; ++j) taps[hidden_index_host[j]] = hidden_out + (int64_t)j * hidden_plane_floats;
    return forward_runs(wav, chunk_start, chunk_len, chunk_len_host, R, c, weights, workspace, workspace_bytes, out, out_row_start,
                        (hipStream_t)stream, taps.data());
}

}  // extern "C"