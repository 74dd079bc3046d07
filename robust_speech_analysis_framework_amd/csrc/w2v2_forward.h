// What the stage files of the Wav2Vec2 forward share: one forward call as a struct (Forward) whose member functions are its
// phases, the named operands of its launches, and the plane split of a value.  A phase is defined next to the kernels it
// launches: w2v2_feat.hip (window tables, feature encoder, feature projection), w2v2_posconv.hip (positional convolution
// and stack), w2v2_encoder.hip (LayerNorm, attention, encoder layers); w2v2.hip has the GEMM operands, the weight planes,
// the order of the phases and the entry points.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "gemm_f32.h"
#include "gemm_f16x3.h"
#include "w2v2_layout.h"

namespace rsaf {
namespace w2v2 {

__device__ __forceinline__ unsigned short f16_bits_w(_Float16 h) { return __builtin_bit_cast(unsigned short, h); }
// xs = hi + lo (+ 2^-22 |xs|): the two fp16 planes of a value that already carries its power-of-two scale (gemm_f16x3.hip)
__device__ __forceinline__ void split2_w(float xs, unsigned short& h, unsigned short& l) {
    const _Float16 hh = (_Float16)xs;
    h = f16_bits_w(hh);
    l = f16_bits_w((_Float16)(xs - (float)hh));
}

// a step of a sequence that ends at the first error
#define RSAF_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

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

int ln(const LnArgs& a, int64_t rows, int D, float eps, hipStream_t s);

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
    // regime: what the frame-count predicates pick at the longest window (w2v2_layout.h); the entry points hand Forward windows
    // of one regime only.
    const Regime regime;
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
          regime(window_regime(c_, Tt)), fused(regime.fused), relpos(c_.flags & F_REL_POS_BIAS), pre_ln(c_.flags & F_PRE_LN),
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

    // the phases, each defined beside the kernels it launches.  w2v2.hip: GEMM operands and the weight planes
    int gemm3(const GemmA& A, const GemmB& B, const Out& o, int M, int N, int K, int nz = 1, const int64_t* zt = nullptr);
    GemmA rows_a(int64_t planes_off, int K, const float* row_scale) const, conv_a(const uint16_t* planes, int i) const,
        conv_a_packed(const uint16_t* planes, int64_t plane, int i) const;
    GemmB weights_b(int64_t planes_off, int64_t scale_off) const;
    int split_wp(int64_t src_off, int64_t nrows, int K, int64_t dst_off, int64_t scale_off, int stat_idx), weight_planes();
    // w2v2_feat.hip
    int window_tables(const int* len_dev), feature_encoder(), conv_gemm(int i, const uint16_t* a_planes, Out& o, int g0, int g, const int* Tg),
        convs_layer_norm(int g0, int g, const int* Tg), convs_group_norm(int g0, int g, const int* Tg), feature_projection();
    // w2v2_posconv.hip
    int positional_conv(), positional_conv_stack(), posstack_mfma(int D), posstack_fp32(int D), posconv_regroup_planes(), posconv_lds(),
        posconv_batched_gemm(),
        conv_runs_fp32(const float* src, const float* w, const float* bias, int act, const char* gemm_family, const char* regroup_family);
    template <int MODE> int posstack_rows(const float* src, float* dst);
    template <int NT> int posstack_conv_launch(int i);
    template <int NT, int SP> int posconv_lds_launch();
    // w2v2_encoder.hip
    int ln_to_qkv(const float* src, const float* res, const float* g, const float* b, float* dst, int k, bool next, float* sum = nullptr);
    int qkv_projection(int l), attention(), attention_three_launch(), out_projection(int l),
        ln_to_ffn(int l, const float* g, const float* b, float* dst), feed_forward(int l, float* dst, const float* res), layer_post_ln(int l),
        layer_pre_ln(int l), encoder_layer(int l);
    template <bool RP> int attention_fused();
};

}  // namespace w2v2
}  // namespace rsaf
