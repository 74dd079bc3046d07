// CNN-LSTM-with-attention classifier forward for gfx950 (reference: CNNLSTM.forward,
// src/models.py:161-193, eval mode; harness behaviours of src/dl_cv_strategies.py:81-84 apply:
// zero-padded frames are NOT masked anywhere).
//
//   x[B,T,D] (read in its native layout: the permute of :172 costs nothing)
//   -> res_block1: act(conv3+BN) -> conv3+BN (+ conv1x1+BN shortcut) -> act     (fp32 MFMA GEMMs,
//      BN folded into the weights at load time, k=3 padding handled in the A-tile loader)
//   -> max_pool1d(2) -> res_block2 (identity shortcut)
//   -> 2-layer bidirectional LSTM: input projections for all time steps as one GEMM per layer
//      (N = 8H: both directions), then a persistent recurrent kernel (cnnlstm_lstm.hip)
//   -> attention pooling (online softmax over time) + dropout(identity) + Linear -> logits[B,2]
//
// This file: the CNN front (exact fp32, and the fp16-split path with its split / scale kernels), the attention head, the
// phases of a forward (Fwd, run_forward) and the entry points.  The weight blob and the workspace are laid out in
// cnnlstm_layout.h.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "cnnlstm_host.h"
#include "cnnlstm_kernels.h"
#include "gemm_f32.h"
#include "gemm_f16x3.h"

namespace rsaf {
namespace cnnlstm {

// ---- max_pool1d(kernel_size=2) over time, channels-last ----------------------------------------
__global__ __launch_bounds__(256) void pool2_kernel(const float4* __restrict__ x, float4* __restrict__ y,
                                                    int B, int T, int Tp, int C4) {
    const int64_t n = (int64_t)B * Tp * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C4);
        const int64_t bt = i / C4;
        const int t = (int)(bt % Tp);
        const int64_t b = bt / Tp;
        const float4 a = x[(b * T + 2 * t) * C4 + c];
        const float4 d = x[(b * T + 2 * t + 1) * C4 + c];
        y[i] = make_float4(fmaxf(a.x, d.x), fmaxf(a.y, d.y), fmaxf(a.z, d.z), fmaxf(a.w, d.w));
    }
}

// ---- attention pooling (softmax over time) + final Linear -----------------------------------------
// The body is shared by the one-batch kernel and the group kernel below: `b` (the batch row) is what blockIdx.x is to both.
template <int NF>   // features per lane: 2H = 64*NF
__device__ __forceinline__ void attnpool_fc_body(const float* __restrict__ seq, const float* __restrict__ watt,
                                                 const float* __restrict__ batt, const float* __restrict__ wfc,
                                                 const float* __restrict__ bfc, float* __restrict__ logits,
                                                 float* __restrict__ pooled_out, int T, int NC, int b) {
    constexpr int F = 64 * NF;
    __shared__ float s_m[4], s_l[4], s_ctx[4][F], s_red[4][16];
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const float* sb = seq + (int64_t)b * T * F;
    float wa[NF], ctx[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) { wa[i] = watt[lane + 64 * i]; ctx[i] = 0.f; }
    const float ba = batt[0];
    float m = -INFINITY, l = 0.f;
    for (int t = w; t < T; t += 4) {
        float v[NF];
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < NF; ++i) { v[i] = sb[(int64_t)t * F + lane + 64 * i]; d += v[i] * wa[i]; }
        const float sc = wave_sum(d) + ba;
        const float mn = fmaxf(m, sc);
        const float a = expf(m - mn);
        const float p = expf(sc - mn);
        l = l * a + p;
#pragma unroll
        for (int i = 0; i < NF; ++i) ctx[i] = ctx[i] * a + p * v[i];
        m = mn;
    }
    if (lane == 0) { s_m[w] = m; s_l[w] = l; }
#pragma unroll
    for (int i = 0; i < NF; ++i) s_ctx[w][lane + 64 * i] = ctx[i];
    __syncthreads();
    const float M = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    float Lt = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) Lt += s_l[k] * expf(s_m[k] - M);
    // thread f (< F) owns pooled feature f
    float pooled = 0.f;
    const int f = threadIdx.x;
    if (f < F) {
#pragma unroll
        for (int k = 0; k < 4; ++k) pooled += s_ctx[k][f] * expf(s_m[k] - M);
        pooled /= Lt;
        if (pooled_out) pooled_out[(int64_t)b * F + f] = pooled;
    }
    if (!wfc) return;                                  // pooling only (AttentionPooling.forward, src/models.py:94-107)
    for (int c = 0; c < NC; ++c) {
        float part = (f < F) ? pooled * wfc[(int64_t)c * F + f] : 0.f;
        part = wave_sum(part);
        if (lane == 0) s_red[w][c] = part;
    }
    __syncthreads();
    if (threadIdx.x < NC)
        logits[(int64_t)b * NC + threadIdx.x] =
            s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x] +
            bfc[threadIdx.x];
}

template <int NF>
__global__ __launch_bounds__(256) void attnpool_fc_kernel(const float* __restrict__ seq, const float* __restrict__ watt,
                                                          const float* __restrict__ batt, const float* __restrict__ wfc,
                                                          const float* __restrict__ bfc, float* __restrict__ logits,
                                                          float* __restrict__ pooled_out, int T, int NC) {
    attnpool_fc_body<NF>(seq, watt, batt, wfc, bfc, logits, pooled_out, T, NC, blockIdx.x);
}

// The heads of several independent forwards (same H and NC; own sequences, own weights, own B and T) in one launch: grid
// (max B, K), blockIdx.y selects the descriptor, which travels by value in the kernel arguments like the recurrences' above.
// A workgroup whose row lies beyond its item's batch leaves before it touches LDS or a barrier.
template <int NF>
__global__ __launch_bounds__(256) void attnpool_fc_group_kernel(const AttnPoolGroup g, int NC) {
    const AttnPoolItem& it = g.item[blockIdx.y];
    if ((int)blockIdx.x >= it.B) return;
    attnpool_fc_body<NF>(it.seq, it.watt, it.batt, it.wfc, it.bfc, it.logits, it.pooled_out, it.T, NC, blockIdx.x);
}

// The same for heads of different H (AttnPoolMixedItem): the features per lane are the item's.  Both exits are taken by the
// whole workgroup.
__global__ __launch_bounds__(256) void attnpool_fc_group_mixed_kernel(const AttnPoolMixedGroup g, int NC) {
    const AttnPoolMixedItem& m = g.item[blockIdx.y];
    const AttnPoolItem& it = m.head;
    if ((int)blockIdx.x >= it.B) return;
    if (m.H == 128) attnpool_fc_body<4>(it.seq, it.watt, it.batt, it.wfc, it.bfc, it.logits, it.pooled_out, it.T, NC, blockIdx.x);
    else attnpool_fc_body<2>(it.seq, it.watt, it.batt, it.wfc, it.bfc, it.logits, it.pooled_out, it.T, NC, blockIdx.x);
}

}  // namespace cnnlstm

void launch_pool2(const float* x, float* y, int B, int T, int Tp, int C, int blocks, hipStream_t s) {
    hipLaunchKernelGGL(cnnlstm::pool2_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<float4*>(y), B, T, Tp, C / 4);
}

int conv3(const float* x, const float* wk, const float* bias, const float* R, int64_t ldr, int64_t sR, float* y, int B, int T,
          int Cin, int Cout, int act, hipStream_t s, const char* tag) {
    GemmParams p = gemm_params_plain(x - Cin, wk, y, T, Cout, 3 * Cin, Cin, 3 * Cin, Cout);
    p.bias = bias; p.R = R; p.ldr = ldr; p.sR1 = sR;
    p.nz = B; p.nz2 = 1; p.sA1 = (int64_t)T * Cin; p.sC1 = (int64_t)T * Cout;
    p.a_pad_k = Cin; p.act = act;
    return launch_gemm_f32(p, s, tag);
}

namespace cnnlstm {

static int tap_copy(float* dst, const float* src, int64_t n, hipStream_t s) {
    if (dst) RSAF_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return RSAF_OK;
}

// ---- the same forward with the convolutions and the LSTM input projections on the fp16-split GEMM (gemm_f16x3.hip) -------
// Every GEMM operand is a pair of fp16 planes under a power-of-two scale.  A k = 3 / pad = 1 convolution reads three
// consecutive rows of a sequence, so its A operand is stored with one zero row in front of and behind every sequence
// ([B][T + 2][C]: the convolution is then a plain GEMM with lda = C, K = 3 C over the padded rows) and carries ONE scale per
// sequence: the input's exact maximum, or for a convolution's own output the bound sqrt(K) max|a| max_n |w_n|_2 + max|b|
// (+ max |residual|) with max|a| the largest |input| that the producing epilogue reported.
__device__ __forceinline__ void split2_c(float xs, unsigned short& h, unsigned short& l) {
    const _Float16 hh = (_Float16)xs;
    h = __builtin_bit_cast(unsigned short, hh);
    l = __builtin_bit_cast(unsigned short, (_Float16)(xs - (float)hh));
}

// largest |x| of every sequence (bit pattern of the float: non-negative floats order like unsigned integers)
__global__ __launch_bounds__(256) void seq_absmax_kernel(const float4* __restrict__ x, int64_t n4_per_seq, int chunks,
                                                         unsigned* __restrict__ amax) {
    const int z = blockIdx.y;
    const float4* p = x + (int64_t)z * n4_per_seq;
    float m = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4_per_seq; i += (int64_t)chunks * 256) {
        const float4 v = p[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    m = wave_max_nonneg(m);
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(amax + z, __float_as_uint(m));
}

// scale[z] = the power of two for bound_z = amax_in[z] * factor_host * wstat[0] + bstat[1] (+ amax_res[z]); a NULL wstat = 1
__global__ __launch_bounds__(256) void cnn_scale_kernel(const unsigned* __restrict__ amax_in, const unsigned* __restrict__ amax_res,
                                                        const unsigned* __restrict__ wstat, const unsigned* __restrict__ bstat,
                                                        float factor_host, float* __restrict__ scale, int n) {
    const int z = blockIdx.x * 256 + threadIdx.x;
    if (z >= n) return;
    float b = __uint_as_float(amax_in[z]) * factor_host * (wstat ? __uint_as_float(wstat[0]) * 1.000001f : 1.0f);
    if (bstat) b += __uint_as_float(bstat[1]);
    if (amax_res) b += __uint_as_float(amax_res[z]);
    scale[z] = f16x2_scale_for_bound(b * 1.000001f);
}

// fp32 [B][T][C] -> plane pair [B][T + 2][C] (zero rows around every sequence), times scale[z]; POOL: the rows are first
// max-pooled in pairs (src is [B][2 T (+1)][C]) and the pooled fp32 rows are kept as well (the residual of res_block2)
template <bool POOL>
__global__ __launch_bounds__(256) void split_padded_kernel(const float4* __restrict__ src, int B, int T, int Tsrc, int C4,
                                                           const float* __restrict__ scale, unsigned short* __restrict__ planes,
                                                           int64_t plane, float4* __restrict__ pooled) {
    const int64_t n = (int64_t)B * (T + 2) * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C4);
        const int64_t bt = i / C4;
        const int tp = (int)(bt % (T + 2));
        const int64_t b = bt / (T + 2);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tp >= 1 && tp <= T) {
            const int t = tp - 1;
            if (POOL) {
                const float4 a = src[(b * Tsrc + 2 * t) * C4 + c], d = src[(b * Tsrc + 2 * t + 1) * C4 + c];
                v = make_float4(fmaxf(a.x, d.x), fmaxf(a.y, d.y), fmaxf(a.z, d.z), fmaxf(a.w, d.w));
                pooled[(b * T + t) * C4 + c] = v;
            } else {
                v = src[(b * Tsrc + t) * C4 + c];
            }
        }
        const float sc = scale[b];
        unsigned short hh[4], ll[4];
        split2_c(v.x * sc, hh[0], ll[0]); split2_c(v.y * sc, hh[1], ll[1]);
        split2_c(v.z * sc, hh[2], ll[2]); split2_c(v.w * sc, hh[3], ll[3]);
        unsigned short* pp = planes + 4 * i;
        *reinterpret_cast<uint2*>(pp) = make_uint2(hh[0] | ((unsigned)hh[1] << 16), hh[2] | ((unsigned)hh[3] << 16));
        *reinterpret_cast<uint2*>(pp + plane) = make_uint2(ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16));
    }
}

// fp32 [B][T][C] -> plane pair of the zero-padded sequences in k16 panels: [C / 16][B (T + 2)][16], times scale[z].  One
// wave moves 16 rows x 64 channels: a lane reads 16 channels of a row (64 bytes) and writes 32 bytes per plane; the 16 rows
// of a panel are 512 contiguous bytes.  The image is the A operand of BOTH the 3-tap convolution (a_tap_panels = C / 16:
// tap k of output row t is image row t + k) and the 1x1 shortcut (the centre rows).
__global__ __launch_bounds__(256) void split_padded_panels_kernel(const float4* __restrict__ src, int B, int T, int C,
                                                                  const float* __restrict__ scale, unsigned short* __restrict__ planes,
                                                                  int64_t plane) {
    const int64_t R = (int64_t)B * (T + 2);
    const int cgroups = C / 64;                                          // 64-channel groups per row (C % 64 == 0)
    const int64_t tiles = ((R + 15) / 16) * cgroups;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wv; tile < tiles; tile += (int64_t)gridDim.x * 4) {
        const int cg = (int)(tile % cgroups);
        const int64_t r = (tile / cgroups) * 16 + (lane >> 2);
        if (r >= R) continue;
        const int c0 = cg * 64 + (lane & 3) * 16;
        const int64_t b = r / (T + 2);
        const int tp = (int)(r - b * (T + 2));
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tp >= 1 && tp <= T) {
            const float4* q = src + ((b * T + (tp - 1)) * C + c0) / 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = q[u];
        }
        const float sc = scale[b];
        unsigned hw[8], lw[8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            unsigned short hh[4], ll[4];
            split2_c(v[u].x * sc, hh[0], ll[0]); split2_c(v[u].y * sc, hh[1], ll[1]);
            split2_c(v[u].z * sc, hh[2], ll[2]); split2_c(v[u].w * sc, hh[3], ll[3]);
            hw[2 * u] = hh[0] | ((unsigned)hh[1] << 16); hw[2 * u + 1] = hh[2] | ((unsigned)hh[3] << 16);
            lw[2 * u] = ll[0] | ((unsigned)ll[1] << 16); lw[2 * u + 1] = ll[2] | ((unsigned)ll[3] << 16);
        }
        unsigned short* pp = planes + ((int64_t)(c0 / 16) * R + r) * 16;
        *reinterpret_cast<uint4*>(pp) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        *reinterpret_cast<uint4*>(pp + 8) = make_uint4(hw[4], hw[5], hw[6], hw[7]);
        *reinterpret_cast<uint4*>(pp + plane) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
        *reinterpret_cast<uint4*>(pp + plane + 8) = make_uint4(lw[4], lw[5], lw[6], lw[7]);
    }
}

// fp32 [B][n4 float4] -> plane pair of the same shape, times scale[b]
__global__ __launch_bounds__(256) void split_rows_kernel(const float4* __restrict__ src, int B, int64_t n4_per_seq,
                                                         const float* __restrict__ scale, unsigned short* __restrict__ planes, int64_t plane) {
    const int64_t n = (int64_t)B * n4_per_seq;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float4 v = src[i];
        const float sc = scale[i / n4_per_seq];
        unsigned short hh[4], ll[4];
        split2_c(v.x * sc, hh[0], ll[0]); split2_c(v.y * sc, hh[1], ll[1]);
        split2_c(v.z * sc, hh[2], ll[2]); split2_c(v.w * sc, hh[3], ll[3]);
        unsigned short* pp = planes + 4 * i;
        *reinterpret_cast<uint2*>(pp) = make_uint2(hh[0] | ((unsigned)hh[1] << 16), hh[2] | ((unsigned)hh[3] << 16));
        *reinterpret_cast<uint2*>(pp + plane) = make_uint2(ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16));
    }
}

// zero the pad rows (first and last of every sequence) of a plane pair [B][T + 2][C] that a GEMM epilogue fills
__global__ __launch_bounds__(256) void zero_pad_rows_kernel(unsigned short* __restrict__ planes, int64_t plane, int B, int T, int C8) {
    const int64_t n = (int64_t)B * 2 * C8 * 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C8);
        int64_t r = i / C8;
        const int pl = (int)(r & 1); r >>= 1;
        const int which = (int)(r & 1);
        const int64_t b = r >> 1;
        const int64_t row = b * (T + 2) + (which ? T + 1 : 0);
        *reinterpret_cast<uint4*>(planes + pl * plane + (row * C8 + c) * 8) = make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---- one forward, cut at its recurrences into phases -------------------------------------------------------------------
//   prep_weights (f16x3 path: the weights as plane pairs, once per distinct blob) | front (CNN + layer-0 input projection)
//   | per layer: recurrence, inproj of the next layer | head.
// The single entries run the phases of their one forward with the one-batch launchers; the group entry runs every phase for
// all items, one grouped recurrence launch per layer in between and one grouped head.  Per item these are the same kernels
// with the same launch parameters in the same order, so the logits are those of K single calls, bit for bit.
struct Fwd {
    Dims d; Layout L;               // the item's own architecture (one for all items, except in a mixed group)
    const float* x; int B, T;
    const float* W;
    float* logits;
    float *res1_out, *res2_out, *lstm_out, *pooled_out;     // stage taps (rsaf_cnnlstm_forward_stages), else NULL
    float *bufA, *bufB, *bufC, *xproj, *seq0, *seq1;        // fp32 buffers of the workspace (InferWs)
    int64_t ws_floats;                                      // what the forward uses of it
    // f16x3 path: own activation planes, amax and scale | the weight planes, row scales, statistics and `one`, which live
    // in this item's workspace (prep) or in that of the first item of the group that carries the same `weights`
    bool f16, prep;
    float* f16base; F16Ws F;
    float* wbase; F16Ws WF;
    const float* lin;               // input of the next LSTM layer
    float* lout;                    // output buffer of the next recurrence
};

static uint16_t* planes_at(float* base, int64_t off) { return reinterpret_cast<uint16_t*>(base + off); }

// argument checks of one forward (idx < 0: the single entries, whose messages carry no item) and its buffers; `short_code`:
// what a workspace below the item's need returns
static int check_item(const Dims& d, const float* x, int B, int T, const float* weights, void* workspace, int64_t workspace_bytes,
                      float* logits, const char* who, int idx, Fwd* f, int short_code = RSAF_ERR_WORKSPACE) {
    if (!(B >= 1 && B <= 65535)) return fail(RSAF_ERR_ARG, who, idx, "batch must be in [1, 65535]");
    if (!(T >= 2)) return fail(RSAF_ERR_ARG, who, idx, "sequence length must be >= 2 (max_pool1d(2) of the reference needs it)");
    if (!((int64_t)B * (T / 2) <= 0x7fffffffLL)) return fail(RSAF_ERR_ARG, who, idx, "B*T too large");
    if (!(x && weights && workspace && logits)) return fail(RSAF_ERR_ARG, who, idx, "NULL pointer");
    const InferWs w = make_infer_ws(d, B, T);
    if (workspace_bytes < w.total * (int64_t)sizeof(float)) return fail(short_code, who, idx, short_code == RSAF_ERR_WORKSPACE ? "workspace too small" : "workspace too small for this item's architecture");
    *f = Fwd{};
    f->d = d; f->L = make_layout(d);
    f->x = x; f->B = B; f->T = T; f->W = weights; f->logits = logits;
    float* ws = static_cast<float*>(workspace);
    f->bufA = ws + w.bufA; f->bufB = ws + w.bufB; f->bufC = ws + w.bufC;
    f->xproj = ws + w.xproj; f->seq0 = ws + w.seq0; f->seq1 = ws + w.seq1;
    f->ws_floats = w.total;
    f->f16 = w.f16;
    if (f->f16) {
        f->f16base = ws + w.f16base;
        f->F = w.F;
        f->prep = true; f->wbase = f->f16base; f->WF = f->F;
    }
    return RSAF_OK;
}

// no two items of a group overlapping in what the forward writes, and items that share `weights` sharing an architecture
static int check_overlaps(const rsaf_cnnlstm_forward_item* items, const Fwd* fs, int K, const char* who) {
    for (int k = 1; k < K; ++k)
        for (int j = 0; j < k; ++j) {
            const rsaf_cnnlstm_forward_item &a = items[j], &b = items[k];
            const int NC = fs[k].d.NC;
            const char* what = overlap(static_cast<const float*>(a.workspace), fs[j].ws_floats, static_cast<const float*>(b.workspace),
                                       fs[k].ws_floats) ? "workspace"
                               : overlap(a.logits, (int64_t)a.B * NC, b.logits, (int64_t)b.B * NC) ? "logits" : nullptr;
            if (what) return fail(RSAF_ERR_ARG, who, k, std::string("shares `") + what + "` with item " + std::to_string(j));
            const Dims &p = fs[j].d, &q = fs[k].d;
            if (a.weights == b.weights && !(p.C == q.C && p.H == q.H && p.act == q.act))
                return fail(RSAF_ERR_ARG, who, k, "shares `weights` with item " + std::to_string(j) + " but not its architecture");
        }
    return RSAF_OK;
}

// weight preparation once per distinct blob: later items read the planes, scales and statistics of the first one
static void share_weight_prep(Fwd* fs, int K) {
    for (int k = 1; k < K; ++k)
        for (int j = 0; j < k; ++j)
            if (fs[k].f16 && fs[j].prep && fs[j].W == fs[k].W) {
                fs[k].prep = false; fs[k].wbase = fs[j].wbase; fs[k].WF = fs[j].WF;
                break;
            }
}

// weights -> plane pairs in k16 panels with their row scales; statistics {max row norm, max |element|} at the slots stat_w,
// stat_b and stat_wih of cnnlstm_layout.h.  A pure function of the blob.
static int prep_weights(const Fwd& f, const Dims& d, const Layout& L, hipStream_t s) {
    const int D = d.D, C = d.C, H = d.H;
    const float* W = f.W;
    const F16Ws& F = f.WF;
    float* base = f.wbase;
    unsigned* stat = reinterpret_cast<unsigned*>(base + F.stat);
    float* one = base + F.one;
    RSAF_CHECK_HIP(hipMemsetAsync(stat, 0, sizeof(unsigned) * 2 * CNN_NSTAT, s));
    const int64_t woff[5] = {L.w1, L.wsc, L.w2, L.w3, L.w4}, boff[5] = {L.b1, L.bsc, L.b2, L.b3, L.b4};
    const int wk[5] = {3 * D, D, 3 * C, 3 * C, 3 * C};
    for (int i = 0; i < 5; ++i) {
        if (woff[i] < 0) continue;                                          // no 1x1 shortcut when D == C
        TRY(launch_f16x2_row_scales(W + woff[i], C, wk[i], wk[i], base + F.ws[i], nullptr, stat + 2 * stat_w(i), s));
        TRY(launch_split_f16x2(W + woff[i], C, wk[i], wk[i], base + F.ws[i], 1, planes_at(base, F.wp[i]), (int64_t)C * wk[i], 1, s));
        TRY(launch_f16x2_row_scales(W + boff[i], 1, C, C, one, nullptr, stat + 2 * stat_b(i), s));
    }
    for (int l = 0; l < d.L; ++l) {
        const int in = l == 0 ? C : 2 * H;
        TRY(launch_f16x2_row_scales(W + L.wih[l], 8 * H, in, in, base + F.wih_s[l], nullptr, stat + 2 * stat_wih(l), s));
        TRY(launch_split_f16x2(W + L.wih[l], 8 * H, in, in, base + F.wih_s[l], 1, planes_at(base, F.wih_p[l]), (int64_t)8 * H * in, 1, s));
    }
    RSAF_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(one), 0x46800000, 1, s));   // 16384.0f: |h| < 1 for every LSTM output
    return RSAF_OK;
}

// input projection of layer l for all time steps, into xproj
static int inproj(Fwd& f, const Dims& d, const Layout& L, int l, hipStream_t s) {
    const int B = f.B, C = d.C, H = d.H, Tp = f.T / 2;
    const int in = l == 0 ? C : 2 * H;
    const int64_t rows = (int64_t)B * Tp;
    if (!f.f16) {
        GemmParams p = gemm_params_plain(f.lin, f.W + L.wih[l], f.xproj, (int)rows, 8 * H, in, in, in, 8 * H);
        p.bias = f.W + L.bih[l];
        return launch_gemm_f32(p, s, "lstm_inproj_gemm");
    }
    // layer 0 reads conv4's planes (one scale per sequence), the layers behind it the plane pair of the previous layer's
    // output under the fixed scale 2^14
    float* one = f.wbase + f.WF.one;
    GemmH3Params p{};
    p.B = planes_at(f.wbase, f.WF.wih_p[l]); p.b_plane = (int64_t)8 * H * in; p.ldb = 16; p.b_panel = 1; p.b_scale = f.wbase + f.WF.wih_s[l];
    p.C = f.xproj; p.ldc = 8 * H; p.bias = f.W + L.bih[l]; p.N = 8 * H; p.K = in; p.act = ACT_NONE; p.alpha = 1.0f;
    if (l == 0) {
        p.A = planes_at(f.f16base, f.F.c4p); p.a_plane = (int64_t)B * Tp * C; p.lda = C; p.sA = (int64_t)Tp * C;
        p.a_scale = f.f16base + f.F.scale + SC4 * B; p.a_scale_zs = 1; p.a_scale_ms = 0;
        p.M = Tp; p.nz = B; p.sC = (int64_t)Tp * 8 * H;
    } else {
        TRY(launch_split_f16x2(f.lin, rows, in, in, one, 0, planes_at(f.f16base, f.F.hp), rows * in, 1, s));
        p.A = planes_at(f.f16base, f.F.hp); p.a_plane = rows * in; p.lda = 16; p.a_panel = 1;
        p.a_scale = one; p.a_scale_zs = 0; p.a_scale_ms = 0;
        p.M = (int)rows; p.nz = 1;
    }
    return launch_gemm_f16x3(p, s, "lstm_inproj_gemm");
}

// one residual block with both convolutions on the exact-fp32 MFMA GEMM (src/models.py:64-76): h = act(conv3(x)) -> bufA,
// the 1x1 shortcut -> bufB (wsc == NULL: the identity, x itself), y = act(conv3(h) + shortcut)
static int resblock_f32(const float* x, int B, int T, int D, int C, int act, const float* w1, const float* b1, const float* wsc,
                        const float* bsc, const float* w2, const float* b2, float* bufA, float* bufB, float* y, hipStream_t s) {
    TRY(conv3(x, w1, b1, nullptr, 0, 0, bufA, B, T, D, C, act, s, "cnn_conv_gemm"));
    const float* sc = x;
    int64_t ldsc = D;
    if (wsc) {
        GemmParams p = gemm_params_plain(x, wsc, bufB, T, C, D, D, D, C);
        p.bias = bsc; p.nz = B; p.sA1 = (int64_t)T * D; p.sC1 = (int64_t)T * C;
        TRY(launch_gemm_f32(p, s, "cnn_conv_gemm"));
        sc = bufB; ldsc = C;
    }
    return conv3(bufA, w2, b2, sc, ldsc, (int64_t)T * ldsc, y, B, T, C, C, act, s, "cnn_conv_gemm");
}

// the two residual blocks on the exact-fp32 MFMA GEMM
static int front_f32(Fwd& f, const Dims& d, const Layout& L, hipStream_t s) {
    const int B = f.B, T = f.T, D = d.D, C = d.C, Tp = T / 2;
    const float* x = f.x;
    const float* W = f.W;
    float *bufA = f.bufA, *bufB = f.bufB, *bufC = f.bufC;
    // res_block1 (src/models.py:64-76, :175)
    TRY(resblock_f32(x, B, T, D, C, d.act, W + L.w1, W + L.b1, D != C ? W + L.wsc : nullptr, D != C ? W + L.bsc : nullptr, W + L.w2,
                     W + L.b2, bufA, bufB, bufC, s));
    TRY(tap_copy(f.res1_out, bufC, (int64_t)B * T * C, s));
    // max_pool1d(2) (:177)
    {
        const int64_t n4 = (int64_t)B * Tp * (C / 4);
        const int blocks = (int)std::min<int64_t>((n4 + 255) / 256, 256 * 16);
        ProfScope prof("cnn_pool2", s, 0.0, (double)B * T * C * 4 * 1.5);
        launch_pool2(bufC, bufA, B, T, Tp, C, blocks, s);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    // res_block2, identity shortcut (:178)
    TRY(conv3(bufA, W + L.w3, W + L.b3, nullptr, 0, 0, bufB, B, Tp, C, C, d.act, s, "cnn_conv_gemm"));
    TRY(conv3(bufB, W + L.w4, W + L.b4, bufA, C, (int64_t)Tp * C, bufC, B, Tp, C, C, d.act, s, "cnn_conv_gemm"));
    return tap_copy(f.res2_out, bufC, (int64_t)B * Tp * C, s);
}

// the same with the convolutions on the fp16-split GEMM, up to conv4's output as the plane pair of the first input projection
static int front_f16x3(Fwd& f, const Dims& d, const Layout& L, hipStream_t s) {
    const int B = f.B, T = f.T, D = d.D, C = d.C, Tp = T / 2;
    const float* x = f.x;
    const float* W = f.W;
    float *bufA = f.bufA, *bufB = f.bufB, *bufC = f.bufC;
    float* f16base = f.f16base;
    const F16Ws& F = f.F;
    const F16Ws& WF = f.WF;
    auto planes = [&](int64_t off) { return planes_at(f16base, off); };
    const unsigned* stat = reinterpret_cast<const unsigned*>(f.wbase + WF.stat);   // [CNN_NSTAT][2], slots stat_w / stat_b
    unsigned* amax = reinterpret_cast<unsigned*>(f16base + F.amax);
    float* scale = f16base + F.scale;
    RSAF_CHECK_HIP(hipMemsetAsync(amax, 0, sizeof(unsigned) * CNN_NAMAX * B, s));
    auto cnn_scale = [&](int a_in, int a_res, int w_slot, int b_slot, float factor, int s_out) {
        hipLaunchKernelGGL(cnn_scale_kernel, dim3((B + 255) / 256), dim3(256), 0, s, amax + (int64_t)a_in * B,
                           a_res >= 0 ? amax + (int64_t)a_res * B : nullptr, w_slot >= 0 ? stat + 2 * w_slot : nullptr,
                           b_slot >= 0 ? stat + 2 * b_slot : nullptr, factor, scale + (int64_t)s_out * B, B);
    };
    // one GEMM of the block: A = padded plane pair (row stride lda, Tr rows per sequence, first tap at a_row0), per-sequence scale
    // (a_panels > 0: A is a panel image of a_panels channel panels over all B (T + 2) padded rows, see split_padded_panels_kernel)
    int a_panels = 0;
    auto gemm = [&](const uint16_t* A, int64_t a_plane, int64_t a_seq_rows, int a_row0, int lda, int s_in, int widx, int M, int N, int K,
                    float* Cf, uint16_t* Cp, int64_t c_plane, int64_t cp_seq_rows, int cp_row0, int s_out, const float* bias,
                    const float* R, int act, int amax_slot, const char* tag) {
        GemmH3Params p{};
        p.A = A + (int64_t)a_row0 * lda; p.a_plane = a_plane; p.lda = lda; p.sA = a_seq_rows * lda;
        if (a_panels > 0) {
            p.A = A + (int64_t)a_row0 * 16; p.lda = 16; p.sA = a_seq_rows * 16;
            p.a_panel = 1; p.a_panel_rows = (int)((int64_t)B * a_seq_rows);
            p.a_tap_panels = K > a_panels * 16 ? a_panels : 0;
        }
        p.a_scale = scale + (int64_t)s_in * B; p.a_scale_zs = 1; p.a_scale_ms = 0;
        p.B = planes_at(f.wbase, WF.wp[widx]); p.b_plane = (int64_t)N * K; p.ldb = 16; p.b_panel = 1; p.b_scale = f.wbase + WF.ws[widx];
        p.C = Cf; p.ldc = N; p.sC = (int64_t)M * N;
        p.Cp = Cp ? Cp + (int64_t)cp_row0 * N : nullptr; p.c_plane = c_plane; p.ldcp = N; p.sCp = cp_seq_rows * N;
        p.c_scale = s_out >= 0 ? scale + (int64_t)s_out * B : nullptr; p.c_scale_zs = 1; p.c_scale_ms = 0;
        p.amax_out = amax_slot >= 0 ? amax + (int64_t)amax_slot * B : nullptr; p.amax_zs = 1;
        p.bias = bias; p.R = R; p.ldr = N; p.sR = (int64_t)M * N;
        p.M = M; p.N = N; p.K = K; p.nz = B; p.act = act; p.alpha = 1.0f;
        return launch_gemm_f16x3(p, s, tag);
    };
    const int64_t pl_x = (int64_t)B * (T + 2) * D, pl_c = (int64_t)B * (T + 2) * C, pl_p = (int64_t)B * (Tp + 2) * C;
    // x -> padded planes under the exact maximum of every sequence; in k16 panels when the width allows (D % 64 == 0, image
    // rows below 2^27): row-major rows reach the DMA as 32-byte pieces of 512 different rows per k-tile, and with one column
    // tile (N = 128) nothing hides that (RSAF_CNN_ROWMAJOR=1: the row-major image, the A/B reference)
    const bool no_panels = [] { const char* e = getenv("RSAF_CNN_ROWMAJOR"); return e && e[0] == '1'; }();   // per call: the tests toggle it
    const bool x_panels = !no_panels && D % 64 == 0 && (int64_t)B * (T + 2) < ((int64_t)1 << 27);
    {
        ProfScope prof("cnn_split_input", s, 0.0, (double)B * T * D * 12.0);
        const int64_t n4 = (int64_t)T * D / 4;
        const int chunks = (int)std::min<int64_t>((n4 + 255) / 256, 64);
        hipLaunchKernelGGL(seq_absmax_kernel, dim3(chunks, B), dim3(256), 0, s, reinterpret_cast<const float4*>(x), n4, chunks, amax + AX * B);
        cnn_scale(AX, -1, -1, -1, 1.0f, SX);
        const int64_t tot = (int64_t)B * (T + 2) * (D / 4);
        if (x_panels) {
            const int64_t tiles = (((int64_t)B * (T + 2) + 15) / 16) * (D / 64);
            hipLaunchKernelGGL(split_padded_panels_kernel, dim3((unsigned)std::min<int64_t>((tiles + 3) / 4, 16384)), dim3(256), 0, s,
                               reinterpret_cast<const float4*>(x), B, T, D, scale + SX * B, planes(F.xp), pl_x);
        } else {
            hipLaunchKernelGGL(split_padded_kernel<false>, dim3((unsigned)std::min<int64_t>((tot + 255) / 256, 8192)), dim3(256), 0, s,
                               reinterpret_cast<const float4*>(x), B, T, T, D / 4, scale + SX * B, planes(F.xp), pl_x, nullptr);
        }
        RSAF_CHECK_HIP(hipGetLastError());
    }
    // res_block1 (src/models.py:64-76, :175): conv1 -> planes, shortcut -> fp32, conv2 (+ shortcut) -> fp32
    cnn_scale(AX, -1, stat_w(W1), stat_b(W1), sqrtf((float)(3 * D)) * 1.00001f, SC1);
    hipLaunchKernelGGL(zero_pad_rows_kernel, dim3(64), dim3(256), 0, s, planes(F.c1p), pl_c, B, T, C / 8);
    a_panels = x_panels ? D / 16 : 0;
    TRY(gemm(planes(F.xp), pl_x, T + 2, 0, D, SX, W1, T, C, 3 * D, nullptr, planes(F.c1p), pl_c, T + 2, 1, SC1, W + L.b1, nullptr,
             d.act, AC1, "cnn_conv_gemm"));
    const float* sc = x;
    if (D != C) {
        TRY(gemm(planes(F.xp), pl_x, T + 2, 1, D, SX, WSC, T, C, D, bufB, nullptr, 0, 0, 0, -1, W + L.bsc, nullptr, ACT_NONE, ASC, "cnn_conv_gemm"));
        sc = bufB;
    }
    a_panels = 0;
    TRY(gemm(planes(F.c1p), pl_c, T + 2, 0, C, SC1, W2, T, C, 3 * C, bufC, nullptr, 0, 0, 0, -1, W + L.b2, sc, d.act, AC2, "cnn_conv_gemm"));
    TRY(tap_copy(f.res1_out, bufC, (int64_t)B * T * C, s));
    // max_pool1d(2) (:177): pooled fp32 rows (the residual of res_block2) + padded planes; max |pooled| <= max |conv2 output|
    cnn_scale(AC2, -1, -1, -1, 1.0f, SPOOL);
    {
        ProfScope prof("cnn_pool2", s, 0.0, (double)B * T * C * 4 * 2.0);
        const int64_t tot = (int64_t)B * (Tp + 2) * (C / 4);
        hipLaunchKernelGGL(split_padded_kernel<true>, dim3((unsigned)std::min<int64_t>((tot + 255) / 256, 8192)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(bufC), B, Tp, T, C / 4, scale + SPOOL * B, planes(F.poolp), pl_p,
                           reinterpret_cast<float4*>(bufA));
        RSAF_CHECK_HIP(hipGetLastError());
    }
    // res_block2, identity shortcut (:178)
    cnn_scale(AC2, -1, stat_w(W3), stat_b(W3), sqrtf((float)(3 * C)) * 1.00001f, SC3);
    hipLaunchKernelGGL(zero_pad_rows_kernel, dim3(64), dim3(256), 0, s, planes(F.c3p), pl_p, B, Tp, C / 8);
    TRY(gemm(planes(F.poolp), pl_p, Tp + 2, 0, C, SPOOL, W3, Tp, C, 3 * C, nullptr, planes(F.c3p), pl_p, Tp + 2, 1, SC3, W + L.b3, nullptr,
             d.act, AC3, "cnn_conv_gemm"));
    TRY(gemm(planes(F.c3p), pl_p, Tp + 2, 0, C, SC3, W4, Tp, C, 3 * C, bufC, nullptr, 0, 0, 0, -1, W + L.b4, bufA, d.act, AC4, "cnn_conv_gemm"));
    TRY(tap_copy(f.res2_out, bufC, (int64_t)B * Tp * C, s));
    // conv4's output as the plane pair of the first input projection, under the exact maximum of every sequence
    cnn_scale(AC4, -1, -1, -1, 1.0f, SC4);
    {
        const int64_t tot = (int64_t)B * Tp * (C / 4);
        hipLaunchKernelGGL(split_rows_kernel, dim3((unsigned)std::min<int64_t>((tot + 255) / 256, 8192)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(bufC), B, (int64_t)Tp * (C / 4), scale + SC4 * B, planes(F.c4p), (int64_t)B * Tp * C);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    return RSAF_OK;
}

// the CNN front up to and including the input projection of the first LSTM layer (:184)
static int front(Fwd& f, const Dims& d, const Layout& L, hipStream_t s) {
    TRY(f.f16 ? front_f16x3(f, d, L, s) : front_f32(f, d, L, s));
    f.lin = f.bufC;
    f.lout = f.seq0;
    return inproj(f, d, L, 0, s);
}

static LstmRecItem rec_item(const Fwd& f, const Dims& d, const Layout& L, int l) {
    return LstmRecItem{f.xproj, f.W + L.whh[l], f.lout, nullptr, nullptr, f.B, f.T / 2};
}

static AttnPoolItem head_item(const Fwd& f, const Layout& L) {
    return AttnPoolItem{f.lin, f.W + L.watt, f.W + L.batt, f.W + L.wfc, f.W + L.bfc, f.logits, f.pooled_out, f.B, f.T / 2};
}

static void launch_attnpool(const AttnPoolItem& it, int H, int NC, hipStream_t s) {      // wfc == NULL: pooling only
    if (H == 128)
        hipLaunchKernelGGL(attnpool_fc_kernel<4>, dim3(it.B), dim3(256), 0, s, it.seq, it.watt, it.batt, it.wfc, it.bfc, it.logits,
                           it.pooled_out, it.T, NC);
    else
        hipLaunchKernelGGL(attnpool_fc_kernel<2>, dim3(it.B), dim3(256), 0, s, it.seq, it.watt, it.batt, it.wfc, it.bfc, it.logits,
                           it.pooled_out, it.T, NC);
}

// attention pooling + fc (:187-191): one launch per forward (SINGLE), one for the heads of all of them (GROUPED: one
// architecture; MIXED: an architecture per item)
static int head(const Fwd* fs, int K, int mode, hipStream_t s) {
    const int NC = fs[0].d.NC;
    if (mode == SINGLE) {
        for (int k = 0; k < K; ++k) {
            const int H = fs[k].d.H;
            const AttnPoolItem it = head_item(fs[k], fs[k].L);
            ProfScope prof("attnpool_fc", s, 0.0, (double)it.B * it.T * 2 * H * 4);
            launch_attnpool(it, H, NC, s);
            RSAF_CHECK_HIP(hipGetLastError());
        }
        return RSAF_OK;
    }
    AttnPoolGroup g{};
    AttnPoolMixedGroup gm{};
    int rows = 0;
    double bytes = 0.0;
    for (int k = 0; k < K; ++k) {
        g.item[k] = head_item(fs[k], fs[k].L);
        gm.item[k] = AttnPoolMixedItem{g.item[k], fs[k].d.H};
        rows = std::max(rows, fs[k].B);
        bytes += (double)g.item[k].B * g.item[k].T * 2 * fs[k].d.H * 4;
    }
    ProfScope prof("attnpool_fc", s, 0.0, bytes);
    if (mode == MIXED) hipLaunchKernelGGL(attnpool_fc_group_mixed_kernel, dim3(rows, K), dim3(256), 0, s, gm, NC);
    else if (fs[0].d.H == 128) hipLaunchKernelGGL(attnpool_fc_group_kernel<4>, dim3(rows, K), dim3(256), 0, s, g, NC);
    else hipLaunchKernelGGL(attnpool_fc_group_kernel<2>, dim3(rows, K), dim3(256), 0, s, g, NC);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// GROUPED / MIXED: one launch per layer carries the recurrences of all items whose batch runs on the 4-row kernel (an item
// above lstm_small_max() has its recurrence launched on its own: launch_lstm_rec_layer), and one launch the heads; SINGLE:
// one launch per item.
// Every item carries its own dims and layout; only a MIXED call has items that differ in them (never in D, NC or L).
static int run_forward(Fwd* fs, int K, int mode, hipStream_t s) {
    const int layers = fs[0].d.L;
    for (int k = 0; k < K; ++k)
        if (fs[k].f16 && fs[k].prep) TRY(prep_weights(fs[k], fs[k].d, fs[k].L, s));
    for (int k = 0; k < K; ++k) TRY(front(fs[k], fs[k].d, fs[k].L, s));
    for (int l = 0; l < layers; ++l) {
        LstmRecMixedItem recs[RSAF_CNNLSTM_GROUP_MAX];
        for (int k = 0; k < K; ++k) recs[k] = LstmRecMixedItem{rec_item(fs[k], fs[k].d, fs[k].L, l), fs[k].d.H};
        TRY(launch_lstm_rec_layer(recs, K, mode, false, s));
        for (int k = 0; k < K; ++k) {
            Fwd& f = fs[k];
            f.lin = f.lout;
            f.lout = (f.lout == f.seq0) ? f.seq1 : f.seq0;
            if (l + 1 < layers) TRY(inproj(f, f.d, f.L, l + 1, s));
        }
    }
    for (int k = 0; k < K; ++k) TRY(tap_copy(fs[k].lstm_out, fs[k].lin, (int64_t)fs[k].B * (fs[k].T / 2) * 2 * fs[k].d.H, s));
    return head(fs, K, mode, s);
}

}  // namespace cnnlstm
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::cnnlstm;

extern "C" {

int64_t rsaf_cnnlstm_weight_floats(int input_dim, int channels, int hidden, int num_classes, int lstm_layers) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    if (check_dims(d, 0) != RSAF_OK) return -1;
    return make_layout(d).total;
}

int rsaf_cnnlstm_weight_offsets(int input_dim, int channels, int hidden, int num_classes, int lstm_layers,
                                int64_t* offsets_host, int cap, int* n_host) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    int rc = check_dims(d, 0);
    if (rc != RSAF_OK) return rc;
    RSAF_CHECK_ARG(offsets_host && n_host, "NULL output");
    const Layout L = make_layout(d);
    int64_t v[10 + 12 + 4];
    int n = 0;
    v[n++] = L.w1; v[n++] = L.b1; v[n++] = L.wsc; v[n++] = L.bsc; v[n++] = L.w2; v[n++] = L.b2;
    v[n++] = L.w3; v[n++] = L.b3; v[n++] = L.w4; v[n++] = L.b4;
    for (int l = 0; l < d.L; ++l) { v[n++] = L.wih[l]; v[n++] = L.bih[l]; v[n++] = L.whh[l]; }
    v[n++] = L.watt; v[n++] = L.batt; v[n++] = L.wfc; v[n++] = L.bfc;
    RSAF_CHECK_ARG(cap >= n, "offsets_host too small");
    for (int i = 0; i < n; ++i) offsets_host[i] = v[i];
    *n_host = n;
    return RSAF_OK;
}

int64_t rsaf_cnnlstm_workspace_bytes(int B, int T, int input_dim, int channels, int hidden, int lstm_layers) {
    if (B <= 0 || T < 2) return -1;
    const Dims d{input_dim, channels, hidden, 2, lstm_layers, ACT_SILU};
    return make_infer_ws(d, B, T).total * (int64_t)sizeof(float);
}

static int forward_single(const char* who, const float* x, int B, int T, int input_dim, int channels, int hidden, int num_classes,
                          int lstm_layers, int act, const float* weights, void* workspace, int64_t workspace_bytes, float* logits,
                          float* res1_out, float* res2_out, float* lstm_out, float* pooled_out, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, act};
    TRY(check_dims(d, 0));
    if (B == 0) return RSAF_OK;
    Fwd f;
    TRY(check_item(d, x, B, T, weights, workspace, workspace_bytes, logits, who, -1, &f));
    f.res1_out = res1_out; f.res2_out = res2_out; f.lstm_out = lstm_out; f.pooled_out = pooled_out;
    return run_forward(&f, 1, SINGLE, (hipStream_t)stream);
}

int rsaf_cnnlstm_forward(const float* x, int B, int T, int input_dim, int channels, int hidden, int num_classes,
                         int lstm_layers, int act, const float* weights, void* workspace,
                         int64_t workspace_bytes, float* logits, rsaf_stream_t stream) {
    return forward_single(__func__, x, B, T, input_dim, channels, hidden, num_classes, lstm_layers, act, weights, workspace,
                          workspace_bytes, logits, nullptr, nullptr, nullptr, nullptr, stream);
}

int rsaf_cnnlstm_forward_stages(const float* x, int B, int T, int input_dim, int channels, int hidden,
                                int num_classes, int lstm_layers, int act, const float* weights, void* workspace,
                                int64_t workspace_bytes, float* logits, float* res1_out, float* res2_out,
                                float* lstm_out, float* pooled_out, rsaf_stream_t stream) {
    return forward_single(__func__, x, B, T, input_dim, channels, hidden, num_classes, lstm_layers, act, weights, workspace,
                          workspace_bytes, logits, res1_out, res2_out, lstm_out, pooled_out, stream);
}

int rsaf_cnnlstm_forward_group(const rsaf_cnnlstm_forward_item* items_host, int K, int input_dim, int channels, int hidden,
                               int num_classes, int lstm_layers, int act, rsaf_stream_t stream) {
    const char* who = __func__;
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, act};
    Fwd fs[RSAF_CNNLSTM_GROUP_MAX];
    TRY(check_group_args(K, items_host, who, "RSAF_CNNLSTM_GROUP_MAX"));
    // widths the layouts cannot be computed for are refused here; the full check of the dims follows the item checks (it is
    // the same for every item, and the item checks name the item)
    if (!(input_dim > 0 && channels > 0 && hidden > 0 && lstm_layers >= 1 && lstm_layers <= 4)) return check_dims(d, 0);
    for (int k = 0; k < K; ++k) {
        const rsaf_cnnlstm_forward_item& it = items_host[k];
        TRY(check_item(d, it.x, it.B, it.T, it.weights, it.workspace, it.workspace_bytes, it.logits, who, k, &fs[k]));
    }
    TRY(check_overlaps(items_host, fs, K, who));
    TRY(check_dims(d, 0));
    share_weight_prep(fs, K);
    return run_forward(fs, K, GROUPED, (hipStream_t)stream);
}

int rsaf_cnnlstm_forward_group_mixed(const rsaf_cnnlstm_forward_item* items_host, const rsaf_cnnlstm_arch* arch_host, int K,
                                     int input_dim, int num_classes, int lstm_layers, rsaf_stream_t stream) {
    const char* who = __func__;
    Fwd fs[RSAF_CNNLSTM_GROUP_MAX];
    TRY(check_group_args(K, items_host, who, "RSAF_CNNLSTM_GROUP_MAX"));
    if (!arch_host) return fail(RSAF_ERR_ARG, who, -1, "arch_host is NULL");
    for (int k = 0; k < K; ++k) {
        const rsaf_cnnlstm_forward_item& it = items_host[k];
        const Dims d{input_dim, arch_host[k].channels, arch_host[k].hidden, num_classes, lstm_layers, arch_host[k].act};
        if (const char* problem = dims_problem(d, 0)) return fail(RSAF_ERR_ARG, who, k, problem);
        TRY(check_item(d, it.x, it.B, it.T, it.weights, it.workspace, it.workspace_bytes, it.logits, who, k, &fs[k], RSAF_ERR_ARG));
    }
    TRY(check_overlaps(items_host, fs, K, who));
    share_weight_prep(fs, K);
    return run_forward(fs, K, MIXED, (hipStream_t)stream);
}

int64_t rsaf_cnn_resblock_workspace_bytes(int B, int T, int out_channels) {
    if (B <= 0 || T < 1) return -1;
    return 2 * pad4((int64_t)B * T * out_channels) * (int64_t)sizeof(float);
}

int rsaf_cnn_resblock_forward(const float* x, int B, int T, int in_channels, int out_channels, int act,
                              const float* w1, const float* b1, const float* wsc, const float* bsc,
                              const float* w2, const float* b2, void* workspace, int64_t workspace_bytes,
                              float* y, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(in_channels > 0 && in_channels % 4 == 0 && out_channels > 0 && out_channels % 4 == 0,
                   "channel counts must be positive multiples of 4");
    RSAF_CHECK_ARG(act == ACT_GELU || act == ACT_SILU, "activation must be gelu (1) or silu (2)");
    RSAF_CHECK_ARG(B >= 0 && B <= 65535, "batch must be in [0, 65535]");
    if (B == 0) return RSAF_OK;
    RSAF_CHECK_ARG(T >= 1, "sequence length must be >= 1");
    RSAF_CHECK_ARG(x && w1 && b1 && w2 && b2 && workspace && y, "NULL pointer");
    RSAF_CHECK_ARG((wsc != nullptr) == (bsc != nullptr), "shortcut weight and bias come together");
    RSAF_CHECK_ARG(wsc || in_channels == out_channels, "identity shortcut needs in_channels == out_channels");
    if (workspace_bytes < rsaf_cnn_resblock_workspace_bytes(B, T, out_channels)) {
        set_error("rsaf_cnn_resblock_forward: workspace too small");
        return RSAF_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int D = in_channels, C = out_channels;
    float* bufA = static_cast<float*>(workspace);
    float* bufB = bufA + pad4((int64_t)B * T * C);
    return resblock_f32(x, B, T, D, C, act, w1, b1, wsc, bsc, w2, b2, bufA, bufB, y, s);
}

int rsaf_attnpool_forward(const float* seq, int B, int T, int features, const float* watt, const float* batt,
                          float* pooled, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(features == 128 || features == 256, "features (2 * lstm_hidden_dim) must be 128 or 256");
    RSAF_CHECK_ARG(B >= 0 && T >= 1, "bad shape");
    if (B == 0) return RSAF_OK;
    RSAF_CHECK_ARG(seq && watt && batt && pooled, "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("attnpool_fc", s, 0.0, (double)B * T * features * 4);
    launch_attnpool(AttnPoolItem{seq, watt, batt, nullptr, nullptr, nullptr, pooled, B, T}, features / 2, 0, s);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

}  // extern "C"
