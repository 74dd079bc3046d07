// One training step of the CNN-LSTM-with-attention classifier on gfx950: forward in training mode and
// the backward pass (reference: CNNLSTM.forward under model.train() + loss.backward(),
// src/models.py:64-76,161-193 and src/dl_cv_strategies.py:118-125,241-243).
//
// Layout: activations channels-last [B][T][C] float32, exactly as in the inference path.  BatchNorm uses the
// statistics of the batch (biased variance over B*T rows, zero-padded frames included), dropout masks are
// inputs (float 0 or 1/(1-p); NULL = no dropout) so that the caller owns the random stream.
//
// Dense work goes through the exact-fp32 MFMA GEMM (gemm_f32.hip):
//   forward    conv = GEMM over the channels-last sequence (taps in K), LSTM input projections;
//   data grad  conv: the same GEMM over dy with tap-flipped, transposed weights; LSTM: dgates . W_ih (B as [K][N]);
//   weight grad  dW[M][taps*N] = sum_rows dy[row][M]^T x[row+tap][N]: both operands are transposed into [.][rows]
//              images (tap shift and sequence boundaries applied while transposing), then an NT GEMM split
//              along rows into `S` partial products that a second kernel sums in a fixed order (deterministic).
// The two recurrences are the persistent kernels of cnnlstm_lstm.hip: the forward one (saving gates and cell states) and the
// BPTT one.  This file: the training CNN, head and BatchNorm kernels and the phases of a step; the parameter blob, the saved
// activations and the scratch are laid out in cnnlstm_layout.h.
#include <algorithm>

#include "cnnlstm_host.h"
#include "cnnlstm_kernels.h"
#include "gemm_f32.h"

namespace rsaf {
namespace cnntrain {

// ---- activation and its derivative ----------------------------------------------------------------------------
__device__ __forceinline__ float act_f(float v, int act) {
    if (act == ACT_GELU) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    return v / (1.0f + expf(-v));
}
__device__ __forceinline__ float act_df(float v, int act) {
    if (act == ACT_GELU)
        return 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
    const float s = 1.0f / (1.0f + expf(-v));
    return s * (1.0f + v * (1.0f - s));
}

// ---- per-channel reductions over rows: partial sums in double, fixed partition => deterministic ------------------
// MODE 0: (sum y, sum y^2)            -> batch statistics
// MODE 1: (sum dz, sum dz*xhat)       -> BatchNorm backward; dz = dout (PRE = 0) or dout*mask*act'(g*xhat+be) (PRE = 1)
// MODE 2: (sum a, -)                  -> bias gradients / column sums
template <int MODE, int PRE>
__global__ __launch_bounds__(256) void colred_partial_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ y,
                                                             const float* __restrict__ mask, const float* __restrict__ stat,
                                                             const float* __restrict__ g, const float* __restrict__ be, int act,
                                                             int64_t rows, int C, double* __restrict__ partial) {
    // thread = (row lane ry, channel cx); block covers 64 channels x 4 row lanes
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cx;
    const int nparts = gridDim.x;
    const int64_t per = (rows + nparts - 1) / nparts;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(rows, r0 + per);
    double s0 = 0.0, s1 = 0.0;
    if (c < C) {
        float mean = 0.f, rstd = 0.f, gg = 0.f, bb = 0.f;
        if (MODE == 1) { mean = stat[c]; rstd = stat[2 * C + c]; gg = g[c]; bb = be[c]; }
#pragma unroll 4
        for (int64_t r = r0 + ry; r < r1; r += 4) {
            if (MODE == 0) {
                const double v = a[r * lda + c];
                s0 += v; s1 += v * v;
            } else if (MODE == 1) {
                const float xh = (y[r * C + c] - mean) * rstd;
                float dz = a[r * lda + c];
                if (PRE) {
                    if (mask) dz *= mask[r * C + c];
                    dz *= act_df(gg * xh + bb, act);
                }
                s0 += dz; s1 += (double)dz * xh;
            } else {
                s0 += a[r * lda + c];
            }
        }
    }
    __shared__ double sh[2][4][64];
    sh[0][ry][cx] = s0; sh[1][ry][cx] = s1;
    __syncthreads();
    if (ry == 0 && c < C) {
        partial[((int64_t)blockIdx.x * 2 + 0) * C + c] = sh[0][0][cx] + sh[0][1][cx] + sh[0][2][cx] + sh[0][3][cx];
        partial[((int64_t)blockIdx.x * 2 + 1) * C + c] = sh[1][0][cx] + sh[1][1][cx] + sh[1][2][cx] + sh[1][3][cx];
    }
}

// FIN 0: stat[c] = mean, stat[C+c] = biased var, stat[2C+c] = rstd        (out0 = stat)
// FIN 1: out0[c] = sum dz*xhat (dgamma), out1[c] = sum dz (dbeta); sums[c] = both / rows for the apply kernel
// FIN 2: out0[c] = sum
template <int FIN>
__global__ __launch_bounds__(256) void colred_final_kernel(const double* __restrict__ partial, int nparts, int64_t rows, int C,
                                                           float eps, float* __restrict__ out0, float* __restrict__ out1,
                                                           float* __restrict__ sums) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (int p = 0; p < nparts; ++p) { s0 += partial[((int64_t)p * 2 + 0) * C + c]; s1 += partial[((int64_t)p * 2 + 1) * C + c]; }
    if (FIN == 0) {
        const double mean = s0 / rows;
        double var = s1 / rows - mean * mean;
        if (var < 0) var = 0;
        out0[c] = (float)mean; out0[C + c] = (float)var; out0[2 * C + c] = (float)(1.0 / sqrt(var + (double)eps));
    } else if (FIN == 1) {
        out0[c] = (float)s1; out1[c] = (float)s0;
        sums[c] = (float)(s0 / rows); sums[C + c] = (float)(s1 / rows);
    } else {
        out0[c] = (float)s0;
    }
}

// ---- elementwise kernels (float4 over channels-last rows) --------------------------------------------------------
// out = act(bn(y)) * mask
__global__ __launch_bounds__(256) void bn_act_mask_kernel(const float4* __restrict__ y, const float* __restrict__ stat,
                                                          const float* __restrict__ g, const float* __restrict__ be,
                                                          const float4* __restrict__ mask, float4* __restrict__ out, int act,
                                                          int64_t n4, int C) {
    const int C4 = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const float4 v = y[i];
        const float4 m = mask ? mask[i] : make_float4(1.f, 1.f, 1.f, 1.f);
        float4 o;
        o.x = act_f((v.x - stat[c + 0]) * stat[2 * C + c + 0] * g[c + 0] + be[c + 0], act) * m.x;
        o.y = act_f((v.y - stat[c + 1]) * stat[2 * C + c + 1] * g[c + 1] + be[c + 1], act) * m.y;
        o.z = act_f((v.z - stat[c + 2]) * stat[2 * C + c + 2] * g[c + 2] + be[c + 2], act) * m.z;
        o.w = act_f((v.w - stat[c + 3]) * stat[2 * C + c + 3] * g[c + 3] + be[c + 3], act) * m.w;
        out[i] = o;
    }
}

// z = bn(y) + (bn_sc(ysc) | ident);  r = act(z)
__global__ __launch_bounds__(256) void bn_add_act_kernel(const float* __restrict__ y, const float* __restrict__ stat,
                                                         const float* __restrict__ g, const float* __restrict__ be,
                                                         const float* __restrict__ ysc, const float* __restrict__ statsc,
                                                         const float* __restrict__ gsc, const float* __restrict__ besc,
                                                         const float* __restrict__ ident, int64_t ld_ident,
                                                         float* __restrict__ z, float* __restrict__ r, int act, int64_t n, int C) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        float v = (y[i] - stat[c]) * stat[2 * C + c] * g[c] + be[c];
        if (ysc) v += (ysc[i] - statsc[c]) * statsc[2 * C + c] * gsc[c] + besc[c];
        else v += ident[(i / C) * ld_ident + c];
        z[i] = v;
        r[i] = act_f(v, act);
    }
}

// dz = dr * act'(z) (+ add)
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ dr, const float* __restrict__ z,
                                                      float* __restrict__ dz, int act, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        dz[i] = dr[i] * act_df(z[i], act);
}

// max_pool1d(2) backward fused with the activation backward of the block in front of it:
// dz1[b][2t+k][c] = (k is the arg-max of act(z1) over the pair, first wins) ? dp[b][t][c] * act'(z1) : 0; an odd last frame gets 0
__global__ __launch_bounds__(256) void pool_bwd_act_kernel(const float* __restrict__ dp, const float* __restrict__ z1,
                                                           float* __restrict__ dz1, int act, int B, int T, int Tp, int C) {
    const int64_t n = (int64_t)B * T * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const int64_t bt = i / C;
        const int t = (int)(bt % T);
        const int64_t b = bt / T;
        const int tp = t >> 1;
        float out = 0.f;
        if (tp < Tp) {
            const int64_t base = (b * T + 2 * tp) * C + c;
            const float za = z1[base], zb = z1[base + C];
            const float ra = act_f(za, act), rb = act_f(zb, act);
            const bool second = rb > ra;                  // first index wins ties (and NaN never wins): ATen max_pool1d
            if (second == ((t & 1) != 0)) out = dp[(b * Tp + tp) * C + c] * act_df((t & 1) ? zb : za, act);
        }
        dz1[i] = out;
    }
}

// BatchNorm backward, second half: dy = g*rstd*(dz - mean(dz) - xhat*mean(dz*xhat)); dz as in colred MODE 1
template <int PRE>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dout, const float* __restrict__ mask,
                                                           const float* __restrict__ y, const float* __restrict__ stat,
                                                           const float* __restrict__ g, const float* __restrict__ be,
                                                           const float* __restrict__ sums, float* __restrict__ dy, int act,
                                                           int64_t n, int C) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const float rstd = stat[2 * C + c];
        const float xh = (y[i] - stat[c]) * rstd;
        float dz = dout[i];
        if (PRE) {
            if (mask) dz *= mask[i];
            dz *= act_df(g[c] * xh + be[c], act);
        }
        dy[i] = g[c] * rstd * (dz - sums[c] - xh * sums[C + c]);
    }
}

// The same for a BatchNorm over exactly two rows (B T' = 2 in block 2: one sequence of four or five frames).  There xhat is
// +s in one row and -s in the other, so dy_a = -dy_b = g*rstd * (dz_a - dz_b)/2 * (1 - s^2), and 1 - s^2 = eps/(var + eps)
// = eps*rstd^2 is 1e-5 to 1e-3 at ordinary variances: the general form above leaves it to the cancellation in
// dz - mean(dz) - xhat*mean(dz*xhat), which keeps 2^-24 of the operands and so loses the whole factor in float32 (gradients
// 2e-4 to 4e-4 of their largest magnitude off float64, the project's bar being 1e-4).  Here the factor is formed directly.
// One thread per channel reads both rows before it writes either (dy may alias dout).
template <int PRE>
__global__ __launch_bounds__(256) void bn_bwd_pair_kernel(const float* __restrict__ dout, const float* __restrict__ mask,
                                                          const float* __restrict__ y, const float* __restrict__ stat,
                                                          const float* __restrict__ g, const float* __restrict__ be, float eps,
                                                          float* __restrict__ dy, int act, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float rstd = stat[2 * C + c];
    float dz[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        dz[r] = dout[r * C + c];
        if (PRE) {
            if (mask) dz[r] *= mask[r * C + c];
            dz[r] *= act_df(g[c] * ((y[r * C + c] - stat[c]) * rstd) + be[c], act);
        }
    }
    const float d = g[c] * rstd * (0.5f * (dz[0] - dz[1])) * (eps * rstd * rstd);
    dy[c] = d;
    dy[C + c] = -d;
}

__global__ __launch_bounds__(256) void mul_kernel(const float4* __restrict__ a, const float4* __restrict__ m,
                                                  float4* __restrict__ out, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 x = a[i], k = m[i];
        out[i] = make_float4(x.x * k.x, x.y * k.y, x.z * k.z, x.w * k.w);
    }
}

__global__ __launch_bounds__(256) void add_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                                                  float4* __restrict__ out, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 x = a[i], k = b[i];
        out[i] = make_float4(x.x + k.x, x.y + k.y, x.z + k.z, x.w + k.w);
    }
}

// w [Cout][3][Cin] -> wf [Cin][3][Cout], wf[ci][j][co] = w[co][2-j][ci]  (data gradient of a k=3/pad=1 convolution)
__global__ __launch_bounds__(256) void flip_taps_kernel(const float* __restrict__ w, float* __restrict__ wf, int Cout, int Cin) {
    const int64_t n = (int64_t)Cout * 3 * Cin;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int co = (int)(i % Cout);
        const int j = (int)((i / Cout) % 3);
        const int ci = (int)(i / (3 * (int64_t)Cout));
        wf[i] = w[((int64_t)co * 3 + (2 - j)) * Cin + ci];
    }
}

// dst[c][b*T + t] = src[(b*T + t + shift)*ld + c] if 0 <= t + shift < T else 0; columns [B*T, kp) are zero
__global__ __launch_bounds__(256) void transpose_shift_kernel(const float* __restrict__ src, int64_t ld, int ncols, int B, int T,
                                                              int shift, float* __restrict__ dst, int64_t kp) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
    const int64_t k0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int64_t rows = (int64_t)B * T;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t k = k0 + ty + 8 * i;
        const int c = c0 + tx;
        float v = 0.f;
        if (k < rows && c < ncols) {
            const int t = (int)(k % T) + shift;
            if (t >= 0 && t < T) v = src[(k + shift) * ld + c];
        }
        tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i;
        const int64_t k = k0 + tx;
        if (c < ncols && k < kp) dst[(int64_t)c * kp + k] = tile[tx][ty + 8 * i];
    }
}

__global__ __launch_bounds__(256) void sum_splits_kernel(const float* __restrict__ part, int S, int64_t n, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float s = 0.f;
        for (int z = 0; z < S; ++z) s += part[(int64_t)z * n + i];
        out[i] = s;
    }
}

// ---- attention pooling, training forward: probabilities and pooled context are kept -----------------------------------
constexpr int ATT_WAVES = 16;     // one 1024-thread workgroup per sequence: 16 row streams in flight on its CU

template <int NF>   // 2H = 64*NF
__global__ __launch_bounds__(ATT_WAVES * 64) void attnpool_train_kernel(const float* __restrict__ seq, const float* __restrict__ watt,
                                                                        const float* __restrict__ batt, float* __restrict__ prob,
                                                                        float* __restrict__ ctx_out, int T) {
    constexpr int F = 64 * NF;
    __shared__ float s_m[ATT_WAVES], s_l[ATT_WAVES], s_ctx[ATT_WAVES][F];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* sb = seq + (int64_t)b * T * F;
    float* pb = prob + (int64_t)b * T;
    float wa[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) wa[i] = watt[lane + 64 * i];
    const float ba = batt[0];
    float m = -INFINITY, l = 0.f;
#pragma unroll 2
    for (int t = w; t < T; t += ATT_WAVES) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < NF; ++i) d += sb[(int64_t)t * F + lane + 64 * i] * wa[i];
        const float sc = wave_sum(d) + ba;
        if (lane == 0) pb[t] = sc;
        const float mn = fmaxf(m, sc);
        l = l * expf(m - mn) + expf(sc - mn);
        m = mn;
    }
    if (lane == 0) { s_m[w] = m; s_l[w] = l; }
    __syncthreads();
    float M = s_m[0];
#pragma unroll
    for (int k = 1; k < ATT_WAVES; ++k) M = fmaxf(M, s_m[k]);
    float Lt = 0.f;
#pragma unroll
    for (int k = 0; k < ATT_WAVES; ++k) Lt += s_l[k] > 0.f ? s_l[k] * expf(s_m[k] - M) : 0.f;
    float ctx[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) ctx[i] = 0.f;
#pragma unroll 2
    for (int t = w; t < T; t += ATT_WAVES) {
        // lane 0 of this wave wrote pb[t] in the first pass: read it past the (non-coherent) vector L1
        const float p = expf(__hip_atomic_load(pb + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - M) / Lt;
#pragma unroll
        for (int i = 0; i < NF; ++i) ctx[i] += p * sb[(int64_t)t * F + lane + 64 * i];
        if (lane == 0) pb[t] = p;                    // after this wave's own read of the score (program order, same address)
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) s_ctx[w][lane + 64 * i] = ctx[i];
    __syncthreads();
    const int f = threadIdx.x;
    if (f < F) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < ATT_WAVES; ++k) a += s_ctx[k][f];
        ctx_out[(int64_t)b * F + f] = a;
    }
}

// logits = (ctx * mask) . wfc^T + bfc
__global__ __launch_bounds__(256) void fc_fwd_kernel(const float* __restrict__ ctx, const float* __restrict__ mask,
                                                     const float* __restrict__ wfc, const float* __restrict__ bfc,
                                                     float* __restrict__ logits, int F, int NC) {
    __shared__ float s_red[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = 0; c < NC; ++c) {
        float part = 0.f;
        for (int f = threadIdx.x; f < F; f += 256) {
            float v = ctx[(int64_t)b * F + f];
            if (mask) v *= mask[(int64_t)b * F + f];
            part += v * wfc[(int64_t)c * F + f];
        }
        part = wave_sum(part);
        __syncthreads();
        if (lane == 0) s_red[w] = part;
        __syncthreads();
        if (threadIdx.x == 0) logits[(int64_t)b * NC + c] = s_red[0] + s_red[1] + s_red[2] + s_red[3] + bfc[c];
    }
}

// classifier backward: thread f owns feature f.  dwfc[c][f], dbfc[c], dctx[b][f]
__global__ __launch_bounds__(256) void fc_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ ctx,
                                                     const float* __restrict__ mask, const float* __restrict__ wfc,
                                                     float* __restrict__ dwfc, float* __restrict__ dbfc, float* __restrict__ dctx,
                                                     int B, int F, int NC) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < F) {
        for (int c = 0; c < NC; ++c) {
            float s = 0.f;
            for (int b = 0; b < B; ++b) {
                float v = ctx[(int64_t)b * F + f];
                if (mask) v *= mask[(int64_t)b * F + f];
                s += dlogits[(int64_t)b * NC + c] * v;
            }
            dwfc[(int64_t)c * F + f] = s;
        }
        for (int b = 0; b < B; ++b) {
            float s = 0.f;
            for (int c = 0; c < NC; ++c) s += dlogits[(int64_t)b * NC + c] * wfc[(int64_t)c * F + f];
            if (mask) s *= mask[(int64_t)b * F + f];
            dctx[(int64_t)b * F + f] = s;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < NC) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dlogits[(int64_t)b * NC + threadIdx.x];
        dbfc[threadIdx.x] = s;
    }
}

// attention pooling backward for one sequence: dh[t][f] = p_t*dctx[f] + ds_t*wa[f], ds_t = p_t*(dp_t - sum_t' p_t' dp_t'),
// dp_t = dctx . h_t; per-sequence partials of dwatt[f] = sum_t ds_t h_t[f] and dbatt = sum_t ds_t
template <int NF>
__global__ __launch_bounds__(ATT_WAVES * 64) void attn_bwd_kernel(const float* __restrict__ seq, const float* __restrict__ prob,
                                                                  const float* __restrict__ dctx, const float* __restrict__ watt,
                                                                  float* __restrict__ dp_scratch, float* __restrict__ dseq,
                                                                  float* __restrict__ dwatt_part, float* __restrict__ dbatt_part, int T) {
    constexpr int F = 64 * NF;
    __shared__ float s_dot[ATT_WAVES], s_db[ATT_WAVES], s_dw[ATT_WAVES][F];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* sb = seq + (int64_t)b * T * F;
    const float* pb = prob + (int64_t)b * T;
    float* dpb = dp_scratch + (int64_t)b * T;
    float* db = dseq + (int64_t)b * T * F;
    float dc[NF], wa[NF], dw[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) { dc[i] = dctx[(int64_t)b * F + lane + 64 * i]; wa[i] = watt[lane + 64 * i]; dw[i] = 0.f; }
    float dot = 0.f;
#pragma unroll 2
    for (int t = w; t < T; t += ATT_WAVES) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < NF; ++i) d += sb[(int64_t)t * F + lane + 64 * i] * dc[i];
        d = wave_sum(d);
        if (lane == 0) dpb[t] = d;
        dot += pb[t] * d;
    }
    if (lane == 0) s_dot[w] = dot;
    __syncthreads();
    dot = 0.f;
#pragma unroll
    for (int k = 0; k < ATT_WAVES; ++k) dot += s_dot[k];
    float dbs = 0.f;
#pragma unroll 2
    for (int t = w; t < T; t += ATT_WAVES) {
        const float p = pb[t];
        const float ds = p * (__hip_atomic_load(dpb + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - dot);   // written by lane 0 above
        dbs += ds;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const float h = sb[(int64_t)t * F + lane + 64 * i];
            db[(int64_t)t * F + lane + 64 * i] = p * dc[i] + ds * wa[i];
            dw[i] += ds * h;
        }
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) s_dw[w][lane + 64 * i] = dw[i];
    if (lane == 0) s_db[w] = dbs;
    __syncthreads();
    const int f = threadIdx.x;
    if (f < F) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < ATT_WAVES; ++k) a += s_dw[k][f];
        dwatt_part[(int64_t)b * F + f] = a;
    }
    if (f == 0) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < ATT_WAVES; ++k) a += s_db[k];
        dbatt_part[b] = a;
    }
}

// ---- host-side helpers ------------------------------------------------------------------------------------------
static inline int ew_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 32)); }

struct Ctx {
    Dims d;
    hipStream_t s;
    float* ws;
    WLayout W;
};

static int bn_stats(const Ctx& c, const float* y, int64_t rows, float* stat) {
    const int C = c.d.C;
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(RED_PARTS, rows / 128));
    double* partial = reinterpret_cast<double*>(c.ws + c.W.red);
    ProfScope prof("train_bn_reduce", c.s, 0.0, (double)rows * C * 4);
    hipLaunchKernelGGL((colred_partial_kernel<0, 0>), dim3(parts, (C + 63) / 64), dim3(256), 0, c.s, y, (int64_t)C, nullptr, nullptr,
                       nullptr, nullptr, nullptr, 0, rows, C, partial);
    hipLaunchKernelGGL((colred_final_kernel<0>), dim3((C + 255) / 256), dim3(256), 0, c.s, partial, parts, rows, C, 1e-5f, stat,
                       nullptr, nullptr);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

static int colsum(const Ctx& c, const float* a, int64_t lda, int64_t rows, int N, float* out) {
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(RED_PARTS, rows / 128));
    double* partial = reinterpret_cast<double*>(c.ws + c.W.red);
    ProfScope prof("train_bn_reduce", c.s, 0.0, (double)rows * N * 4);
    hipLaunchKernelGGL((colred_partial_kernel<2, 0>), dim3(parts, (N + 63) / 64), dim3(256), 0, c.s, a, lda, nullptr, nullptr, nullptr,
                       nullptr, nullptr, 0, rows, N, partial);
    hipLaunchKernelGGL((colred_final_kernel<2>), dim3((N + 255) / 256), dim3(256), 0, c.s, partial, parts, rows, N, 0.f, out, nullptr,
                       nullptr);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// BatchNorm backward: dgamma, dbeta and dy (dy may alias dout)
static int bn_backward(const Ctx& c, const float* dout, const float* mask, bool pre, const float* y, const float* stat,
                       const float* g, const float* be, int64_t rows, float* dgamma, float* dbeta, float* dy) {
    const int C = c.d.C;
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(RED_PARTS, rows / 128));
    double* partial = reinterpret_cast<double*>(c.ws + c.W.red);
    float* sums = c.ws + c.W.bn_sums;                    // [2][C]
    {
        ProfScope prof("train_bn_reduce", c.s, 0.0, (double)rows * C * 8);
        if (pre)
            hipLaunchKernelGGL((colred_partial_kernel<1, 1>), dim3(parts, (C + 63) / 64), dim3(256), 0, c.s, dout, (int64_t)C, y, mask, stat,
                               g, be, c.d.act, rows, C, partial);
        else
            hipLaunchKernelGGL((colred_partial_kernel<1, 0>), dim3(parts, (C + 63) / 64), dim3(256), 0, c.s, dout, (int64_t)C, y, mask, stat,
                               g, be, c.d.act, rows, C, partial);
        hipLaunchKernelGGL((colred_final_kernel<1>), dim3((C + 255) / 256), dim3(256), 0, c.s, partial, parts, rows, C, 0.f, dgamma, dbeta,
                           sums);
    }
    {
        ProfScope prof("train_elementwise", c.s, 0.0, (double)rows * C * 12);
        const int64_t n = rows * C;
        if (rows == 2) {                                 // the two-row closed form (bn_bwd_pair_kernel); eps: that of bn_stats
            if (pre)
                hipLaunchKernelGGL((bn_bwd_pair_kernel<1>), dim3((C + 255) / 256), dim3(256), 0, c.s, dout, mask, y, stat, g, be, 1e-5f, dy, c.d.act, C);
            else
                hipLaunchKernelGGL((bn_bwd_pair_kernel<0>), dim3((C + 255) / 256), dim3(256), 0, c.s, dout, mask, y, stat, g, be, 1e-5f, dy, c.d.act, C);
        } else if (pre)
            hipLaunchKernelGGL((bn_bwd_apply_kernel<1>), dim3(ew_blocks(n)), dim3(256), 0, c.s, dout, mask, y, stat, g, be, sums, dy, c.d.act, n, C);
        else
            hipLaunchKernelGGL((bn_bwd_apply_kernel<0>), dim3(ew_blocks(n)), dim3(256), 0, c.s, dout, mask, y, stat, g, be, sums, dy, c.d.act, n, C);
    }
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

static int transpose_shift(const Ctx& c, const float* src, int64_t ld, int ncols, int B, int T, int shift, float* dst, int64_t kp) {
    ProfScope prof("train_transpose", c.s, 0.0, (double)B * T * ncols * 8);
    dim3 grid((unsigned)(kp / 32), (ncols + 31) / 32);
    hipLaunchKernelGGL(transpose_shift_kernel, grid, dim3(256), 0, c.s, src, ld, ncols, B, T, shift, dst, kp);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// dW[M][taps*N] (tap-major) = sum over rows of dy[row][M]^T xin[row + tap - taps/2][N], sequence boundaries respected;
// `shift0` replaces the tap shift when taps == 1 (recurrent weight gradients use -1 / +1)
static int wgrad(const Ctx& c, const float* dy, int64_t ld_dy, int M, const float* xin, int64_t ld_x, int N, int taps, int shift0,
                 int B, int T, float* out) {
    const int64_t rows = (int64_t)B * T;
    const Split sp = make_split(rows);
    float* t1 = c.ws + c.W.t1;
    float* t2 = c.ws + c.W.t2;
    float* part = c.ws + c.W.part;
    TRY(transpose_shift(c, dy, ld_dy, M, B, T, 0, t1, sp.kp));
    for (int j = 0; j < taps; ++j)
        TRY(transpose_shift(c, xin, ld_x, N, B, T, taps == 1 ? shift0 : j - taps / 2, t2 + (int64_t)j * N * sp.kp, sp.kp));
    const int NN = taps * N;
    GemmParams p = gemm_params_plain(t1, t2, sp.s == 1 ? out : part, M, NN, (int)sp.kc, sp.kp, sp.kp, NN);
    p.nz = (int)sp.s; p.nz2 = 1; p.sA1 = sp.kc; p.sB1 = sp.kc; p.sC1 = (int64_t)M * NN;
    TRY(launch_gemm_f32(p, c.s, "train_wgrad_gemm"));
    if (sp.s > 1) {
        const int64_t n = (int64_t)M * NN;
        ProfScope prof("train_elementwise", c.s, 0.0, (double)n * sp.s * 4);
        hipLaunchKernelGGL(sum_splits_kernel, dim3(ew_blocks(n)), dim3(256), 0, c.s, part, (int)sp.s, n, out);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    return RSAF_OK;
}

// data gradient of a k=3/pad=1 convolution: dx[B][T][Cin] from dy[B][T][Cout] and w[Cout][3][Cin]
static int flip_taps(const Ctx& c, const float* w, float* wf, int Cout, int Cin) {
    const int64_t n = (int64_t)Cout * 3 * Cin;
    ProfScope prof("train_elementwise", c.s, 0.0, (double)n * 8);
    hipLaunchKernelGGL(flip_taps_kernel, dim3(ew_blocks(n)), dim3(256), 0, c.s, w, wf, Cout, Cin);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

static int conv3_dgrad(const Ctx& c, const float* dy, const float* w, float* dx, int B, int T, int Cin, int Cout) {
    float* wf = c.ws + c.W.wflip;
    TRY(flip_taps(c, w, wf, Cout, Cin));
    return conv3(dy, wf, nullptr, nullptr, 0, 0, dx, B, T, Cout, Cin, ACT_NONE, c.s, "train_dgrad_gemm");
}

// ---- one replica's step, cut at its recurrences into phases -----------------------------------------------------------
// forward:  fwd_cnn (+ layer-0 input projection) | per layer: recurrence | fwd_after_rec (dropout + next input projection)
//           | fwd_head;   backward:  bwd_head | per layer: BPTT recurrence | bwd_after_rec | bwd_blocks.
// bwd_blocks ends with the gradient of the step's input where a replica asks for one (Replica::dx; the _dx entries): the 1x1
// data gradient of the shortcut, the flip of W1 and the k = 3 data-gradient GEMM with N = D, whose epilogue adds the two terms.
// A replica without dx runs the launches of the plain entries, in their order.
// The single entries run the phases of their one replica with the one-recurrence launchers; the group entries run every
// phase for all replicas and one grouped recurrence launch in between.
struct Replica {
    rsaf_cnnlstm_train_item it;
    PLayout L;                      // the replica's own architecture is c.d (one for all replicas, except in a mixed group)
    SLayout S;
    WLayout WL;
    Ctx c;
    const float* lin;               // forward: input of the next LSTM layer, `in` features wide
    int in;
    float *dcur, *dnext;            // backward: gradient w.r.t. the output of the current layer | the free buffer
    float* dx;                      // backward: where the gradient w.r.t. x goes [B][T][D], or NULL: none wanted
    float* dx_scratch;              //           tap-flipped transposed res_block1.conv1 weights [D][3][C] (dx_scratch_floats)
};

// argument checks of one replica (idx < 0: the single entries, whose messages carry no item)
// `short_code`: what a saved / scratch buffer below the replica's need returns
static int check_item(const Dims& d, const rsaf_cnnlstm_train_item& it, bool backward, hipStream_t s, const char* who, int idx,
                      Replica* r, int short_code = RSAF_ERR_WORKSPACE) {
    if (!(it.B >= 1 && it.B <= 65535)) return fail(RSAF_ERR_ARG, who, idx, "batch must be in [1, 65535]");
    if (!(it.T >= 2)) return fail(RSAF_ERR_ARG, who, idx, "sequence length must be >= 2 (max_pool1d(2) of the reference needs it)");
    if (!((int64_t)it.B * it.T <= 0x3fffffffLL)) return fail(RSAF_ERR_ARG, who, idx, "B*T too large");
    const bool ptrs = it.x && it.params && it.saved && it.scratch && (backward ? it.dlogits && it.grads : it.logits != nullptr);
    if (!ptrs) return fail(RSAF_ERR_ARG, who, idx, "NULL pointer");
    r->it = it;
    r->L = make_playout(d);
    r->S = make_slayout(d, it.B, it.T);
    r->WL = make_wlayout(d, it.B, it.T);
    if (it.saved_floats < r->S.total || it.scratch_floats < r->WL.total)
        return fail(short_code, who, idx, short_code == RSAF_ERR_WORKSPACE ? "saved/scratch buffer too small"
                                                                           : "saved/scratch buffer too small for this item's architecture");
    r->c = Ctx{d, s, it.scratch, r->WL};
    r->lin = nullptr; r->in = 0; r->dcur = r->dnext = nullptr;
    r->dx = r->dx_scratch = nullptr;
    return RSAF_OK;
}

// the input-gradient part of a backward item, after check_item: its own scratch, and no float of dx or dx_scratch inside
// anything else the item reads or writes
static int check_item_dx(const rsaf_cnnlstm_train_dx_item& it, const char* who, int idx, Replica* r) {
    if (!it.dx) return RSAF_OK;
    const Dims& d = r->c.d;
    const int64_t n_dx = (int64_t)it.B * it.T * d.D, n_scr = dx_scratch_floats(d);
    if (!it.dx_scratch) return fail(RSAF_ERR_ARG, who, idx, "dx without dx_scratch");
    if (it.dx_scratch_floats < n_scr) return fail(RSAF_ERR_WORKSPACE, who, idx, "dx_scratch too small (rsaf_cnnlstm_train_dx_scratch_floats)");
    struct { const char* name; const float* p; int64_t n; } other[] = {
        {"x", it.x, n_dx}, {"saved", it.saved, r->S.total}, {"scratch", it.scratch, r->WL.total}, {"grads", it.grads, r->L.total}};
    for (const auto& o : other) {
        if (overlap(it.dx, n_dx, o.p, o.n)) return fail(RSAF_ERR_ARG, who, idx, std::string("`dx` overlaps `") + o.name + "`");
        if (overlap(it.dx_scratch, n_scr, o.p, o.n)) return fail(RSAF_ERR_ARG, who, idx, std::string("`dx_scratch` overlaps `") + o.name + "`");
    }
    if (overlap(it.dx, n_dx, it.dx_scratch, n_scr)) return fail(RSAF_ERR_ARG, who, idx, "`dx` overlaps `dx_scratch`");
    r->dx = it.dx;
    r->dx_scratch = it.dx_scratch;
    return RSAF_OK;
}

static rsaf_cnnlstm_train_item base_item(const rsaf_cnnlstm_train_dx_item& it) {
    return rsaf_cnnlstm_train_item{it.x, it.B, it.T, it.params, it.mask_block1, it.mask_block2, it.mask_lstm_host, it.mask_fc, it.saved,
                                   it.saved_floats, it.scratch, it.scratch_floats, it.logits, it.bn_stats_out, it.dlogits, it.grads};
}

// dx and dx_scratch of item k against everything item j writes, and the other way round (after check_item_dx of both)
static int check_overlaps_dx(int K, const char* who, const Replica* reps) {
    auto ranges = [](const Replica& r, const float* (&p)[5], int64_t (&n)[5]) {
        p[0] = r.it.saved; n[0] = r.S.total; p[1] = r.it.scratch; n[1] = r.WL.total; p[2] = r.it.grads; n[2] = r.L.total;
        p[3] = r.dx; n[3] = r.dx ? (int64_t)r.it.B * r.it.T * r.c.d.D : 0;
        p[4] = r.dx_scratch; n[4] = r.dx ? dx_scratch_floats(r.c.d) : 0;
    };
    static const char* const names[5] = {"saved", "scratch", "grads", "dx", "dx_scratch"};
    for (int k = 1; k < K; ++k)
        for (int j = 0; j < k; ++j) {
            const float *pa[5], *pb[5];
            int64_t na[5], nb[5];
            ranges(reps[j], pa, na);
            ranges(reps[k], pb, nb);
            for (int a = 0; a < 5; ++a)
                for (int b = 0; b < 5; ++b) {
                    if ((a < 3 && b < 3) || !na[a] || !nb[b]) continue;       // the pairs without dx: check_overlaps
                    if (overlap(pa[a], na[a], pb[b], nb[b]))
                        return fail(RSAF_ERR_ARG, who, k, std::string("its `") + names[b] + "` overlaps `" + names[a] + "` of item " + std::to_string(j));
                }
        }
    return RSAF_OK;
}

// no two replicas overlapping in what the pass writes (reps[k].c.d: the replica's own dims)
static int check_overlaps(const rsaf_cnnlstm_train_item* items, int K, bool backward, const char* who, const Replica* reps) {
    for (int k = 1; k < K; ++k)
        for (int j = 0; j < k; ++j) {
            const rsaf_cnnlstm_train_item &a = items[j], &b = items[k];
            const int NC = reps[k].c.d.NC;
            const char* what = overlap(a.saved, reps[j].S.total, b.saved, reps[k].S.total) ? "saved"
                               : overlap(a.scratch, reps[j].WL.total, b.scratch, reps[k].WL.total) ? "scratch"
                               : !backward && overlap(a.logits, (int64_t)a.B * NC, b.logits, (int64_t)b.B * NC) ? "logits"
                               : backward && overlap(a.grads, reps[j].L.total, b.grads, reps[k].L.total) ? "grads" : nullptr;
            if (what) return fail(RSAF_ERR_ARG, who, k, std::string("shares `") + what + "` with item " + std::to_string(j));
        }
    return RSAF_OK;
}

static int check_group(const Dims& d, const rsaf_cnnlstm_train_item* items, int K, bool backward, hipStream_t s, const char* who,
                       Replica* reps) {
    TRY(check_dims(d));
    TRY(check_group_args(K, items, who));
    for (int k = 0; k < K; ++k) TRY(check_item(d, items[k], backward, s, who, k, &reps[k]));
    return check_overlaps(items, K, backward, who, reps);
}

// the same for a mixed group: the dims of item k are (input_dim, arch[k], num_classes, lstm_layers), and every message names its item
static int check_group_mixed(const rsaf_cnnlstm_train_item* items, const rsaf_cnnlstm_arch* arch, int K, int input_dim, int num_classes,
                             int lstm_layers, bool backward, hipStream_t s, const char* who, Replica* reps) {
    TRY(check_group_args(K, items, who));
    if (!arch) return fail(RSAF_ERR_ARG, who, -1, "arch_host is NULL");
    for (int k = 0; k < K; ++k) {
        const Dims d{input_dim, arch[k].channels, arch[k].hidden, num_classes, lstm_layers, arch[k].act};
        if (const char* problem = dims_problem(d, TRAIN_C_MAX)) return fail(RSAF_ERR_ARG, who, k, problem);
        TRY(check_item(d, items[k], backward, s, who, k, &reps[k], RSAF_ERR_ARG));
    }
    return check_overlaps(items, K, backward, who, reps);
}

// the backward groups with input gradients: the checks of the plain entries on the plain part of every item, then the dx part
static int check_group_dx(const Dims* d, const rsaf_cnnlstm_train_dx_item* items, const rsaf_cnnlstm_arch* arch, int K, int input_dim,
                          int num_classes, int lstm_layers, hipStream_t s, const char* who, Replica* reps) {
    TRY(check_group_args(K, items, who));
    rsaf_cnnlstm_train_item base[RSAF_CNNLSTM_GROUP_MAX];
    for (int k = 0; k < K; ++k) base[k] = base_item(items[k]);
    if (d) TRY(check_group(*d, base, K, true, s, who, reps));
    else TRY(check_group_mixed(base, arch, K, input_dim, num_classes, lstm_layers, true, s, who, reps));
    for (int k = 0; k < K; ++k) TRY(check_item_dx(items[k], who, k, &reps[k]));
    return check_overlaps_dx(K, who, reps);
}

static int fwd_inproj(Replica& r, const PLayout& L, int l) {
    const Dims& d = r.c.d;
    const int64_t rows2 = (int64_t)r.it.B * (r.it.T / 2);
    GemmParams p = gemm_params_plain(r.lin, r.it.params + L.wih[l], r.it.saved + r.S.gates[l], (int)rows2, 8 * d.H, r.in, r.in, r.in, 8 * d.H);
    p.bias = r.it.params + L.bsum[l];
    return launch_gemm_f32(p, r.c.s, "train_lstm_inproj_gemm");
}

static int fwd_cnn(Replica& r, const PLayout& L) {
    const Ctx& c = r.c;
    const Dims& d = c.d;
    const SLayout& S = r.S;
    hipStream_t s = c.s;
    const int B = r.it.B, T = r.it.T, D = d.D, C = d.C, Tp = T / 2, act = d.act;
    const int64_t rows = (int64_t)B * T, rows2 = (int64_t)B * Tp;
    const float* x = r.it.x;
    const float* P = r.it.params;
    float* saved = r.it.saved;
    float* st = saved + S.stat;
    auto stat = [&](int i) { return st + (int64_t)i * 3 * C; };
    float* r1 = r.it.scratch + r.WL.bufA;

    // ---- res_block1 (src/models.py:64-76) --------------------------------------------------------------------
    TRY(conv3(x, P + L.c1.w, P + L.c1.b, nullptr, 0, 0, saved + S.y1, B, T, D, C, ACT_NONE, s, "train_conv_gemm"));
    TRY(bn_stats(c, saved + S.y1, rows, stat(0)));
    {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows * C * 12);
        hipLaunchKernelGGL(bn_act_mask_kernel, dim3(ew_blocks(rows * C / 4)), dim3(256), 0, s, reinterpret_cast<const float4*>(saved + S.y1),
                           stat(0), P + L.c1.g, P + L.c1.be, reinterpret_cast<const float4*>(r.it.mask_block1),
                           reinterpret_cast<float4*>(saved + S.a1d), act, rows * C / 4, C);
    }
    if (D != C) {
        GemmParams p = gemm_params_plain(x, P + L.sc.w, saved + S.ysc, (int)rows, C, D, D, D, C);
        p.bias = P + L.sc.b;
        TRY(launch_gemm_f32(p, s, "train_conv_gemm"));
        TRY(bn_stats(c, saved + S.ysc, rows, stat(1)));
    }
    TRY(conv3(saved + S.a1d, P + L.c2.w, P + L.c2.b, nullptr, 0, 0, saved + S.y2, B, T, C, C, ACT_NONE, s, "train_conv_gemm"));
    TRY(bn_stats(c, saved + S.y2, rows, stat(2)));
    {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows * C * 16);
        hipLaunchKernelGGL(bn_add_act_kernel, dim3(ew_blocks(rows * C)), dim3(256), 0, s, saved + S.y2, stat(2), P + L.c2.g, P + L.c2.be,
                           D != C ? saved + S.ysc : nullptr, stat(1), D != C ? P + L.sc.g : nullptr, D != C ? P + L.sc.be : nullptr,
                           x, (int64_t)D, saved + S.z1, r1, act, rows * C, C);
    }
    // ---- max_pool1d(2) (:177) -----------------------------------------------------------------------------------
    {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows * C * 6);
        launch_pool2(r1, saved + S.p, B, T, Tp, C, ew_blocks(rows2 * C / 4), s);
    }
    // ---- res_block2, identity shortcut (:178) ----------------------------------------------------------------------
    TRY(conv3(saved + S.p, P + L.c3.w, P + L.c3.b, nullptr, 0, 0, saved + S.y3, B, Tp, C, C, ACT_NONE, s, "train_conv_gemm"));
    TRY(bn_stats(c, saved + S.y3, rows2, stat(3)));
    {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows2 * C * 12);
        hipLaunchKernelGGL(bn_act_mask_kernel, dim3(ew_blocks(rows2 * C / 4)), dim3(256), 0, s, reinterpret_cast<const float4*>(saved + S.y3),
                           stat(3), P + L.c3.g, P + L.c3.be, reinterpret_cast<const float4*>(r.it.mask_block2),
                           reinterpret_cast<float4*>(saved + S.a3d), act, rows2 * C / 4, C);
    }
    TRY(conv3(saved + S.a3d, P + L.c4.w, P + L.c4.b, nullptr, 0, 0, saved + S.y4, B, Tp, C, C, ACT_NONE, s, "train_conv_gemm"));
    TRY(bn_stats(c, saved + S.y4, rows2, stat(4)));
    {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows2 * C * 16);
        hipLaunchKernelGGL(bn_add_act_kernel, dim3(ew_blocks(rows2 * C)), dim3(256), 0, s, saved + S.y4, stat(4), P + L.c4.g, P + L.c4.be,
                           nullptr, nullptr, nullptr, nullptr, saved + S.p, (int64_t)C, saved + S.z2, saved + S.r2, act, rows2 * C, C);
    }
    RSAF_CHECK_HIP(hipGetLastError());
    // ---- LSTM (:184): input projection of the first layer ------------------------------------------------------------
    r.lin = saved + S.r2;
    r.in = C;
    return fwd_inproj(r, L, 0);
}

static LstmRecItem fwd_rec_item(const Replica& r, const PLayout& L, int l) {
    float* gates = r.it.saved + r.S.gates[l];
    return LstmRecItem{gates, r.it.params + L.whh[l], r.it.saved + r.S.hout[l], gates, r.it.saved + r.S.cst[l], r.it.B, r.it.T / 2};
}

// dropout between the layers and the next layer's input projection
static int fwd_after_rec(Replica& r, const PLayout& L, int l) {
    const Dims& d = r.c.d;
    hipStream_t s = r.c.s;
    const int H = d.H;
    const int64_t rows2 = (int64_t)r.it.B * (r.it.T / 2);
    r.lin = r.it.saved + r.S.hout[l];
    r.in = 2 * H;
    if (l == d.L - 1) return RSAF_OK;
    const float* mk = r.it.mask_lstm_host ? r.it.mask_lstm_host[l] : nullptr;
    if (mk) {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows2 * 2 * H * 12);
        hipLaunchKernelGGL(mul_kernel, dim3(ew_blocks(rows2 * 2 * H / 4)), dim3(256), 0, s, reinterpret_cast<const float4*>(r.lin),
                           reinterpret_cast<const float4*>(mk), reinterpret_cast<float4*>(r.it.saved + r.S.hdrop[l]), rows2 * 2 * H / 4);
        RSAF_CHECK_HIP(hipGetLastError());
        r.lin = r.it.saved + r.S.hdrop[l];
    }
    return fwd_inproj(r, L, l + 1);
}

// attention pooling + dropout + classifier (:187-191)
static int fwd_head(Replica& r, const PLayout& L) {
    const Dims& d = r.c.d;
    const SLayout& S = r.S;
    hipStream_t s = r.c.s;
    const int B = r.it.B, Tp = r.it.T / 2, H = d.H;
    const int64_t rows2 = (int64_t)B * Tp;
    const float* P = r.it.params;
    float* saved = r.it.saved;
    {
        ProfScope prof("train_attnpool", s, 0.0, (double)rows2 * 2 * H * 8);
        if (H == 128)
            hipLaunchKernelGGL(attnpool_train_kernel<4>, dim3(B), dim3(ATT_WAVES * 64), 0, s, r.lin, P + L.watt, P + L.batt, saved + S.prob, saved + S.ctx, Tp);
        else
            hipLaunchKernelGGL(attnpool_train_kernel<2>, dim3(B), dim3(ATT_WAVES * 64), 0, s, r.lin, P + L.watt, P + L.batt, saved + S.prob, saved + S.ctx, Tp);
        hipLaunchKernelGGL(fc_fwd_kernel, dim3(B), dim3(256), 0, s, saved + S.ctx, r.it.mask_fc, P + L.wfc, P + L.bfc, r.it.logits, 2 * H, d.NC);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    if (r.it.bn_stats_out)
        RSAF_CHECK_HIP(hipMemcpyAsync(r.it.bn_stats_out, saved + S.stat, sizeof(float) * 5 * 3 * d.C, hipMemcpyDeviceToDevice, s));
    return RSAF_OK;
}

// classifier + attention pooling
static int bwd_head(Replica& r, const PLayout& L) {
    const Ctx& c = r.c;
    const Dims& d = c.d;
    const SLayout& S = r.S;
    hipStream_t s = c.s;
    const int B = r.it.B, Tp = r.it.T / 2, H = d.H, F = 2 * H;
    const int64_t rows2 = (int64_t)B * Tp;
    const float* P = r.it.params;
    float* G = r.it.grads;
    float* saved = r.it.saved;
    float* dctx = r.it.scratch + r.WL.dctx;
    float* dwatt_part = r.it.scratch + r.WL.dwatt_part;
    float* dbatt_part = r.it.scratch + r.WL.dbatt_part;
    float* dp_scr = r.it.scratch + r.WL.dp;
    const float* seq_top = saved + S.hout[d.L - 1];
    float* dseq = r.it.scratch + r.WL.bufA;             // [rows2][2H]
    {
        ProfScope prof("train_attnpool", s, 0.0, (double)rows2 * F * 12);
        hipLaunchKernelGGL(fc_bwd_kernel, dim3((F + 255) / 256), dim3(256), 0, s, r.it.dlogits, saved + S.ctx, r.it.mask_fc, P + L.wfc,
                           G + L.wfc, G + L.bfc, dctx, B, F, d.NC);
        if (H == 128)
            hipLaunchKernelGGL(attn_bwd_kernel<4>, dim3(B), dim3(ATT_WAVES * 64), 0, s, seq_top, saved + S.prob, dctx, P + L.watt, dp_scr, dseq,
                               dwatt_part, dbatt_part, Tp);
        else
            hipLaunchKernelGGL(attn_bwd_kernel<2>, dim3(B), dim3(ATT_WAVES * 64), 0, s, seq_top, saved + S.prob, dctx, P + L.watt, dp_scr, dseq,
                               dwatt_part, dbatt_part, Tp);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    TRY(colsum(c, dwatt_part, F, B, F, G + L.watt));
    TRY(colsum(c, dbatt_part, 1, B, 1, G + L.batt));
    r.dcur = dseq;                                      // gradient w.r.t. the output of the top layer  [rows2][2H]
    r.dnext = r.it.scratch + r.WL.bufB;
    return RSAF_OK;
}

static LstmBwdItem bwd_rec_item(const Replica& r, const PLayout& L, int l) {
    return LstmBwdItem{r.it.saved + r.S.gates[l], r.it.saved + r.S.cst[l], r.dcur, r.it.params + L.whh[l], r.it.B, r.it.T / 2};
}

// after the BPTT recurrence of layer l, `gates` holds dgates (pre-activation gradients) [rows2][8H]: bias, weight and
// input gradients
static int bwd_after_rec(Replica& r, const PLayout& L, int l) {
    const Ctx& c = r.c;
    const Dims& d = c.d;
    const SLayout& S = r.S;
    hipStream_t s = c.s;
    const int B = r.it.B, Tp = r.it.T / 2, C = d.C, H = d.H, F = 2 * H;
    const int64_t rows2 = (int64_t)B * Tp;
    const float* P = r.it.params;
    float* G = r.it.grads;
    float* saved = r.it.saved;
    const float* const* mask_lstm_host = r.it.mask_lstm_host;
    float* gates = saved + S.gates[l];
    const int in = l == 0 ? C : 2 * H;
    const float* lin = l == 0 ? saved + S.r2
                              : ((mask_lstm_host && mask_lstm_host[l - 1]) ? saved + S.hdrop[l - 1] : saved + S.hout[l - 1]);
    TRY(colsum(c, gates, 8 * H, rows2, 8 * H, G + L.bsum[l]));
    TRY(wgrad(c, gates, 8 * H, 8 * H, lin, in, in, 1, 0, B, Tp, G + L.wih[l]));
    for (int dir = 0; dir < 2; ++dir)
        TRY(wgrad(c, gates + dir * 4 * H, 8 * H, 4 * H, saved + S.hout[l] + dir * H, 2 * H, H, 1, dir ? +1 : -1, B, Tp,
                  G + L.whh[l] + (int64_t)dir * 4 * H * H));
    // input gradient: dgates . W_ih  (B operand [K = 8H][N = in])
    {
        GemmParams p = gemm_params_plain(gates, P + L.wih[l], r.dnext, (int)rows2, in, 8 * H, 8 * H, in, in);
        p.b_kn = 1;
        TRY(launch_gemm_f32(p, s, "train_dgrad_gemm"));
    }
    if (l > 0 && mask_lstm_host && mask_lstm_host[l - 1]) {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows2 * F * 12);
        hipLaunchKernelGGL(mul_kernel, dim3(ew_blocks(rows2 * F / 4)), dim3(256), 0, s, reinterpret_cast<const float4*>(r.dnext),
                           reinterpret_cast<const float4*>(mask_lstm_host[l - 1]), reinterpret_cast<float4*>(r.dnext), rows2 * F / 4);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    std::swap(r.dcur, r.dnext);
    return RSAF_OK;
}

// the two residual blocks; r.dcur = dr2 [rows2][C], r.dnext (the other of bufA, bufB) is free
static int bwd_blocks(Replica& r, const PLayout& L) {
    const Ctx& c = r.c;
    const Dims& d = c.d;
    const SLayout& S = r.S;
    hipStream_t s = c.s;
    const int B = r.it.B, T = r.it.T, Tp = T / 2, D = d.D, C = d.C, act = d.act;
    const int64_t rows = (int64_t)B * T, rows2 = (int64_t)B * Tp;
    const float* x = r.it.x;
    const float* P = r.it.params;
    float* G = r.it.grads;
    float* saved = r.it.saved;
    float* st = saved + S.stat;
    auto stat = [&](int i) { return st + (int64_t)i * 3 * C; };
    float* bufA = r.it.scratch + r.WL.bufA;
    float* bufB = r.it.scratch + r.WL.bufB;
    float* bufC = r.it.scratch + r.WL.bufC;
    float* dr2 = r.dcur;
    float* dz2 = r.dnext;
    // ---- res_block2 -------------------------------------------------------------------------------------------------------
    {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows2 * C * 12);
        hipLaunchKernelGGL(act_bwd_kernel, dim3(ew_blocks(rows2 * C)), dim3(256), 0, s, dr2, saved + S.z2, dz2, act, rows2 * C);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    float* dy = dr2;                                    // reuse
    TRY(bn_backward(c, dz2, nullptr, false, saved + S.y4, stat(4), P + L.c4.g, P + L.c4.be, rows2, G + L.c4.g, G + L.c4.be, dy));
    TRY(colsum(c, dy, C, rows2, C, G + L.c4.b));
    TRY(wgrad(c, dy, C, C, saved + S.a3d, C, C, 3, 0, B, Tp, G + L.c4.w));
    float* da = bufC;
    TRY(conv3_dgrad(c, dy, P + L.c4.w, da, B, Tp, C, C));
    TRY(bn_backward(c, da, r.it.mask_block2, true, saved + S.y3, stat(3), P + L.c3.g, P + L.c3.be, rows2, G + L.c3.g, G + L.c3.be, dy));
    TRY(colsum(c, dy, C, rows2, C, G + L.c3.b));
    TRY(wgrad(c, dy, C, C, saved + S.p, C, C, 3, 0, B, Tp, G + L.c3.w));
    TRY(conv3_dgrad(c, dy, P + L.c3.w, da, B, Tp, C, C));
    float* dpool = dy;                                  // dp = dgrad + dz2 (identity shortcut)
    {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows2 * C * 12);
        hipLaunchKernelGGL(add_kernel, dim3(ew_blocks(rows2 * C / 4)), dim3(256), 0, s, reinterpret_cast<const float4*>(da),
                           reinterpret_cast<const float4*>(dz2), reinterpret_cast<float4*>(dpool), rows2 * C / 4);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    // ---- max_pool1d backward + activation backward of res_block1 ------------------------------------------------------------
    float* dz1 = bufC;                                  // [rows][C]  (da is dead)
    {
        ProfScope prof("train_elementwise", s, 0.0, (double)rows * C * 10);
        hipLaunchKernelGGL(pool_bwd_act_kernel, dim3(ew_blocks(rows * C)), dim3(256), 0, s, dpool, saved + S.z1, dz1, act, B, T, Tp, C);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    // ---- res_block1 -------------------------------------------------------------------------------------------------------
    float* dy1 = dz2 == bufA ? bufA : bufB;             // any buffer other than dz1 (bufC)
    float* dy2 = dy1 == bufA ? bufB : bufA;
    if (D != C) {
        TRY(bn_backward(c, dz1, nullptr, false, saved + S.ysc, stat(1), P + L.sc.g, P + L.sc.be, rows, G + L.sc.g, G + L.sc.be, dy1));
        TRY(colsum(c, dy1, C, rows, C, G + L.sc.b));
        TRY(wgrad(c, dy1, C, C, x, D, D, 1, 0, B, T, G + L.sc.w));
    }
    TRY(bn_backward(c, dz1, nullptr, false, saved + S.y2, stat(2), P + L.c2.g, P + L.c2.be, rows, G + L.c2.g, G + L.c2.be, dy2));
    TRY(colsum(c, dy2, C, rows, C, G + L.c2.b));
    TRY(wgrad(c, dy2, C, C, saved + S.a1d, C, C, 3, 0, B, T, G + L.c2.w));
    // input gradient, shortcut term: dz1 itself for the identity (bufC is not written again), else dy_sc . Wsc while dy1 still
    // holds dy_sc.  It waits in t2, which is free between two weight gradients and holds [Nmax >= 3D][kp >= rows] floats.
    const float* dx_sc = dz1;
    if (r.dx && D != C) {
        float* sc_term = c.ws + c.W.t2;                              // [rows][D]
        GemmParams p = gemm_params_plain(dy1, P + L.sc.w, sc_term, (int)rows, D, C, C, D, D);
        p.b_kn = 1;                                                  // Wsc [C][D] read as [K][N]
        TRY(launch_gemm_f32(p, s, "train_dgrad_gemm"));
        dx_sc = sc_term;
    }
    TRY(conv3_dgrad(c, dy2, P + L.c2.w, dy1, B, T, C, C));           // dy1 now holds d(a1d)
    TRY(bn_backward(c, dy1, r.it.mask_block1, true, saved + S.y1, stat(0), P + L.c1.g, P + L.c1.be, rows, G + L.c1.g, G + L.c1.be, dy2));
    TRY(colsum(c, dy2, C, rows, C, G + L.c1.b));
    if (r.dx) {
        // dx = dgrad of conv1 (the k = 3 data-gradient GEMM with N = D, flipped weights [D][3][C] in dx_scratch) + the shortcut
        // term as the epilogue's residual; ahead of the last weight gradient, which takes t2 back
        TRY(flip_taps(c, P + L.c1.w, r.dx_scratch, C, D));
        TRY(conv3(dy2, r.dx_scratch, nullptr, dx_sc, D, (int64_t)T * D, r.dx, B, T, C, D, ACT_NONE, s, "train_dgrad_gemm"));
    }
    TRY(wgrad(c, dy2, C, C, x, D, D, 3, 0, B, T, G + L.c1.w));
    return RSAF_OK;
}

// GROUPED (one architecture): one launch carries the recurrences of all replicas (4-row kernels; needs every batch at or
// under the threshold, else all run per replica).  MIXED (an architecture per replica): one launch carries those at or under
// the threshold, and a replica above it has its recurrence launched on its own.  SINGLE: one launch per replica through the
// one-recurrence launchers (launch_lstm_rec_layer / launch_lstm_bwd_layer, all_or_none).  Every replica carries its own dims
// (c.d) and layouts.

static int run_forward(Replica* reps, int K, int mode) {
    hipStream_t s = reps[0].c.s;
    const int layers = reps[0].c.d.L;
    for (int k = 0; k < K; ++k) TRY(fwd_cnn(reps[k], reps[k].L));
    for (int l = 0; l < layers; ++l) {
        LstmRecMixedItem recs[RSAF_CNNLSTM_GROUP_MAX];
        for (int k = 0; k < K; ++k) recs[k] = LstmRecMixedItem{fwd_rec_item(reps[k], reps[k].L, l), reps[k].c.d.H};
        TRY(launch_lstm_rec_layer(recs, K, mode, true, s));
        for (int k = 0; k < K; ++k) TRY(fwd_after_rec(reps[k], reps[k].L, l));
    }
    for (int k = 0; k < K; ++k) TRY(fwd_head(reps[k], reps[k].L));
    return RSAF_OK;
}

static int run_backward(Replica* reps, int K, int mode) {
    hipStream_t s = reps[0].c.s;
    const int layers = reps[0].c.d.L;
    for (int k = 0; k < K; ++k) TRY(bwd_head(reps[k], reps[k].L));
    for (int l = layers - 1; l >= 0; --l) {              // LSTM layers, top down
        LstmBwdMixedItem recs[RSAF_CNNLSTM_GROUP_MAX];
        for (int k = 0; k < K; ++k) recs[k] = LstmBwdMixedItem{bwd_rec_item(reps[k], reps[k].L, l), reps[k].c.d.H};
        TRY(launch_lstm_bwd_layer(recs, K, mode, true, s));
        for (int k = 0; k < K; ++k) TRY(bwd_after_rec(reps[k], reps[k].L, l));
    }
    for (int k = 0; k < K; ++k) TRY(bwd_blocks(reps[k], reps[k].L));
    return RSAF_OK;
}

}  // namespace cnntrain
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::cnntrain;

extern "C" {

int64_t rsaf_cnnlstm_train_param_floats(int input_dim, int channels, int hidden, int num_classes, int lstm_layers) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    if (check_dims(d) != RSAF_OK) return -1;
    return make_playout(d).total;
}

int rsaf_cnnlstm_train_param_offsets(int input_dim, int channels, int hidden, int num_classes, int lstm_layers,
                                     int64_t* offsets_host, int cap, int* n_host) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, ACT_SILU};
    TRY(check_dims(d));
    RSAF_CHECK_ARG(offsets_host && n_host, "NULL output");
    const PLayout L = make_playout(d);
    int64_t v[20 + 12 + 4];
    int n = 0;
    for (const ConvP* c : {&L.c1, &L.sc, &L.c2, &L.c3, &L.c4}) { v[n++] = c->w; v[n++] = c->b; v[n++] = c->g; v[n++] = c->be; }
    for (int l = 0; l < d.L; ++l) { v[n++] = L.wih[l]; v[n++] = L.bsum[l]; v[n++] = L.whh[l]; }
    v[n++] = L.watt; v[n++] = L.batt; v[n++] = L.wfc; v[n++] = L.bfc;
    RSAF_CHECK_ARG(cap >= n, "offsets_host too small");
    for (int i = 0; i < n; ++i) offsets_host[i] = v[i];
    *n_host = n;
    return RSAF_OK;
}

int64_t rsaf_cnnlstm_train_saved_floats(int B, int T, int input_dim, int channels, int hidden, int lstm_layers) {
    if (B <= 0 || T < 2) return -1;
    Dims d{input_dim, channels, hidden, 2, lstm_layers, ACT_SILU};
    if (check_dims(d) != RSAF_OK) return -1;
    return make_slayout(d, B, T).total;
}

int64_t rsaf_cnnlstm_train_scratch_floats(int B, int T, int input_dim, int channels, int hidden, int lstm_layers) {
    if (B <= 0 || T < 2) return -1;
    Dims d{input_dim, channels, hidden, 2, lstm_layers, ACT_SILU};
    if (check_dims(d) != RSAF_OK) return -1;
    return make_wlayout(d, B, T).total;
}

int rsaf_cnnlstm_train_forward(const float* x, int B, int T, int input_dim, int channels, int hidden, int num_classes,
                               int lstm_layers, int act, const float* params, const float* mask_block1,
                               const float* mask_block2, const float* const* mask_lstm_host, const float* mask_fc, float* saved,
                               int64_t saved_floats, float* scratch, int64_t scratch_floats, float* logits,
                               float* bn_stats_out, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, act};
    TRY(check_dims(d));
    const rsaf_cnnlstm_train_item it{x, B, T, params, mask_block1, mask_block2, mask_lstm_host, mask_fc, saved, saved_floats,
                                     scratch, scratch_floats, logits, bn_stats_out, nullptr, nullptr};
    Replica r;
    TRY(check_item(d, it, false, (hipStream_t)stream, __func__, -1, &r));
    return run_forward(&r, 1, SINGLE);
}

int rsaf_cnnlstm_train_backward(const float* x, int B, int T, int input_dim, int channels, int hidden, int num_classes,
                                int lstm_layers, int act, const float* params, const float* mask_block1,
                                const float* mask_block2, const float* const* mask_lstm_host, const float* mask_fc, float* saved,
                                int64_t saved_floats, float* scratch, int64_t scratch_floats, const float* dlogits, float* grads,
                                rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, act};
    TRY(check_dims(d));
    const rsaf_cnnlstm_train_item it{x, B, T, params, mask_block1, mask_block2, mask_lstm_host, mask_fc, saved, saved_floats,
                                     scratch, scratch_floats, nullptr, nullptr, dlogits, grads};
    Replica r;
    TRY(check_item(d, it, true, (hipStream_t)stream, __func__, -1, &r));
    return run_backward(&r, 1, SINGLE);
}

int64_t rsaf_cnnlstm_train_dx_scratch_floats(int input_dim, int channels) {
    Dims d{input_dim, channels, 64, 2, 1, ACT_SILU};
    if (check_dims(d) != RSAF_OK) return -1;
    return dx_scratch_floats(d);
}

int rsaf_cnnlstm_train_backward_dx(const float* x, int B, int T, int input_dim, int channels, int hidden, int num_classes,
                                   int lstm_layers, int act, const float* params, const float* mask_block1,
                                   const float* mask_block2, const float* const* mask_lstm_host, const float* mask_fc, float* saved,
                                   int64_t saved_floats, float* scratch, int64_t scratch_floats, const float* dlogits, float* grads,
                                   float* dx, float* dx_scratch, int64_t dx_scratch_floats, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, act};
    TRY(check_dims(d));
    const rsaf_cnnlstm_train_dx_item it{x, B, T, params, mask_block1, mask_block2, mask_lstm_host, mask_fc, saved, saved_floats,
                                        scratch, scratch_floats, nullptr, nullptr, dlogits, grads, dx, dx_scratch, dx_scratch_floats};
    Replica r;
    TRY(check_item(d, base_item(it), true, (hipStream_t)stream, __func__, -1, &r));
    TRY(check_item_dx(it, __func__, -1, &r));
    return run_backward(&r, 1, SINGLE);
}

int rsaf_cnnlstm_train_group_max(void) { return RSAF_CNNLSTM_GROUP_MAX; }

int rsaf_cnnlstm_train_forward_group(const rsaf_cnnlstm_train_item* items_host, int K, int input_dim, int channels, int hidden,
                                     int num_classes, int lstm_layers, int act, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, act};
    Replica reps[RSAF_CNNLSTM_GROUP_MAX];
    TRY(check_group(d, items_host, K, false, (hipStream_t)stream, __func__, reps));
    return run_forward(reps, K, GROUPED);
}

int rsaf_cnnlstm_train_backward_group(const rsaf_cnnlstm_train_item* items_host, int K, int input_dim, int channels, int hidden,
                                      int num_classes, int lstm_layers, int act, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, act};
    Replica reps[RSAF_CNNLSTM_GROUP_MAX];
    TRY(check_group(d, items_host, K, true, (hipStream_t)stream, __func__, reps));
    return run_backward(reps, K, GROUPED);
}

int rsaf_cnnlstm_train_backward_group_dx(const rsaf_cnnlstm_train_dx_item* items_host, int K, int input_dim, int channels, int hidden,
                                         int num_classes, int lstm_layers, int act, rsaf_stream_t stream) {
    Dims d{input_dim, channels, hidden, num_classes, lstm_layers, act};
    Replica reps[RSAF_CNNLSTM_GROUP_MAX];
    TRY(check_group_dx(&d, items_host, nullptr, K, input_dim, num_classes, lstm_layers, (hipStream_t)stream, __func__, reps));
    return run_backward(reps, K, GROUPED);
}

int rsaf_cnnlstm_train_forward_group_mixed(const rsaf_cnnlstm_train_item* items_host, const rsaf_cnnlstm_arch* arch_host, int K,
                                           int input_dim, int num_classes, int lstm_layers, rsaf_stream_t stream) {
    Replica reps[RSAF_CNNLSTM_GROUP_MAX];
    TRY(check_group_mixed(items_host, arch_host, K, input_dim, num_classes, lstm_layers, false, (hipStream_t)stream, __func__, reps));
    return run_forward(reps, K, MIXED);
}

int rsaf_cnnlstm_train_backward_group_mixed(const rsaf_cnnlstm_train_item* items_host, const rsaf_cnnlstm_arch* arch_host, int K,
                                            int input_dim, int num_classes, int lstm_layers, rsaf_stream_t stream) {
    Replica reps[RSAF_CNNLSTM_GROUP_MAX];
    TRY(check_group_mixed(items_host, arch_host, K, input_dim, num_classes, lstm_layers, true, (hipStream_t)stream, __func__, reps));
    return run_backward(reps, K, MIXED);
}

int rsaf_cnnlstm_train_backward_group_mixed_dx(const rsaf_cnnlstm_train_dx_item* items_host, const rsaf_cnnlstm_arch* arch_host, int K,
                                               int input_dim, int num_classes, int lstm_layers, rsaf_stream_t stream) {
    Replica reps[RSAF_CNNLSTM_GROUP_MAX];
    TRY(check_group_dx(nullptr, items_host, arch_host, K, input_dim, num_classes, lstm_layers, (hipStream_t)stream, __func__, reps));
    return run_backward(reps, K, MIXED);
}

}  // extern "C"
