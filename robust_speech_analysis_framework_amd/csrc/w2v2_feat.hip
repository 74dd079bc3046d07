// Wav2Vec2 forward, first stage: window tables, per-window normalisation, the seven feature-encoder convolutions (group-norm
// and layer-norm mode) and the feature projection; the kernels, then the Forward phases that launch them.
#include "w2v2_forward.h"
#include "gn_stats.h"

namespace rsaf {
namespace w2v2 {

// Tw[i][w], row0, the packed-output offsets and the row -> window map from the device copy of the lengths
__global__ __launch_bounds__(256) void w2v2_tables_kernel(const int* __restrict__ len, int n, int C, int Hd, int* __restrict__ Tw,
                                                          int64_t* __restrict__ row0, int64_t* __restrict__ ztab) {
    for (int w = threadIdx.x; w < n; w += 256) {
        int m = len[w];
        for (int i = 0; i < 7; ++i) { m = m >= KERN[i] ? (m - KERN[i]) / STRD[i] + 1 : 0; Tw[(int64_t)i * n + w] = m; }
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
                gn::slab_add(y, s[k], q[k], mx[k]);
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

// GroupNorm coefficients per (window, channel) and the window's bound: |GELU(a y + b)| <= |a| max|y| + |b|.  The moments come
// from the slabs' float sums where those suffice (gn_stats.h); a channel whose mean outweighs its spread is summed again here,
// in double, over its recomputed conv0 outputs (the FMA order of conv0_kernel: the y the apply pass will see).
// xn, len: the windows' samples and their stride; cb: the conv bias or NULL
__global__ __launch_bounds__(256) void gn_finalize_kernel(const float* __restrict__ part, const float* __restrict__ g,
                                                          const float* __restrict__ be, float* __restrict__ ab,
                                                          unsigned* __restrict__ amax, int n, int C, int slabs,
                                                          const int* __restrict__ T0w, const float* __restrict__ xn, int len,
                                                          const float* __restrict__ w0, const float* __restrict__ cb) {
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
    gn::Moments m = gn::moments_of_sums(s, q, T0);
    if (!gn::sums_suffice(m)) {
        const float* __restrict__ x = xn + (int64_t)chunk * len;
        float wr[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) wr[j] = w0[c * 10 + j];
        const float bi = cb ? cb[c] : 0.f;
        gn::Sums64 acc;
        for (int t = 0; t < T0; ++t) {
            float y = 0.f;
#pragma unroll
            for (int j = 0; j < 10; ++j) y = fmaf(wr[j], x[5 * t + j], y);
            if (cb) y += bi;
            acc.add(y);
        }
        m = gn::moments_of_sums(acc.s, acc.q, T0);
    }
    float af, bf;
    gn::coefficients(m, g[c], be[c], af, bf);
    ab[((int64_t)chunk * 2 + 0) * C + c] = af;
    ab[((int64_t)chunk * 2 + 1) * C + c] = bf;
    atomicMax(amax + chunk, __float_as_uint((fabsf(af) * mx + fabsf(bf)) * 1.000001f));
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

// window tables; len_dev NULL (equal windows): the length table is filled here
int Forward::window_tables(const int* len_dev) {
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

// 1-3. feature encoder, G windows at a time (its activations are the large ones: 15 999 x 512 per window)
int Forward::feature_encoder() {
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
int Forward::conv_gemm(int i, const uint16_t* a_planes, Out& o, int g0, int g, const int* Tg) {
    if (i == 6) { o.Cf = ws + W.c6; o.sC = 0; }
    o.bias = conv_bias ? cbias + (int64_t)i * C : nullptr;
    return gemm3(conv_a(a_planes, i), weights_b(W.wp_conv[i - 1], W.ws_conv[i - 1]), o, Tg[i], C, KERN[i] * C, g,
                 ztab + ((int64_t)(i - 1) * n + g0) * 2);
}
// 2-3 (layer mode). conv0 + LayerNorm + GELU in one pass; conv1..6 as GEMMs writing fp32 rows (+ bias) into the Q buffer,
// then LayerNorm -> GELU -> planes back into P (the GEMM has consumed them); conv6 writes its packed rows, and its
// LayerNorm + GELU join the feature projection's LayerNorm (step 4)
int Forward::convs_layer_norm(int g0, int g, const int* Tg) {
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
int Forward::convs_group_norm(int g0, int g, const int* Tg) {
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
                       Wt + L.gng, Wt + L.gnb, ws + W.ab, camax, g, C, slabs_g, Tw + g0, ws + W.xn, R.maxlen, Wt + L.conv0, cbias);
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
int Forward::feature_projection() {
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

}  // namespace w2v2
}  // namespace rsaf
