// Wav2Vec2 forward, encoder: LayerNorm (ln), attention (fused on the fp16 matrix pipe, or three launches), WavLM's bias gate
// and the encoder layers; the kernels, then the Forward phases that launch them.
#include "w2v2_forward.h"
#include "attn_softmax.h"

namespace rsaf {
namespace w2v2 {

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
//   * the score tile's register layout is an operand of the second product (element j of lane half h = key 16 s + 8 (j >> 2)
//     + 4 h + (j & 3)), P = e * 2^14 split into hi + lo, e = exp(s - max) un-normalised (attn_softmax.h: the maximum on the
//     raw accumulators, one fma into a base-2 argument, the bare v_exp_f32, a three-instruction split of two elements); the V
//     fragment (the same key order) comes out of row-major V by two ds_read_b64_tr_b16 (4 keys x 16 columns per 16-lane
//     group, delivered column-major), V chunks swizzled by ((row >> 1) & 1) << 2 so that the four rows of a transposed
//     read sit on disjoint banks; the fragments of a step are requested one step ahead (counted lgkmcnt);
//   * the second product is O^T = V^T P^T (V the A operand): the query stays on the lane, so acc / sum is in-lane, already
//     in the window's scale, and leaves as the plane pair of the out-projection's A operand in 16-byte stores.
// Matrix cycles: 192 MFMAs of 32 cycles per wave against 512 of 64 on the fp32 pipe.
// The grid is one-dimensional: attn::wg_slot gives the two query halves of a (window, head) ids 8 apart, so that they run on
// one XCD at the same time and K / V come from HBM once (they were fetched twice: 6.9 GB per launch of 2 000 windows).
// RELPOS (WavLM, REL_POS_BIAS): score(q, key) += gate[q][head] * tab[head][key - q].  The head's table over |key - q| <= 255
// (511 floats of reltab, 2 KB of static LDS beside the 64 KB of K / V blocks: still two workgroups per CU) is staged once per
// workgroup; a lane loads its query's gate once and reads tab at (255 - q) + key: the keys of a lane are compile-time
// offsets, and the 32 queries of a half-wave read 32 consecutive words (no bank conflict).  The plain instance reads neither
// of the two trailing arguments and keeps its code.
using ah8 = __attribute__((ext_vector_type(8))) _Float16;
typedef short atr4 __attribute__((__vector_size__(4 * sizeof(short))));
typedef short atr8 __attribute__((__vector_size__(8 * sizeof(short))));
typedef unsigned au4 __attribute__((ext_vector_type(4)));

// max(a, b, c): one v_max3_f32
__device__ __forceinline__ float attn_max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
// lanes 32-63 of a change places with lanes 0-31 of b
__device__ __forceinline__ void attn_swap32(unsigned& a, unsigned& b) {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}

// The transposed V fragments of one P V step (16 keys x 32 columns, both planes): [hi keys 0-7 | hi keys 8-15 | lo | lo] of
// the lane's address `a` plus immediates.  The reads stay asm (hipcc 7.2 has no builtin for them) and volatile, which keeps
// them in program order among themselves and behind the barrier that publishes the staged block; they carry no memory
// clobber, so the vector work of the next probabilities is free to move across them.  Their results are not valid before
// attn_v_wait has passed them through: the wait is counted, LEFT = the reads issued after these four (LDS returns in order).
template <int OFF>
__device__ __forceinline__ void attn_v_issue(unsigned a, atr4 (&f)[4]) {
    constexpr int LO = attn::V_LO, ROWS8 = attn::V_ROWS8;                       // bytes: to the lo plane, to 8 keys further
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f[0]) : "v"(a), "n"(OFF));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f[1]) : "v"(a), "n"(OFF + ROWS8));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f[2]) : "v"(a), "n"(OFF + LO));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f[3]) : "v"(a), "n"(OFF + LO + ROWS8));
}
template <int LEFT>
__device__ __forceinline__ void attn_v_wait(atr4 (&f)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]) : "n"(LEFT));
}

// One of the 16 steps of a 128-key block B of O^T += V^T P^T: STEP = 4 t4 + 2 s2 + ct is key tile t4 (32 keys), k-step s2 (16
// keys: elements 8 s2 .. 8 s2 + 7 of the score tile) and column tile ct (32 of the 64 columns).  The probabilities of a k-step
// are made in front of its first column tile; the fragments of step STEP + 1 are requested before this step waits for its own.
template <int B, int STEP>
__device__ __forceinline__ void attn_pv_step(const af32x16 (&sc)[8], float m, float c2, unsigned va, float& sum0, float& sum1,
                                             unsigned (&ph)[4], unsigned (&pl)[4], atr4 (&vf)[2][4], af32x16& o0, af32x16& o1) {
    constexpr int t4 = STEP >> 2, s2 = (STEP >> 1) & 1, ct = STEP & 1, kt = 4 * B + t4;
    if constexpr (ct == 0) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float e0 = attn::exp2_bare(attn::exp2_arg(sc[kt][8 * s2 + 2 * w], m, c2));
            const float e1 = attn::exp2_bare(attn::exp2_arg(sc[kt][8 * s2 + 2 * w + 1], m, c2));
            sum0 += e0;
            sum1 += e1;
            // (v_ldexp_f32: as multiplies the compiler pairs them into packed-fp32 instructions plus the moves that line their
            // operands up, which cost more beside MFMAs than they save)
            attn::split2(__builtin_ldexpf(e0, attn::P_SHIFT), __builtin_ldexpf(e1, attn::P_SHIFT), ph[w], pl[w]);
        }
    }
    if constexpr (STEP + 1 < 16) attn_v_issue<attn::v_step_bytes(STEP + 1)>(((STEP + 1) & 1) ? va ^ 64u : va, vf[(STEP + 1) & 1]);
    attn_v_wait<(STEP + 1 < 16) ? 4 : 0>(vf[STEP & 1]);
    // (whole-vector moves: rebuilding the fragments element by element from the 4-element results,
    // `vh[j] = bit_cast(th0[j])`, came out of hipcc 7.2 as a broadcast of element 0)
    const ah8 vh = __builtin_bit_cast(ah8, __builtin_shufflevector(vf[STEP & 1][0], vf[STEP & 1][1], 0, 1, 2, 3, 4, 5, 6, 7));
    const ah8 vl = __builtin_bit_cast(ah8, __builtin_shufflevector(vf[STEP & 1][2], vf[STEP & 1][3], 0, 1, 2, 3, 4, 5, 6, 7));
    const ah8 p_hi = __builtin_bit_cast(ah8, au4{ph[0], ph[1], ph[2], ph[3]});
    const ah8 p_lo = __builtin_bit_cast(ah8, au4{pl[0], pl[1], pl[2], pl[3]});
    af32x16& o = ct == 0 ? o0 : o1;
    o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, p_lo, o, 0, 0, 0);
    o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, p_hi, o, 0, 0, 0);
    o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, p_hi, o, 0, 0, 0);
}
template <int B, int... STEP>
__device__ __forceinline__ void attn_pv_block(std::integer_sequence<int, STEP...>, const af32x16 (&sc)[8], float m, float c2, unsigned va,
                                              float& sum0, float& sum1, unsigned (&ph)[4], unsigned (&pl)[4], atr4 (&vf)[2][4],
                                              af32x16& o0, af32x16& o1) {
    attn_v_issue<attn::v_step_bytes(0)>(va, vf[0]);
    (attn_pv_step<B, STEP>(sc, m, c2, va, sum0, sum1, ph, pl, vf, o0, o1), ...);
}

template <bool RELPOS>
__global__ __launch_bounds__(256, 2) void attn_f16x3_kernel(const unsigned short* __restrict__ qkvp, int64_t in_plane,
                                                            unsigned short* __restrict__ planes, int64_t plane_stride,
                                                            int64_t n_rows, const int* __restrict__ Tw,
                                                            const int64_t* __restrict__ row0, int NH, int Hd, float scale,
                                                            const float* __restrict__ row_scale,
                                                            const float* __restrict__ gate, const float* __restrict__ reltab,
                                                            int64_t pairs, int halves) {
    constexpr int HD = AttnLds::HD, KB = AttnLds::KB, PLANE = AttnLds::PLANE;    // one staged block: 2 planes x 16 KB (halfs)
    extern __shared__ __attribute__((aligned(1024))) unsigned short kvh[];      // two blocks
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const attn::WgSlot slot = attn::wg_slot(blockIdx.x, halves);                 // (window x head, query half)
    if (slot.pair >= pairs) return;                                             // padding of the last group of 16 ids
    const int win = (int)(slot.pair / NH), head = (int)(slot.pair - (int64_t)win * NH), qhalf = slot.half;
    const int T = Tw[win];
    if (qhalf * 128 >= T) return;                                               // (workgroup-uniform)
    const int64_t wrow0 = row0[win];
    const int64_t ld = 3 * (int64_t)Hd;                                         // halfs per row of a plane
    const unsigned short* base = qkvp + wrow0 * ld + (int64_t)head * HD;       // q of this window and head, plane 0
    const int q0 = qhalf * 128 + wv * 32;
    const int nblk = (T + KB - 1) / KB;                                         // 1 or 2 key blocks
    const float sw = row_scale[wrow0];                                          // the window's power of two
    const float sinv = pow2_inverse(sw);
    float qgate = 0.0f;                                                         // RELPOS: this lane's query
    const float* qtab = nullptr;                                                //         tab[key - q] = qtab[key]
    if constexpr (RELPOS) {
        __shared__ float tabs[512];
        for (int i = tid; i < 511; i += 256) tabs[i] = reltab[(int64_t)head * REL_TAB + (REL_SPAN - 256) + i];   // d = i - 255
        const int q = qhalf * 128 + wv * 32 + l31;                               // <= 255 (published by the first drain())
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
    unsigned short* buf0 = kvh + AttnLds::BLOCK0;
    unsigned short* buf1 = kvh + AttnLds::BLOCK1;

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
    // ---- softmax over the keys of this lane's query: key = 32 kt + (e & 3) + 8 (e >> 2) + 4 h (attn_softmax.h) ----
    // Pass 1, the row maximum: on the raw accumulators (sscale > 0 commutes with the max; RELPOS: on the biased scores, which
    // replace them), two elements per v_max3_f32.  Only a tile that reaches beyond T holds keys to mask: a wave-uniform test.
    const float sscale = scale * sinv * sinv;                                   // q and k both carry s_w
    const float c2 = RELPOS ? attn::LOG2E : attn::exp2_scale(sscale);
    float m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
        if (kt < 4 * nblk) {                                                    // (wave-uniform)
            if constexpr (RELPOS) {                                             // (the table read is unconditional: in bounds for every key)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    sc[kt][e] = fmaf(qgate, qtab[32 * kt + (e & 3) + 8 * (e >> 2) + 4 * h], sc[kt][e] * sscale);
            }
            if (32 * kt + 32 > T) {
                asm volatile("; tile with keys to mask");                       // (keeps the branch: as selects this costs every tile two instructions per score)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (4 * h >= T - (32 * kt + (e & 3) + 8 * (e >> 2))) sc[kt][e] = -INFINITY;   // key >= T
            }
#pragma unroll
            for (int e = 0; e < 16; e += 4) {
                m0 = attn_max3(m0, sc[kt][e], sc[kt][e + 1]);
                m1 = attn_max3(m1, sc[kt][e + 2], sc[kt][e + 3]);
            }
        }
    }
    float m = fmaxf(m0, m1);
    m = fmaxf(m, __shfl_xor(m, 32, 64));

    // ---- O^T = V^T P^T, P = 2^((s - m) c2) 2^14 formed tile by tile in front of the MFMAs that consume it ----
    // (V^T is the A operand, P^T the B operand: the fragments are the ones P V would take, the operands change places, and
    // the accumulator comes out with the QUERY on the lane, as the scores do: the row sum and its reciprocal stay in-lane, and
    // a lane's registers hold four consecutive columns of its query's output row.)
    af32x16 o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.0f; o1[e] = 0.0f; }
    float sum0 = 0.0f, sum1 = 0.0f;
    // transposed-read addressing (attn_softmax.h): the step, the + 8 keys, the plane and the column tile (chunk bit 2:
    // address ^ 64) are immediates on ONE lane address per block
    static_assert(attn::V_HD == HD && attn::V_KB == KB, "attn_softmax.h restates the staged block");
    const unsigned vlane = (unsigned)attn::v_lane_bytes(lane);
    unsigned short* v0buf = nblk == 1 ? buf1 : buf0;
    unsigned short* v1buf = nblk == 1 ? buf0 : buf1;
    unsigned ph[4], pl[4];
    atr4 vf[2][4];
    {
        // V block 0 is where the score phase left it; V1 goes to the other buffer while V0 is multiplied
        if (nblk > 1) stage(2 * Hd, KB, v1buf, true);
        const unsigned va = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const unsigned short*)v0buf + vlane;
        attn_pv_block<0>(std::make_integer_sequence<int, 16>{}, sc, m, c2, va, sum0, sum1, ph, pl, vf, o0, o1);
    }
    if (nblk > 1) {
        drain();
        const unsigned va = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const unsigned short*)v1buf + vlane;
        attn_pv_block<1>(std::make_integer_sequence<int, 16>{}, sc, m, c2, va, sum0, sum1, ph, pl, vf, o0, o1);
    }
    float sum = sum0 + sum1;
    sum += __shfl_xor(sum, 32, 64);
    const float rinv = 1.0f / (sum * attn::P_SCALE);                            // the normalisation, and the 2^14 of P taken back

    // C layout of O^T: column = lane & 31 (query within the wave's 32), row = (e & 3) + 8 (e >> 2) + 4 h (d within the column
    // tile).  acc / sum = o * s_w: already the out-projection's A operand in the window's scale (|o| <= max |v| of the window,
    // and v * s_w < 2^15).  k16 panels of n_rows rows (gemm_f16x3.h): column head * 64 + d -> panel 4 head + (d >> 4),
    // k = d & 15.  Registers 8 gp .. 8 gp + 7 of tile ct are k = 4 h + {0..3} and 8 + 4 h + {0..3} of panel 2 ct + gp: the
    // two halves of the wave exchange one of the two groups (v_permlane32_swap), after which lane h holds k = 8 h .. 8 h + 7,
    // 16 bytes per plane, and a wave instruction writes 32 rows x 32 bytes = 1 KB of a panel without a gap.
    const int q = q0 + l31;
    const int64_t panel_sz = n_rows * 16;
    unsigned short* op = planes + (int64_t)(head * 4) * panel_sz + (wrow0 + q) * 16 + attn::store_k0(lane);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            unsigned hi[4], lo[4];                                              // [k = 4 h ..: 2 words][k = 8 + 4 h ..: 2 words]
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int e = 8 * gp + 2 * w;
                attn::split2((ct == 0 ? o0[e] : o1[e]) * rinv, (ct == 0 ? o0[e + 1] : o1[e + 1]) * rinv, hi[w], lo[w]);
            }
            // lower half keeps k 0..3 and takes k 4..7 from the upper one, which takes k 8..11 and keeps k 12..15
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                attn_swap32(hi[w], hi[w + 2]);
                attn_swap32(lo[w], lo[w + 2]);
            }
            if (q < T) {
                unsigned short* d0 = op + (int64_t)attn::store_panel(ct, gp) * panel_sz;
                *reinterpret_cast<uint4*>(d0) = uint4{hi[0], hi[1], hi[2], hi[3]};
                *reinterpret_cast<uint4*>(d0 + plane_stride) = uint4{lo[0], lo[1], lo[2], lo[3]};
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

int ln(const LnArgs& a, int64_t rows, int D, float eps, hipStream_t s) {
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

// The LayerNorm between two q/k/v projections: LN(src (+ res)) under g / b, fp32 rows into dst (x, the att buffer for the
// gates, the call's `out`, or none), hidden_states[k] into its tap.
// next: layer k follows and reads the planes in W.xp under the scales in W.s_x (fused attention: this LayerNorm also reports
// the window's largest row norm, behind the scale of that layer's q / k / v).  Else dst is `out`: frame t of window w at
// row out_row_start[w] + t (or packed, window after window).
// The tap takes this LayerNorm's output, except in the PRE_LN flow while a layer follows: there hidden_states[k] is the
// un-normalised residual stream h that this LayerNorm reads.  sum (PRE_LN after the positional conv): src + res goes there.
int Forward::ln_to_qkv(const float* src, const float* res, const float* g, const float* b, float* dst, int k, bool next,
                       float* sum) {
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
int Forward::qkv_projection(int l) {
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
int Forward::attention() { return fused ? (relpos ? attention_fused<true>() : attention_fused<false>()) : attention_three_launch(); }
template <bool RP>
int Forward::attention_fused() {
    // 2 x 2 T^2 hd flops per (chunk, head)
    double att_flops = 0.0;
    for (const auto& tg : R.tgroups) att_flops += 4.0 * (tg.second - tg.first) * c.NH * (double)R.T6[tg.first] * R.T6[tg.first] * hd;
    ProfScope prof("w2v2_attn_fused", s, att_flops, 0.0);
    RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)attn_f16x3_kernel<RP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AttnLds::bytes()));
    const int64_t pairs = (int64_t)n * c.NH;                                    // (window, head); one workgroup per query half of each
    const int halves = (Tt + 127) / 128;
    hipLaunchKernelGGL(attn_f16x3_kernel<RP>, dim3((unsigned)attn::grid_size(pairs, halves)), dim3(256), AttnLds::bytes(), s,
                       planes_at(W.qkv), rows * 3 * Hd, planes_at(W.attp), rows * Hd, rows, Tw + (int64_t)6 * n, row0, c.NH, Hd, scale,
                       ws + W.s_qkv, gate(), reltab(), pairs, halves);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}
// three launches per run of equal windows (head widths other than 64: test geometries), then the planes of the result
// (the fused kernel writes them itself)
int Forward::attention_three_launch() {
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
int Forward::out_projection(int l) {
    Out o;
    o.Cf = ws + W.y; o.bias = Wt + L.layers[l].bo; o.R = x;
    return gemm3(rows_a(W.attp, Hd, fused ? ws + W.s_qkv : ws + W.s_att), weights_b(W.wp_o[l], W.ws_o[l]), o, (int)rows, Hd, Hd);
}
// LN(y) under g / b as the planes the feed forward reads, with the bound behind the scale of the ffn1 output; fp32 rows
// into dst (or none)
int Forward::ln_to_ffn(int l, const float* g, const float* b, float* dst) {
    const int b0 = WSTAT_LAYER0 + WSTAT_PER_LAYER * l;
    LnArgs a;
    a.x = ws + W.y; a.g = g; a.b = b; a.out = dst;
    a.planes = planes_at(W.xp); a.panel = true; a.scale_out = ws + W.s_x;
    a.bound_w = wstat(b0 + 2); a.bound_b = wstat(b0 + 4); a.bound_scale_out = ws + W.s_ffn;
    return ln(a, rows, Hd, c.eps, s);
}
// dst = GELU(xp W1^T + b1) W2^T + b2 + res; the GELU output only exists as planes (A of the second GEMM)
int Forward::feed_forward(int l, float* dst, const float* res) {
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
int Forward::layer_post_ln(int l) {
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
int Forward::layer_pre_ln(int l) {
    const LayerOff& lo = L.layers[l];
    RSAF_TRY(out_projection(l));
    RSAF_TRY(ln_to_ffn(l, Wt + lo.ln2g, Wt + lo.ln2b, nullptr));
    RSAF_TRY(feed_forward(l, x, ws + W.y));
    if (l == c.L - 1) return ln_to_qkv(x, nullptr, Wt + L.elng, Wt + L.elnb, out, l + 1, false);
    const LayerOff& nx = L.layers[l + 1];
    return ln_to_qkv(x, nullptr, Wt + nx.ln1g, Wt + nx.ln1b, gate_rows(), l + 1, true);
}
int Forward::encoder_layer(int l) {
    RSAF_TRY(qkv_projection(l));
    RSAF_TRY(attention());
    return pre_ln ? layer_pre_ln(l) : layer_post_ln(l);
}

}  // namespace w2v2
}  // namespace rsaf
