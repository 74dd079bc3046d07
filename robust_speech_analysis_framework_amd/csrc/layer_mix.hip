// Learned mix of encoder layers on gfx950: x[b,t,:] = sum_l p[l] h[b,l,t,:] and the gradient of the loss with respect to p
// (rsaf_layer_mix_forward / _backward, include/rsaf.h).  Both are streams over h, L + 1 times the size of x, so each reads h
// once with float4 loads and touches x / dx once per position; the softmax over the L weights and its Jacobian are the
// caller's.  Addressing, the partition of the backward and the order of its sums: layer_mix_layout.h.
//
// rsaf_collate_mix_group / rsaf_collate_mix_backward_group are the same two streams over layer stacks that stay resident in a
// DeviceSequenceStore arena: the mixed, padded batch comes straight out of the collate launch and dL/dp straight from the
// resident blocks and the step's dx, so the padded stack [B][L][T][D] never exists.  rsaf_layer_mix_adam_group is the step
// of the L weights (softmax Jacobian, Adam, next softmax), one wave per item.
#include <cmath>

#include "cnnlstm_host.h"       // TRY, fail, check_group_args (the group entries' checks)
#include "layer_mix_layout.h"
#include "rsaf_common.h"

namespace rsaf {
namespace layermix {

__global__ __launch_bounds__(MIX_THREADS) void layer_mix_fwd_kernel(const float4* __restrict__ h, const float* __restrict__ p,
                                                                    float4* __restrict__ x, Parts P, int L) {
    for (int64_t i = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x; i < P.n4; i += (int64_t)gridDim.x * MIX_THREADS) {
        const float4* hi = h + h_index(P, L, i, 0);
        float4 a;
        mix_term(a, p[0], hi[0], true);                                           // L = 1, p = [1]: the bits of h
#pragma unroll 4
        for (int l = 1; l < L; ++l) mix_term(a, p[l], hi[(int64_t)l * P.td4], false);
        x[i] = a;
    }
}

// one part of the positions per workgroup; LB: L rounded up to 4, 8, 16 or 32 so that the L sums stay in registers
template <int LB>
__global__ __launch_bounds__(MIX_THREADS) void layer_mix_bwd_partial_kernel(const float4* __restrict__ h, const float4* __restrict__ dx,
                                                                            double* __restrict__ partials, Parts P, int L) {
    const int64_t i0 = (int64_t)blockIdx.x * P.per, i1 = min(P.n4, i0 + P.per);
    double acc[LB];
#pragma unroll
    for (int l = 0; l < LB; ++l) acc[l] = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += MIX_THREADS) {
        const float4 g = dx[i];
        const float4* hi = h + h_index(P, L, i, 0);
#pragma unroll
        for (int l = 0; l < LB; ++l)
            if (l < L) {                                  // uniform
                const float4 v = hi[(int64_t)l * P.td4];
                double s = acc[l];
                s += (double)v.x * (double)g.x; s += (double)v.y * (double)g.y;
                s += (double)v.z * (double)g.z; s += (double)v.w * (double)g.w;
                acc[l] = s;
            }
    }
    __shared__ double sh[MIX_THREADS / 64][LB];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int l = 0; l < LB; ++l) {
        const double s = wave_sum_f64(acc[l]);
        if (lane == 0) sh[w][l] = s;
    }
    __syncthreads();
    if (threadIdx.x < L) partials[(int64_t)blockIdx.x * L + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// one wave per layer: lane j adds parts j, j + 64, ... in ascending order
__global__ __launch_bounds__(MIX_THREADS) void layer_mix_bwd_final_kernel(const double* __restrict__ partials, int64_t parts, int L,
                                                                          float* __restrict__ dp) {
    const int lane = threadIdx.x & 63, l = blockIdx.x * (MIX_THREADS / 64) + (threadIdx.x >> 6);
    if (l >= L) return;                                   // whole waves leave; no barrier follows
    double s = 0.0;
    for (int64_t q = lane; q < parts; q += 64) s += partials[q * L + l];
    s = wave_sum_f64(s);
    if (lane == 0) dp[l] = (float)s;
}

// ---- rsaf_collate_mix_group: the mix inside the collate launch --------------------------------------------------------
// Grid and member geometry as in collate_pad_group_kernel (aggregate.hip): the workgroups of all items back to back, each
// one chunk of MIXC_CHUNK consecutive float4 of one member's out.  A member's frames that exist are one contiguous run per
// layer, `stride` float4 apart, so nothing is divided per element.
struct MixcItem {
    const float4* arena;
    const long long* row_start;
    const int* row_count;
    const float* p;
    float4* out;
    const long long* label_src;
    const long long* label_index;
    long long* label_out;
    long long arena_rows, label_count;
    unsigned first_block;          // of this item in the grid
    unsigned blocks_per_member;    // mix_chunks(T, width)
    int B, T, L;
};
struct MixcGroup {
    MixcItem item[RSAF_CNNLSTM_GROUP_MAX];
    int K, w4;                     // w4: float4 of a row
};
static_assert(sizeof(MixcGroup) <= 3584, "the descriptors travel by value in the kernel arguments");

// layers l0 .. l0 + MIXC_LAYERS_IN_FLIGHT of the lane's positions: all loads, then the terms in ascending l
template <bool FIRST>
__device__ __forceinline__ void mix_layers(float4 (&a)[MIXC_PER_THREAD], const bool (&in)[MIXC_PER_THREAD], const float4* __restrict__ src,
                                           const float* __restrict__ p, int64_t stride, int64_t e0, int l0, int L) {
    float4 v[MIXC_LAYERS_IN_FLIGHT][MIXC_PER_THREAD];
    float pl[MIXC_LAYERS_IN_FLIGHT];
#pragma unroll
    for (int i = 0; i < MIXC_LAYERS_IN_FLIGHT; ++i)
        if (l0 + i < L) {                                 // uniform
            pl[i] = p[l0 + i];
#pragma unroll
            for (int j = 0; j < MIXC_PER_THREAD; ++j)
                if (in[j]) v[i][j] = src[(int64_t)(l0 + i) * stride + e0 + j * MIX_THREADS];
        }
#pragma unroll
    for (int i = 0; i < MIXC_LAYERS_IN_FLIGHT; ++i)
        if (l0 + i < L) {
#pragma unroll
            for (int j = 0; j < MIXC_PER_THREAD; ++j)
                if (in[j]) mix_term(a[j], pl[i], v[i][j], FIRST && i == 0);
        }
}

__global__ __launch_bounds__(MIX_THREADS) void collate_mix_group_kernel(const MixcGroup g) {
    int k = 0;
    while (k + 1 < g.K && blockIdx.x >= g.item[k + 1].first_block) ++k;
    const MixcItem& it = g.item[k];
    const unsigned blk = blockIdx.x - it.first_block;
    const unsigned b = blk / it.blocks_per_member, chunk = blk - b * it.blocks_per_member;
    const int64_t start = it.row_start[b], own = it.row_count[b];
    const bool inside = block_inside(start, own, it.L, it.arena_rows);
    const int64_t n = inside ? min(own, (int64_t)it.T) : 0;                 // frames that are mixed
    const int64_t hi = n * g.w4, end = (int64_t)it.T * g.w4, stride = inside ? own * g.w4 : 0;
    const float4* src = it.arena + (inside ? start : 0) * g.w4;             // read at [l stride, l stride + hi) only
    float4* dst = it.out + (int64_t)b * end;
    const int64_t e0 = (int64_t)chunk * MIXC_CHUNK + threadIdx.x;
    float4 a[MIXC_PER_THREAD];
    bool in[MIXC_PER_THREAD];
#pragma unroll
    for (int j = 0; j < MIXC_PER_THREAD; ++j) {
        a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        in[j] = e0 + j * MIX_THREADS < hi;
    }
    mix_layers<true>(a, in, src, it.p, stride, e0, 0, it.L);
    for (int l0 = MIXC_LAYERS_IN_FLIGHT; l0 < it.L; l0 += MIXC_LAYERS_IN_FLIGHT) mix_layers<false>(a, in, src, it.p, stride, e0, l0, it.L);
#pragma unroll
    for (int j = 0; j < MIXC_PER_THREAD; ++j) {
        const int64_t e = e0 + j * MIX_THREADS;
        if (e < end) dst[e] = a[j];
    }
    if (blk == 0 && it.label_out) {
        for (int i = threadIdx.x; i < it.B; i += MIX_THREADS) {
            const long long j = it.label_index[i];
            it.label_out[i] = (j >= 0 && j < it.label_count) ? it.label_src[j] : -1LL;
        }
    }
}

// ---- rsaf_collate_mix_backward_group ----------------------------------------------------------------------------------
// layer_mix_bwd_partial_kernel over the padded shape of every item, reading the resident blocks: the same parts, the same
// lanes, the same order; a position whose frame does not exist adds nothing.  The part's first position is found by division
// once (uniform); a lane adds its offset and steps by MIX_THREADS float4 afterwards, in 32 bits (mix_first_pos / mix_step_pos).
struct MixbItem {
    const float4* arena;
    const long long* row_start;
    const int* row_count;
    const float4* dx;
    double* partials;
    float* dp_out;
    long long arena_rows;
    Parts P;                       // of the padded shape (B, L, T, width)
    unsigned first_block;
    int B, T, L;
};
struct MixbGroup {
    MixbItem item[RSAF_CNNLSTM_GROUP_MAX];
    int K, w4;
};
static_assert(sizeof(MixbGroup) <= 3584, "the descriptors travel by value in the kernel arguments");

// what a lane needs of the member it stands in: where layer 0 of its block starts, the float4 between layers, the frames read
struct MixMember {
    const float4* src;
    int64_t stride;
    uint32_t n;
};
__device__ __forceinline__ MixMember mix_member(const MixbItem& it, int64_t b, int64_t w4) {
    const int64_t start = it.row_start[b], own = it.row_count[b];
    const bool inside = block_inside(start, own, it.L, it.arena_rows);
    MixMember m;
    m.src = it.arena + (inside ? start : 0) * w4;
    m.stride = inside ? own * w4 : 0;
    m.n = inside ? (uint32_t)min(own, (int64_t)it.T) : 0u;
    return m;
}

template <int LB>
__global__ __launch_bounds__(MIX_THREADS) void collate_mix_bwd_partial_kernel(const MixbGroup g) {
    int k = 0;
    while (k + 1 < g.K && blockIdx.x >= g.item[k + 1].first_block) ++k;
    const MixbItem& it = g.item[k];
    const int64_t q = blockIdx.x - it.first_block;
    const int L = it.L;
    const uint32_t w4 = g.w4, T = it.T;
    const int64_t i0 = q * it.P.per, i1 = min(it.P.n4, i0 + it.P.per);
    // The part's first member and the one after it are looked up once per workgroup, ahead of everything else: the addresses
    // are uniform and no store precedes them, so they are scalar loads that do not queue behind the vector stream.  A per-lane
    // lookup in front of a lane's first arena load cost one dependent round trip per part (profiles/r29/).  A part that
    // reaches a third member (per > T width / 4) looks that one up per lane.
    int64_t b0;
    MixPos pos = mix_first_pos(it.P, w4, T, i0, threadIdx.x, &b0);
    const MixMember m0 = mix_member(it, b0, w4);
    MixMember m1 = m0;
    if (b0 + 1 < it.B) m1 = mix_member(it, b0 + 1, w4);
    double acc[LB];
#pragma unroll
    for (int l = 0; l < LB; ++l) acc[l] = 0.0;
    MixMember m = m0;
    uint32_t seen = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += MIX_THREADS) {
        if (pos.db != seen) {                             // b0 + db < B here: i < n4
            m = pos.db == 1 ? m1 : mix_member(it, b0 + pos.db, w4);
            seen = pos.db;
        }
        if (pos.t < m.n) {
            const float4 gq = it.dx[i];
            const float4* hi = m.src + (int64_t)pos.t * w4 + pos.c;
            // Four layers at a time, their loads issued together.  With a test of l < L per layer the compiler makes every layer a
            // branch of its own and waits for each load before the next is issued: one load in flight per wave, which is what
            // bounds the dense kernel (profiles/r29/).  A layer past L - 1 of a started group reads layer L - 1 again (the line
            // is in cache) into an accumulator that is never written out, so the sums of the layers that exist keep their
            // order and their bits.
#pragma unroll
            for (int l0 = 0; l0 < LB; l0 += MIXC_LAYERS_IN_FLIGHT)
                if (l0 < L) {                             // uniform
                    float4 v[MIXC_LAYERS_IN_FLIGHT];
#pragma unroll
                    for (int j = 0; j < MIXC_LAYERS_IN_FLIGHT; ++j) v[j] = hi[(int64_t)min(l0 + j, L - 1) * m.stride];
#pragma unroll
                    for (int j = 0; j < MIXC_LAYERS_IN_FLIGHT; ++j) {
                        double s = acc[l0 + j];
                        s += (double)v[j].x * (double)gq.x; s += (double)v[j].y * (double)gq.y;
                        s += (double)v[j].z * (double)gq.z; s += (double)v[j].w * (double)gq.w;
                        acc[l0 + j] = s;
                    }
                }
        }
        mix_step_pos(pos, w4, T);
    }
    __shared__ double sh[MIX_THREADS / 64][LB];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int l = 0; l < LB; ++l) {
        const double s = wave_sum_f64(acc[l]);
        if (lane == 0) sh[w][l] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < L) it.partials[q * L + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// one wave per (item, l), the waves of item k from wave0[k] on: layer_mix_bwd_final_kernel's sum
struct MixfGroup {
    const double* partials[RSAF_CNNLSTM_GROUP_MAX];
    float* dp[RSAF_CNNLSTM_GROUP_MAX];
    long long parts[RSAF_CNNLSTM_GROUP_MAX];
    int L[RSAF_CNNLSTM_GROUP_MAX], wave0[RSAF_CNNLSTM_GROUP_MAX];
    int K;
};

__global__ __launch_bounds__(MIX_THREADS) void collate_mix_bwd_final_kernel(const MixfGroup g) {
    const int lane = threadIdx.x & 63, wave = blockIdx.x * (MIX_THREADS / 64) + (threadIdx.x >> 6);
    int k = 0;
    while (k + 1 < g.K && wave >= g.wave0[k + 1]) ++k;
    const int l = wave - g.wave0[k], L = g.L[k];
    if (l >= L) return;                                   // whole waves leave; no barrier follows
    const double* partials = g.partials[k];
    double s = 0.0;
    for (int64_t q = lane; q < g.parts[k]; q += 64) s += partials[q * L + l];
    s = wave_sum_f64(s);
    if (lane == 0) g.dp[k][l] = (float)s;
}

// ---- rsaf_layer_mix_adam_group: one wave per item, lane l owns weight l --------------------------------------------------
struct MixAdamItem {
    const float* p;
    const float* dp;
    const float* dw;
    float* dw_out;
    float* w;
    float* m;
    float* v;
    float* p_next;
    double step_size, b1, b2, eps, inv_sqrt_bc2;          // as AdamRep of cnnlstm_optim.hip
    int L, mode;
};
struct MixAdamGroup {
    MixAdamItem item[RSAF_CNNLSTM_GROUP_MAX];
};
static_assert(sizeof(MixAdamGroup) <= 3584, "the descriptors travel by value in the kernel arguments");

__global__ __launch_bounds__(64) void layer_mix_adam_group_kernel(const MixAdamGroup g) {
    const MixAdamItem& it = g.item[blockIdx.x];
    const int lane = threadIdx.x;
    const bool live = lane < it.L;
    float wn = 0.0f;
    if (it.mode != RSAF_LAYER_MIX_SOFTMAX_ONLY) {
        float gq = 0.0f;
        if (it.mode == RSAF_LAYER_MIX_FROM_DP) {
            const double pd = live ? (double)it.p[lane] : 0.0, dd = live ? (double)it.dp[lane] : 0.0;
            const double s = wave_sum_f64(pd * dd);
            gq = (float)(pd * (dd - s));
            if (live && it.dw_out) it.dw_out[lane] = gq;
        } else if (live) {
            gq = it.dw[lane];
        }
        if (live) {                                       // adam_one of cnnlstm_optim.hip, unscaled
            const double gd = (double)gq;
            const double md = it.b1 * (double)it.m[lane] + (1.0 - it.b1) * gd;
            const double vd = it.b2 * (double)it.v[lane] + (1.0 - it.b2) * gd * gd;
            it.m[lane] = (float)md;
            it.v[lane] = (float)vd;
            wn = (float)((double)it.w[lane] - it.step_size * md / (sqrt(vd) * it.inv_sqrt_bc2 + it.eps));
            it.w[lane] = wn;
        }
    } else if (live) {
        wn = it.w[lane];
    }
    double mx = live ? (double)wn : -__builtin_huge_val();
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    const double e = live ? exp((double)wn - mx) : 0.0;
    const double s = wave_sum_f64(e);
    if (live) it.p_next[lane] = (float)(e / s);
}

static int check_shape(const Shape& s) {
    const char* problem = shape_problem(s);
    RSAF_CHECK_ARG(!problem, problem);
    return RSAF_OK;
}

static bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

using cnnlstm::check_group_args;
using cnnlstm::fail;

// what the forward and the backward item of the collate mix share: the arena, the members and B, T, L
template <typename ItemT>
static int check_mix_addressing(const ItemT& it, int k, int width, const char* who) {
    if (!(it.B >= 1 && it.T >= 1)) return fail(RSAF_ERR_ARG, who, k, "B and T must be >= 1");
    if (!(it.L >= 1 && it.L <= RSAF_LAYER_MIX_MAX)) return fail(RSAF_ERR_ARG, who, k, "num_layers must be in [1, 32] (RSAF_LAYER_MIX_MAX)");
    const int64_t bt = (int64_t)it.B * it.T;             // < 2^62; the product with width is never formed before it is known to fit
    if (!(bt < MIX_N_MAX && width <= (MIX_N_MAX - 1) / bt)) return fail(RSAF_ERR_ARG, who, k, "B * T * width must be < 2^40");
    if (!(it.arena && it.row_start && it.row_count)) return fail(RSAF_ERR_ARG, who, k, "NULL pointer");
    if (!(it.arena_rows >= 0)) return fail(RSAF_ERR_ARG, who, k, "arena_rows must be >= 0");
    return RSAF_OK;
}

template <typename ItemT>
static double counted_frames(const ItemT& it) {
    const int64_t all = (int64_t)it.B * it.T;
    return (double)(it.frames >= 0 && it.frames <= all ? it.frames : all);
}

}  // namespace layermix
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::layermix;

extern "C" {

int rsaf_layer_mix_forward(const float* h, int B, int L, int T, int D, const float* p, float* x, rsaf_stream_t stream) {
    const Shape s{B, L, T, D};
    if (int rc = check_shape(s)) return rc;
    RSAF_CHECK_ARG(h && p && x, "NULL pointer");
    RSAF_CHECK_ARG(al16(h) && al16(x), "h and x must be 16-byte aligned");
    const Parts P = make_parts(s);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("layer_mix_forward", st, 2.0 * P.n4 * 4 * L, (double)P.n4 * 16 * (L + 1));
    hipLaunchKernelGGL(layer_mix_fwd_kernel, dim3((unsigned)forward_blocks(P)), dim3(MIX_THREADS), 0, st,
                       reinterpret_cast<const float4*>(h), p, reinterpret_cast<float4*>(x), P, L);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int64_t rsaf_layer_mix_partials(int B, int L, int T, int D) {
    const Shape s{B, L, T, D};
    if (shape_problem(s)) return -1;
    return partials_doubles(s);
}

int rsaf_layer_mix_backward(const float* h, const float* dx, int B, int L, int T, int D, double* partials, int64_t partials_count,
                            float* dp_out, rsaf_stream_t stream) {
    const Shape s{B, L, T, D};
    if (int rc = check_shape(s)) return rc;
    RSAF_CHECK_ARG(h && dx && partials && dp_out, "NULL pointer");
    RSAF_CHECK_ARG(al16(h) && al16(dx), "h and dx must be 16-byte aligned");
    RSAF_CHECK_ARG((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "partials must be 8-byte aligned");
    const Parts P = make_parts(s);
    if (partials_count < P.parts * L) {
        set_error(std::string(__func__) + ": partials too small (rsaf_layer_mix_partials)");
        return RSAF_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("layer_mix_backward", st, 2.0 * P.n4 * 4 * L, (double)P.n4 * 16 * (L + 1));
    const float4* h4 = reinterpret_cast<const float4*>(h);
    const float4* g4 = reinterpret_cast<const float4*>(dx);
    const dim3 grid((unsigned)P.parts), block(MIX_THREADS);
    if (L <= 4) hipLaunchKernelGGL(layer_mix_bwd_partial_kernel<4>, grid, block, 0, st, h4, g4, partials, P, L);
    else if (L <= 8) hipLaunchKernelGGL(layer_mix_bwd_partial_kernel<8>, grid, block, 0, st, h4, g4, partials, P, L);
    else if (L <= 16) hipLaunchKernelGGL(layer_mix_bwd_partial_kernel<16>, grid, block, 0, st, h4, g4, partials, P, L);
    else hipLaunchKernelGGL(layer_mix_bwd_partial_kernel<32>, grid, block, 0, st, h4, g4, partials, P, L);
    hipLaunchKernelGGL(layer_mix_bwd_final_kernel, dim3((L + MIX_THREADS / 64 - 1) / (MIX_THREADS / 64)), block, 0, st, partials, P.parts, L,
                       dp_out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_collate_mix_group(const rsaf_collate_mix_item* items_host, int K, int width, rsaf_stream_t stream) {
    static_assert(sizeof(rsaf_collate_mix_item) == 104, "rsaf_collate_mix_item is part of the ABI (CollateMixItem of _lib.py)");
    TRY(check_group_args(K, items_host, __func__));
    if (!(width >= 4 && width % 4 == 0)) return fail(RSAF_ERR_ARG, __func__, -1, "width must be a positive multiple of 4");
    MixcGroup g{};
    g.K = K;
    g.w4 = width / 4;
    cnnlstm::WrittenRanges wrote;
    int64_t blocks = 0;
    double floats = 0.0;
    for (int k = 0; k < K; ++k) {
        const rsaf_collate_mix_item& it = items_host[k];
        TRY(check_mix_addressing(it, k, width, __func__));
        if (!(it.p && it.out)) return fail(RSAF_ERR_ARG, __func__, k, "NULL pointer");
        if (!(al16(it.arena) && al16(it.out))) return fail(RSAF_ERR_ARG, __func__, k, "arena and out must be 16-byte aligned");
        const int n_label = (it.label_src != nullptr) + (it.label_index != nullptr) + (it.label_out != nullptr);
        if (!(n_label == 0 || n_label == 3) || (n_label == 0 && it.label_count != 0) || it.label_count < 0)
            return fail(RSAF_ERR_ARG, __func__, k, "label_src, label_count, label_index and label_out go together: all or none");
        const int64_t out_floats = (int64_t)it.B * it.T * width;
        TRY(wrote.add(it.out, out_floats * 4, k, "out", __func__));
        TRY(wrote.add(it.label_out, (int64_t)it.B * 8, k, "label_out", __func__));
        const int64_t per_member = mix_chunks(it.T, width);
        if (!(per_member <= 0x7fffffffLL && blocks + per_member * it.B <= 0x7fffffffLL))
            return fail(RSAF_ERR_ARG, __func__, k, "too many elements for one launch");
        g.item[k] = MixcItem{reinterpret_cast<const float4*>(it.arena), reinterpret_cast<const long long*>(it.row_start), it.row_count,
                             it.p, reinterpret_cast<float4*>(it.out), reinterpret_cast<const long long*>(it.label_src),
                             reinterpret_cast<const long long*>(it.label_index), reinterpret_cast<long long*>(it.label_out),
                             it.arena_rows, it.label_count, (unsigned)blocks, (unsigned)per_member, it.B, it.T, it.L};
        blocks += per_member * it.B;
        floats += (double)out_floats + (double)it.L * counted_frames(it) * width;
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_collate_mix", s, 0.0, 4.0 * floats);
    hipLaunchKernelGGL(collate_mix_group_kernel, dim3((unsigned)blocks), dim3(MIX_THREADS), 0, s, g);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_collate_mix_backward_group(const rsaf_collate_mix_backward_item* items_host, int K, int width, rsaf_stream_t stream) {
    static_assert(sizeof(rsaf_collate_mix_backward_item) == 88,
                  "rsaf_collate_mix_backward_item is part of the ABI (CollateMixBackwardItem of _lib.py)");
    TRY(check_group_args(K, items_host, __func__));
    if (!(width >= 4 && width % 4 == 0)) return fail(RSAF_ERR_ARG, __func__, -1, "width must be a positive multiple of 4");
    MixbGroup g{};
    MixfGroup f{};
    g.K = f.K = K;
    g.w4 = width / 4;
    cnnlstm::WrittenRanges wrote;
    int64_t blocks = 0;
    int waves = 0, l_max = 0;
    double floats = 0.0;
    for (int k = 0; k < K; ++k) {
        const rsaf_collate_mix_backward_item& it = items_host[k];
        TRY(check_mix_addressing(it, k, width, __func__));
        if (!(it.dx && it.partials && it.dp_out)) return fail(RSAF_ERR_ARG, __func__, k, "NULL pointer");
        if (!(al16(it.arena) && al16(it.dx))) return fail(RSAF_ERR_ARG, __func__, k, "arena and dx must be 16-byte aligned");
        if (reinterpret_cast<uintptr_t>(it.partials) & 7) return fail(RSAF_ERR_ARG, __func__, k, "partials must be 8-byte aligned");
        const Parts P = make_parts(Shape{it.B, it.L, it.T, width});
        if (it.partials_count < P.parts * it.L) return fail(RSAF_ERR_WORKSPACE, __func__, k, "partials too small (rsaf_layer_mix_partials)");
        TRY(wrote.add(it.partials, P.parts * it.L * 8, k, "partials", __func__));
        TRY(wrote.add(it.dp_out, (int64_t)it.L * 4, k, "dp_out", __func__));
        g.item[k] = MixbItem{reinterpret_cast<const float4*>(it.arena), reinterpret_cast<const long long*>(it.row_start), it.row_count,
                             reinterpret_cast<const float4*>(it.dx), it.partials, it.dp_out, it.arena_rows, P, (unsigned)blocks,
                             it.B, it.T, it.L};
        blocks += P.parts;                                 // <= 16 * MIX_PARTS_MAX
        f.partials[k] = it.partials; f.dp[k] = it.dp_out; f.parts[k] = P.parts; f.L[k] = it.L; f.wave0[k] = waves;
        waves += it.L;
        l_max = std::max(l_max, it.L);
        floats += (double)(it.L + 1) * counted_frames(it) * width;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(MIX_THREADS);
    {                                                      // the family counts both launches; the bytes are the first one's
        ProfScope prof("train_collate_mix_backward", s, 0.0, 4.0 * floats);
        if (l_max <= 4) hipLaunchKernelGGL(collate_mix_bwd_partial_kernel<4>, grid, block, 0, s, g);
        else if (l_max <= 8) hipLaunchKernelGGL(collate_mix_bwd_partial_kernel<8>, grid, block, 0, s, g);
        else if (l_max <= 16) hipLaunchKernelGGL(collate_mix_bwd_partial_kernel<16>, grid, block, 0, s, g);
        else hipLaunchKernelGGL(collate_mix_bwd_partial_kernel<32>, grid, block, 0, s, g);
    }
    ProfScope prof("train_collate_mix_backward", s, 0.0, 0.0);
    hipLaunchKernelGGL(collate_mix_bwd_final_kernel, dim3((waves + MIX_THREADS / 64 - 1) / (MIX_THREADS / 64)), block, 0, s, f);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_layer_mix_adam_group(const rsaf_layer_mix_adam_item* items_host, int K, rsaf_stream_t stream) {
    static_assert(sizeof(rsaf_layer_mix_adam_item) == 112, "rsaf_layer_mix_adam_item is part of the ABI (LayerMixAdamItem of _lib.py)");
    TRY(check_group_args(K, items_host, __func__));
    MixAdamGroup g{};
    for (int k = 0; k < K; ++k) {
        const rsaf_layer_mix_adam_item& it = items_host[k];
        if (!(it.L >= 1 && it.L <= RSAF_LAYER_MIX_MAX)) return fail(RSAF_ERR_ARG, __func__, k, "num_layers must be in [1, 32] (RSAF_LAYER_MIX_MAX)");
        if (!(it.mode >= RSAF_LAYER_MIX_FROM_DP && it.mode <= RSAF_LAYER_MIX_SOFTMAX_ONLY)) return fail(RSAF_ERR_ARG, __func__, k, "unknown mode");
        if (!(it.w && it.p_next)) return fail(RSAF_ERR_ARG, __func__, k, "NULL pointer");
        MixAdamItem& r = g.item[k];
        r.w = it.w; r.p_next = it.p_next; r.L = it.L; r.mode = it.mode;
        if (it.mode == RSAF_LAYER_MIX_SOFTMAX_ONLY) continue;
        if (!(it.exp_avg && it.exp_avg_sq && (it.mode == RSAF_LAYER_MIX_FROM_DP ? it.p && it.dp : it.dw != nullptr)))
            return fail(RSAF_ERR_ARG, __func__, k, "NULL pointer");
        if (!(it.step >= 1)) return fail(RSAF_ERR_ARG, __func__, k, "step counts from 1");
        if (!(it.beta1 >= 0.0 && it.beta1 < 1.0 && it.beta2 >= 0.0 && it.beta2 < 1.0 && it.eps >= 0.0 && it.lr >= 0.0))
            return fail(RSAF_ERR_ARG, __func__, k, "needs 0 <= beta < 1, eps >= 0, lr >= 0");
        for (int j = 0; j < k; ++j)
            if (items_host[j].w == it.w) return fail(RSAF_ERR_ARG, __func__, k, "shares its weights with item " + std::to_string(j));
        r.p = it.p; r.dp = it.dp; r.dw = it.dw; r.dw_out = it.mode == RSAF_LAYER_MIX_FROM_DP ? it.dw_out : nullptr;
        r.m = it.exp_avg; r.v = it.exp_avg_sq;
        r.b1 = it.beta1; r.b2 = it.beta2; r.eps = it.eps;
        r.step_size = it.lr / (1.0 - std::pow(it.beta1, (double)it.step));
        r.inv_sqrt_bc2 = 1.0 / std::sqrt(1.0 - std::pow(it.beta2, (double)it.step));
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("layer_mix_adam", s, 0.0, 0.0);
    hipLaunchKernelGGL(layer_mix_adam_group_kernel, dim3((unsigned)K), dim3(64), 0, s, g);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

}  // extern "C"
