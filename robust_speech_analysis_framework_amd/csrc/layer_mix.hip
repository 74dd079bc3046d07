// Learned mix of encoder layers on gfx950: x[b,t,:] = sum_l p[l] h[b,l,t,:] and the gradient of the loss with respect to p
// (rsaf_layer_mix_forward / _backward, include/rsaf.h).  Both are streams over h, L + 1 times the size of x, so each reads h
// once with float4 loads and touches x / dx once per position; the softmax over the L weights and its Jacobian are the
// caller's.  Addressing, the partition of the backward and the order of its sums: layer_mix_layout.h.
#include "layer_mix_layout.h"
#include "rsaf_common.h"

namespace rsaf {
namespace layermix {

__global__ __launch_bounds__(MIX_THREADS) void layer_mix_fwd_kernel(const float4* __restrict__ h, const float* __restrict__ p,
                                                                    float4* __restrict__ x, Parts P, int L) {
    for (int64_t i = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x; i < P.n4; i += (int64_t)gridDim.x * MIX_THREADS) {
        const float4* hi = h + h_index(P, L, i, 0);
        const float p0 = p[0];
        const float4 v0 = hi[0];
        float4 a = make_float4(p0 * v0.x, p0 * v0.y, p0 * v0.z, p0 * v0.w);      // L = 1, p = [1]: the bits of h
#pragma unroll 4
        for (int l = 1; l < L; ++l) {
            const float pl = p[l];
            const float4 v = hi[(int64_t)l * P.td4];
            a.x += pl * v.x; a.y += pl * v.y; a.z += pl * v.z; a.w += pl * v.w;
        }
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

static int check_shape(const Shape& s) {
    const char* problem = shape_problem(s);
    RSAF_CHECK_ARG(!problem, problem);
    return RSAF_OK;
}

static bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

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

}  // extern "C"
