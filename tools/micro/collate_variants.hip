// How many elements per lane the collate copy of csrc/aggregate.hip should take: the copy of one 4 x T x 768 batch (T = 4 378
// and 20 000, all members of full length) at 1 / 2 / 4 / 8 / 16 float4 per lane, plain and with nontemporal loads and
// stores, against a row-gather kernel of the gather_rows_kernel form (one wave per row, an int64 row index).  20 launches
// between two events per figure, ten different source batches in turn, the variants alternating over three rounds.
// All indices are in range by construction.
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/micro/collate_variants.hip -o tools/micro/collate_variants.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

template <int PT, bool NT>
__global__ __launch_bounds__(256) void collate(const f4* __restrict__ arena, const long long* __restrict__ start,
                                               const int* __restrict__ count, f4* __restrict__ out, int T, long long w, unsigned bpm) {
    const unsigned b = blockIdx.x / bpm, chunk = blockIdx.x - b * bpm;
    const long long n = min(max(count[b], 0), T);
    const long long end = (long long)T * w, hi = n * w;
    const long long e0 = (long long)chunk * (256 * PT) + threadIdx.x;
    const f4* src = arena + start[b] * w;
    f4* dst = out + (long long)b * T * w;
    f4 v[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const long long e = e0 + j * 256;
        v[j] = f4{0.f, 0.f, 0.f, 0.f};
        if (e < hi) v[j] = NT ? __builtin_nontemporal_load(src + e) : src[e];
    }
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const long long e = e0 + j * 256;
        if (e < end) { if (NT) __builtin_nontemporal_store(v[j], dst + e); else dst[e] = v[j]; }
    }
}

__global__ __launch_bounds__(256) void gather(const float* __restrict__ src, long long ld, const long long* __restrict__ src_row,
                                              long long n_rows, int width, float* __restrict__ dst) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const long long s = src_row[r];
    const float4* sp = s >= 0 ? reinterpret_cast<const float4*>(src + s * ld) : nullptr;
    float4* dp = reinterpret_cast<float4*>(dst + r * ld);
    for (int c = lane; c < width / 4; c += 64) dp[c] = sp ? sp[c] : make_float4(0.f, 0.f, 0.f, 0.f);
}

int main() {
    const int B = 4, W = 768, NB = 10, REPS = 20;
    for (int T : {4378, 20000}) {
        const long long rows = (long long)NB * B * T;
        float *arena, *out;
        CK(hipMalloc(&arena, rows * W * 4));
        CK(hipMalloc(&out, (long long)B * T * W * 4));
        CK(hipMemset(arena, 1, rows * W * 4));
        std::vector<long long> st(NB * B), idx((size_t)NB * B * T);
        std::vector<int> cnt(NB * B, T);
        for (int i = 0; i < NB * B; ++i) st[i] = (long long)i * T;
        for (size_t i = 0; i < idx.size(); ++i) idx[i] = (long long)i;
        long long *dst_, *didx; int* dcnt;
        CK(hipMalloc(&dst_, st.size() * 8)); CK(hipMalloc(&dcnt, cnt.size() * 4)); CK(hipMalloc(&didx, idx.size() * 8));
        CK(hipMemcpy(dst_, st.data(), st.size() * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(dcnt, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(didx, idx.data(), idx.size() * 8, hipMemcpyHostToDevice));
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        const long long w = W / 4, member = (long long)T * w;
        auto run = [&](int variant, int rep) {
            const int k = rep % NB;
            const long long* s = dst_ + k * B; const int* c = dcnt + k * B;
            const f4* a = reinterpret_cast<const f4*>(arena); f4* o = reinterpret_cast<f4*>(out);
#define LAUNCH(PT, NT) { unsigned bpm = (unsigned)((member + 256 * PT - 1) / (256 * PT)); \
                         hipLaunchKernelGGL((collate<PT, NT>), dim3(bpm * B), dim3(256), 0, 0, a, s, c, o, T, w, bpm); }
            switch (variant) {
                case 0: hipLaunchKernelGGL(gather, dim3((unsigned)(((long long)B * T + 3) / 4)), dim3(256), 0, 0, arena, (long long)W,
                                           didx + (long long)k * B * T, (long long)B * T, W, out); break;
                case 1: LAUNCH(8, false) break;
                case 2: LAUNCH(4, false) break;
                case 3: LAUNCH(2, false) break;
                case 4: LAUNCH(1, false) break;
                case 5: LAUNCH(16, false) break;
                case 6: LAUNCH(8, true) break;
                case 7: LAUNCH(4, true) break;
                case 8: LAUNCH(2, true) break;
            }
        };
        const char* names[] = {"gather_rows form", "collate PT=8", "collate PT=4", "collate PT=2", "collate PT=1", "collate PT=16",
                               "collate PT=8 nt", "collate PT=4 nt", "collate PT=2 nt"};
        for (int v = 0; v < 9; ++v) run(v, 0);
        CK(hipDeviceSynchronize());
        for (int round = 0; round < 3; ++round)
            for (int v = 0; v < 9; ++v) {
                CK(hipEventRecord(e0, 0));
                for (int r = 0; r < REPS; ++r) run(v, r);
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                CK(hipGetLastError());
                float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
                printf("T=%5d round %d %-18s %8.4f ms per batch  %6.2f TB/s\n", T, round, names[v], ms / REPS,
                       2.0 * B * T * W * 4 / (ms / REPS * 1e-3) / 1e12);
            }
        CK(hipFree(arena)); CK(hipFree(out)); CK(hipFree(dst_)); CK(hipFree(dcnt)); CK(hipFree(didx));
    }
    return 0;
}
