// Session aggregation and batch assembly behind the extractors for gfx950.
//   rsaf_segment_mean_std : per participant mean and sample standard deviation (ddof = 1, NaN skipped) of every
//                           feature column, the arithmetic of DataFrame.groupby(...).agg(['mean', 'std'])
//                           in src/utils.py:49.
//   rsaf_rows_segment_mean_f32 : per file column means of float32 frame rows, several planes per launch (one per Wav2Vec2
//                           hidden state): np.mean(sequence, axis=0) of src/foundation_model_extractor.py:160 for every
//                           tapped layer at once, accumulated in fp64 in row order (deterministic, no atomics).
//   rsaf_gather_rows_f32  : row gather with zero fill: np.vstack of a participant's clip sequences
//                           (src/utils.py:96) and the right-zero-padded batch of collate_fn
//                           (src/dl_cv_strategies.py:81-84) are both one launch.
//   rsaf_collate_pad_group : the padded batches of K DataLoader steps (collate_fn, src/dl_cv_strategies.py:81-84) out of
//                           sequences that live back to back in one device arena, ONE launch for all K: no index
//                           array, no memset, the zeros of the padding written by the same kernel.
//   rsaf_collate_augment_group : the same launch with each member's augmentation pipeline (the reference's `transform=` of
//                           SequenceDataset, src/dl_cv_strategies.py:19-62) applied between the loads and the stores,
//                           every value a pure function of (seed, epoch, sample, op, element) (augment_rng.h).
// All but the last are HBM-bound streaming kernels (every input element is read once or twice, coalesced along the row);
// a member that draws Gaussian noise pays a Philox block and two Box-Muller pairs per four elements.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "augment_rng.h"
#include "cnnlstm_host.h"       // TRY, fail, check_group_args (the group entries' checks); rsaf_common.h

namespace rsaf {
namespace aggregate {

// one workgroup per (segment, 256-column slab); thread = column, rows walked in the given order
__global__ __launch_bounds__(256) void segment_mean_std_kernel(const double* __restrict__ rows, int64_t ld,
                                                               const int* __restrict__ row_index, const int* __restrict__ seg_off,
                                                               int width, double* __restrict__ out) {
    const int seg = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    if (col >= width) return;
    const int a = seg_off[seg], b = seg_off[seg + 1];
    const double qn = __longlong_as_double(0x7ff8000000000000LL);
    double sum = 0.0;
    int cnt = 0;
    for (int i = a; i < b; ++i) {
        const double v = rows[(int64_t)row_index[i] * ld + col];
        if (v == v) { sum += v; ++cnt; }
    }
    const double mean = cnt > 0 ? sum / (double)cnt : qn;
    double ssq = 0.0;
    for (int i = a; i < b; ++i) {
        const double v = rows[(int64_t)row_index[i] * ld + col];
        if (v == v) { const double d = v - mean; ssq += d * d; }
    }
    double* o = out + ((int64_t)seg * width + col) * 2;
    o[0] = mean;
    o[1] = cnt > 1 ? sqrt(ssq / (double)(cnt - 1)) : qn;
}

// one workgroup per (segment, 256-column slab, plane); thread = column, the segment's rows summed in order in fp64 (8 loads in
// flight per thread); an empty segment gives NaN, as np.mean does
__global__ __launch_bounds__(256) void rows_segment_mean_kernel(const float* __restrict__ rows, int64_t ld, int64_t plane_floats,
                                                                const int64_t* __restrict__ seg_off, int n_seg, int width,
                                                                float* __restrict__ out) {
    const int seg = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x, pl = blockIdx.z;
    if (col >= width) return;
    const int64_t a = seg_off[seg], b = seg_off[seg + 1];
    const float* p = rows + (int64_t)pl * plane_floats + col;
    double sum = 0.0;
    int64_t i = a;
    for (; i + 8 <= b; i += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(i + k) * ld];
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += (double)v[k];
    }
    for (; i < b; ++i) sum += (double)p[i * ld];
    out[((int64_t)pl * n_seg + seg) * width + col] = b > a ? (float)(sum / (double)(b - a)) : __int_as_float(0x7fc00000);
}

// dst row r = src row src_row[r] (zeros when src_row[r] < 0); one wave per row, float4 when the row allows it
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, int64_t ld_src,
                                                          const int64_t* __restrict__ src_row, int64_t n_rows, int width,
                                                          float* __restrict__ dst, int64_t ld_dst, int vec4) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const int64_t s = src_row[r];
    float* d = dst + r * ld_dst;
    if (vec4) {
        const float4* sp = s >= 0 ? reinterpret_cast<const float4*>(src + s * ld_src) : nullptr;
        float4* dp = reinterpret_cast<float4*>(d);
        for (int c = lane; c < width / 4; c += 64) dp[c] = sp ? sp[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (int c = lane; c < width; c += 64) d[c] = s >= 0 ? src[s * ld_src + c] : 0.0f;
    }
}


// ---- rsaf_collate_pad_group -------------------------------------------------------------------------------------------
// A member's slice out[b] is T * width contiguous floats, and so are the frames it copies (arena rows row_start[b] ..
// + n): a member is one contiguous copy followed by one contiguous run of zeros, and a workgroup takes COLLATE_CHUNK
// consecutive elements (float4 or float) of one member.  Nothing is divided per element: the rows that exist in the
// arena become an element range [lo, hi) once per workgroup.
// Elements per lane, all loaded before the first store.  8 and 1 were both measured in this kernel with tools/lockstep_feed_bench.py
// (profiles/r24/lockstep_feed.txt and lockstep_feed_one_per_lane.txt): the launch of a K = 16 group step moves 5.7-5.8 TB/s
// (read + written) with 8 and 4.7-4.8 with 1, one 4 x 20 000 x 768 batch takes 0.090 against 0.094 ms.  A stand-alone copy
// of the loop (tools/micro/collate_variants.hip) ranks them the other way round, so that ranking was not adopted.
constexpr int COLLATE_PER_THREAD = 8;
constexpr int COLLATE_CHUNK = 256 * COLLATE_PER_THREAD;       // elements of one workgroup: 32 KB of float4, 8 KB of float

struct CollateItem {
    const float* arena;
    const long long* row_start;
    const int* row_count;
    float* out;
    const long long* label_src;
    const long long* label_index;
    long long* label_out;
    long long arena_rows, label_count;
    unsigned first_block;          // of this item in the grid
    unsigned blocks_per_member;    // ceil(T * row elements / COLLATE_CHUNK)
    int B, T, vec4;
};
struct CollateGroup {
    CollateItem item[RSAF_CNNLSTM_GROUP_MAX];
    int K, width;
};
static_assert(sizeof(CollateGroup) <= 3584, "the descriptors travel by value in the kernel arguments");

template <typename V>
__device__ __forceinline__ void collate_chunk(const V* __restrict__ src, V* __restrict__ dst, int64_t e0, int64_t lo, int64_t hi,
                                              int64_t end) {
    V v[COLLATE_PER_THREAD];
#pragma unroll
    for (int j = 0; j < COLLATE_PER_THREAD; ++j) {
        const int64_t e = e0 + j * 256;
        v[j] = V{};
        if (e >= lo && e < hi) v[j] = src[e];
    }
#pragma unroll
    for (int j = 0; j < COLLATE_PER_THREAD; ++j) {
        const int64_t e = e0 + j * 256;
        if (e < end) dst[e] = v[j];
    }
}

// grid: the workgroups of all items back to back (item k from first_block on), blocks_per_member per member
__global__ __launch_bounds__(256) void collate_pad_group_kernel(const CollateGroup g) {
    int k = 0;
    while (k + 1 < g.K && blockIdx.x >= g.item[k + 1].first_block) ++k;
    const CollateItem& it = g.item[k];
    const unsigned blk = blockIdx.x - it.first_block;
    const unsigned b = blk / it.blocks_per_member, chunk = blk - b * it.blocks_per_member;
    if (blk == 0 && it.label_out) {
        for (int i = threadIdx.x; i < it.B; i += 256) {
            const long long j = it.label_index[i];
            it.label_out[i] = (j >= 0 && j < it.label_count) ? it.label_src[j] : -1LL;
        }
    }
    const int64_t start = it.row_start[b];
    const int64_t n = min(max(it.row_count[b], 0), it.T);
    // the frames t of the member whose arena row start + t exists: [t_lo, t_hi), empty when none does
    const int64_t t_lo = start < 0 ? (start < -n ? n : -start) : 0;
    const int64_t t_hi = start >= it.arena_rows ? t_lo : max(min(n, it.arena_rows - start), t_lo);
    const int64_t w = it.vec4 ? g.width / 4 : g.width;                    // elements of a row
    const int64_t end = (int64_t)it.T * w, lo = t_lo * w, hi = t_hi * w;
    const int64_t e0 = (int64_t)chunk * COLLATE_CHUNK + threadIdx.x;
    // src is formed from the member's first row only where one of its rows exists, and read only at elements of [lo, hi)
    const float* src = it.arena + (t_hi > t_lo ? start : 0) * g.width;
    float* dst = it.out + (int64_t)b * it.T * g.width;
    if (it.vec4) collate_chunk(reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), e0, lo, hi, end);
    else collate_chunk(src, dst, e0, lo, hi, end);
}

// ---- rsaf_collate_augment_group ---------------------------------------------------------------------------------------
// The same chunk walk with the member's augmentation pipeline between the loads and the stores (the mapping: include/rsaf.h,
// coded in augment_rng.h).  The op loop is the outer one: an op's table entry (uniform loads) and parameter block are the
// same for the whole workgroup, which then applies the op to the elements it holds in registers, and only to those of
// [lo, hi): the padding is never touched.  A workgroup whose member fires no op falls through to the stores, a plain copy.
struct AugmentItem {
    CollateItem c;
    const rsaf_augment_op* ops;
    const long long* sample_id;
    unsigned long long seed;
    unsigned epoch;
    int n_ops;
};
struct AugmentGroup {
    AugmentItem item[RSAF_CNNLSTM_GROUP_MAX];
    int K, width;
};
static_assert(sizeof(AugmentGroup) <= 3584, "the descriptors travel by value in the kernel arguments");

// N floats per element: 4 (float4 path) or 1 (dword path).  `w`: elements of a row; e0, lo, hi, end in elements; `own_n`:
// the member's own frames (what TimeMask divides).  An element's flat float index in the member is N * e on either path.
template <int N>
__device__ __forceinline__ void augment_chunk(const AugmentItem& it, int width, const float* __restrict__ src, float* __restrict__ dst,
                                              int64_t e0, int64_t lo, int64_t hi, int64_t end, int64_t own_n, uint32_t sample) {
    constexpr int P = COLLATE_PER_THREAD;
    const int64_t w = width / N;
    float x[P][N];
    bool in[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int64_t e = e0 + j * 256;
        in[j] = e >= lo && e < hi;
        if constexpr (N == 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in[j]) v = reinterpret_cast<const float4*>(src)[e];
            x[j][0] = v.x; x[j][1] = v.y; x[j][2] = v.z; x[j][3] = v.w;
        } else {
            x[j][0] = in[j] ? src[e] : 0.0f;
        }
    }
    // the op table is not written while the kernel runs: read through the constant address space, its uniform loads are scalar
    // on both store paths
    typedef const rsaf_augment_op __attribute__((address_space(4))) ConstOp;
    const ConstOp* table = (const ConstOp*)it.ops;
    for (int s = 0; s < it.n_ops; ++s) {
        rsaf_augment_op op;
        op.kind = table[s].kind;
        op.fire_threshold = table[s].fire_threshold;
        op.always = table[s].always;
        op.a = table[s].a;
        op.b = table[s].b;
        uint32_t pw[4];
        rng::augment_param_block(it.seed, it.epoch, sample, s, pw);
        if (!rng::augment_fires(op.always, op.fire_threshold, pw[0])) continue;
        if (op.kind == rng::AUGMENT_SCALE) {
            const float f = rng::augment_uniform(op.a, op.b, pw[1]);
#pragma unroll
            for (int j = 0; j < P; ++j)
                if (in[j]) {
#pragma unroll
                    for (int c = 0; c < N; ++c) x[j][c] *= f;
                }
        } else if (op.kind == rng::AUGMENT_GAUSSIAN_NOISE) {
            const float amp = rng::augment_uniform(op.a, op.b, pw[1]);
#pragma unroll
            for (int j = 0; j < P; ++j)
                if (in[j]) {
                    const uint64_t flat = (uint64_t)(e0 + j * 256) * N;        // < 2^34 (entry check)
                    uint32_t ew[4];
                    rng::augment_element_block(it.seed, it.epoch, sample, s, (uint32_t)(flat >> 2), ew);
                    if constexpr (N == 4) {
                        float z[4];
                        rng::augment_normal_pair(ew[0], ew[1], &z[0], &z[1]);
                        rng::augment_normal_pair(ew[2], ew[3], &z[2], &z[3]);
#pragma unroll
                        for (int c = 0; c < 4; ++c) x[j][c] = fmaf(amp, z[c], x[j][c]);
                    } else {
                        x[j][0] = fmaf(amp, rng::augment_normal_of(ew, (unsigned)(flat & 3)), x[j][0]);
                    }
                }
        } else if (op.kind == rng::AUGMENT_TIME_MASK) {
            int64_t start, len;
            rng::augment_span(own_n, op.a, op.b, pw[1], pw[2], &start, &len);
            const int64_t m_lo = start * w, m_hi = (start + len) * w;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const int64_t e = e0 + j * 256;
                if (e >= m_lo && e < m_hi) {
#pragma unroll
                    for (int c = 0; c < N; ++c) x[j][c] = 0.0f;
                }
            }
        } else if (op.kind == rng::AUGMENT_FEATURE_MASK) {
            int64_t start, len;
            rng::augment_span(width, op.a, op.b, pw[1], pw[2], &start, &len);
            // the column of the lane's first element, then one step of 256 elements at a time: no division per element
            const uint32_t uw = (uint32_t)w, step = 256u % uw;
            uint32_t col = (uint32_t)((uint64_t)e0 % uw);
#pragma unroll
            for (int j = 0; j < P; ++j) {
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    const int64_t d = (int64_t)col * N + c;
                    if (d >= start && d < start + len) x[j][c] = 0.0f;      // +0.0 in the padding as well
                }
                col += step;
                if (col >= uw) col -= uw;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int64_t e = e0 + j * 256;
        if (e < end) {
            if constexpr (N == 4) reinterpret_cast<float4*>(dst)[e] = make_float4(x[j][0], x[j][1], x[j][2], x[j][3]);
            else dst[e] = x[j][0];
        }
    }
}

// grid and member geometry: those of collate_pad_group_kernel
__global__ __launch_bounds__(256) void collate_augment_group_kernel(const AugmentGroup g) {
    int k = 0;
    while (k + 1 < g.K && blockIdx.x >= g.item[k + 1].c.first_block) ++k;
    const AugmentItem& ai = g.item[k];
    const CollateItem& it = ai.c;
    const unsigned blk = blockIdx.x - it.first_block;
    const unsigned b = blk / it.blocks_per_member, chunk = blk - b * it.blocks_per_member;
    const int64_t start = it.row_start[b];
    const int64_t own_n = max(it.row_count[b], 0);
    const int64_t n = min(own_n, (int64_t)it.T);
    const uint32_t sample = ai.n_ops > 0 ? (uint32_t)ai.sample_id[b] : 0u;
    const int64_t t_lo = start < 0 ? (start < -n ? n : -start) : 0;
    const int64_t t_hi = start >= it.arena_rows ? t_lo : max(min(n, it.arena_rows - start), t_lo);
    const int64_t w = it.vec4 ? g.width / 4 : g.width;
    const int64_t end = (int64_t)it.T * w, lo = t_lo * w, hi = t_hi * w;
    const int64_t e0 = (int64_t)chunk * COLLATE_CHUNK + threadIdx.x;
    const float* src = it.arena + (t_hi > t_lo ? start : 0) * g.width;
    float* dst = it.out + (int64_t)b * it.T * g.width;
    if (it.vec4) augment_chunk<4>(ai, g.width, src, dst, e0, lo, hi, end, own_n, sample);
    else augment_chunk<1>(ai, g.width, src, dst, e0, lo, hi, end, own_n, sample);
    // the labels last: no store stands between the kernel's entry and the uniform loads above
    if (blk == 0 && it.label_out) {
        for (int i = threadIdx.x; i < it.B; i += 256) {
            const long long j = it.label_index[i];
            it.label_out[i] = (j >= 0 && j < it.label_count) ? it.label_src[j] : -1LL;
        }
    }
}

// ---- what both collate entries check and size, item by item, before their launch ----------------------------------------
struct CollatePlan {
    rsaf::cnnlstm::WrittenRanges wrote;
    int64_t blocks = 0;
    double floats = 0.0;          // read + written, for the profiling family

    int add(const rsaf_collate_item& it, int k, int width, const char* who, CollateItem* out) {
        using namespace rsaf::cnnlstm;
        if (!(it.B >= 1 && it.T >= 1)) return fail(RSAF_ERR_ARG, who, k, "B and T must be >= 1");
        const int64_t out_floats = (int64_t)it.B * it.T * width;         // < 2^31 * 2^31 * 2^31 overflows: test the factors
        if (!((int64_t)it.B * it.T < (1LL << 40) && out_floats < (1LL << 40) && out_floats > 0))
            return fail(RSAF_ERR_ARG, who, k, "B * T * width must be < 2^40");
        if (!(it.arena && it.row_start && it.row_count && it.out)) return fail(RSAF_ERR_ARG, who, k, "NULL pointer");
        if (!(it.arena_rows >= 0)) return fail(RSAF_ERR_ARG, who, k, "arena_rows must be >= 0");
        const int n_label = (it.label_src != nullptr) + (it.label_index != nullptr) + (it.label_out != nullptr);
        if (!(n_label == 0 || n_label == 3) || (n_label == 0 && it.label_count != 0) || it.label_count < 0)
            return fail(RSAF_ERR_ARG, who, k, "label_src, label_count, label_index and label_out go together: all or none");
        TRY(wrote.add(it.out, out_floats * 4, k, "out", who));
        TRY(wrote.add(it.label_out, (int64_t)it.B * 8, k, "label_out", who));
        const int vec4 = width % 4 == 0 && ((reinterpret_cast<uintptr_t>(it.arena) | reinterpret_cast<uintptr_t>(it.out)) & 15) == 0;
        const int64_t member = (int64_t)it.T * (vec4 ? width / 4 : width);
        const int64_t per_member = (member + COLLATE_CHUNK - 1) / COLLATE_CHUNK;
        if (!(per_member <= 0x7fffffffLL && blocks + per_member * it.B <= 0x7fffffffLL))
            return fail(RSAF_ERR_ARG, who, k, "too many elements for one launch");
        *out = CollateItem{it.arena, reinterpret_cast<const long long*>(it.row_start), it.row_count, it.out,
                           reinterpret_cast<const long long*>(it.label_src), reinterpret_cast<const long long*>(it.label_index),
                           reinterpret_cast<long long*>(it.label_out), it.arena_rows, it.label_count,
                           (unsigned)blocks, (unsigned)per_member, it.B, it.T, vec4};
        blocks += per_member * it.B;
        const int64_t frames = it.frames >= 0 && it.frames <= (int64_t)it.B * it.T ? it.frames : (int64_t)it.B * it.T;
        floats += (double)out_floats + (double)frames * width;
        return RSAF_OK;
    }
};

}  // namespace aggregate
}  // namespace rsaf

using namespace rsaf;

extern "C" {

int rsaf_segment_mean_std(const double* rows, int64_t ld, const int* row_index, const int* seg_off, int n_seg, int width,
                          double* out, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_seg >= 0 && width >= 0 && ld >= width, "bad sizes");
    if (n_seg == 0 || width == 0) return RSAF_OK;
    RSAF_CHECK_ARG(rows && row_index && seg_off && out, "NULL pointer");
    RSAF_CHECK_ARG(n_seg <= 0x7fffffff && (width + 255) / 256 <= 65535, "too many segments or columns for one launch");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("segment_mean_std", s, 0.0, 0.0);
    hipLaunchKernelGGL(aggregate::segment_mean_std_kernel, dim3((unsigned)n_seg, (unsigned)((width + 255) / 256)), dim3(256), 0, s,
                       rows, ld, row_index, seg_off, width, out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_rows_segment_mean_f32(const float* rows, int64_t ld, int64_t plane_floats, int n_planes, const int64_t* seg_off, int n_seg,
                               int width, float* out, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_planes >= 0 && n_seg >= 0 && width >= 0 && ld >= width && plane_floats >= 0, "bad sizes");
    if (n_planes == 0 || n_seg == 0 || width == 0) return RSAF_OK;
    RSAF_CHECK_ARG(rows && seg_off && out, "NULL pointer");
    RSAF_CHECK_ARG(n_planes <= 65535 && (width + 255) / 256 <= 65535, "too many planes or columns for one launch");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("rows_segment_mean", s, 0.0, 0.0);
    hipLaunchKernelGGL(aggregate::rows_segment_mean_kernel, dim3((unsigned)n_seg, (unsigned)((width + 255) / 256), (unsigned)n_planes),
                       dim3(256), 0, s, rows, ld, plane_floats, seg_off, n_seg, width, out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_gather_rows_f32(const float* src, int64_t ld_src, const int64_t* src_row, int64_t n_rows, int width, float* dst,
                         int64_t ld_dst, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_rows >= 0 && width >= 0 && ld_src >= width && ld_dst >= width, "bad sizes");
    if (n_rows == 0 || width == 0) return RSAF_OK;
    RSAF_CHECK_ARG(src && src_row && dst, "NULL pointer");
    RSAF_CHECK_ARG((n_rows + 3) / 4 <= 0x7fffffffLL, "too many rows for one launch");
    const int vec4 = (width % 4 == 0) && (ld_src % 4 == 0) && (ld_dst % 4 == 0) &&
                     ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("gather_rows", s, 0.0, 8.0 * (double)n_rows * width);
    hipLaunchKernelGGL(aggregate::gather_rows_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, src, ld_src, src_row,
                       n_rows, width, dst, ld_dst, vec4);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_collate_pad_group(const rsaf_collate_item* items_host, int K, int width, rsaf_stream_t stream) {
    using namespace rsaf::cnnlstm;
    static_assert(sizeof(rsaf_collate_item) == 88, "rsaf_collate_item is part of the ABI (CollateItem of _lib.py)");
    TRY(check_group_args(K, items_host, __func__));
    if (!(width >= 1)) return fail(RSAF_ERR_ARG, __func__, -1, "width must be >= 1");
    aggregate::CollateGroup g{};
    g.K = K;
    g.width = width;
    aggregate::CollatePlan plan;
    for (int k = 0; k < K; ++k) TRY(plan.add(items_host[k], k, width, __func__, &g.item[k]));
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_collate", s, 0.0, 4.0 * plan.floats);
    hipLaunchKernelGGL(aggregate::collate_pad_group_kernel, dim3((unsigned)plan.blocks), dim3(256), 0, s, g);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_collate_augment_group(const rsaf_collate_augment_item* items_host, int K, int width, rsaf_stream_t stream) {
    using namespace rsaf::cnnlstm;
    static_assert(sizeof(rsaf_augment_op) == 32, "rsaf_augment_op is part of the ABI (AugmentOp of _lib.py)");
    static_assert(sizeof(rsaf_collate_augment_item) == 136 && offsetof(rsaf_collate_augment_item, ops) == sizeof(rsaf_collate_item),
                  "rsaf_collate_augment_item is part of the ABI (CollateAugmentItem of _lib.py) and opens with rsaf_collate_item");
    TRY(check_group_args(K, items_host, __func__));
    if (!(width >= 1)) return fail(RSAF_ERR_ARG, __func__, -1, "width must be >= 1");
    aggregate::AugmentGroup g{};
    g.K = K;
    g.width = width;
    aggregate::CollatePlan plan;
    for (int k = 0; k < K; ++k) {
        const rsaf_collate_augment_item& it = items_host[k];
        rsaf_collate_item batch;
        std::memcpy(&batch, &it, sizeof batch);
        TRY(plan.add(batch, k, width, __func__, &g.item[k].c));
        if (!(it.n_ops >= 0 && it.n_ops <= RSAF_AUGMENT_MAX)) return fail(RSAF_ERR_ARG, __func__, k, "n_ops must be in [0, 8] (RSAF_AUGMENT_MAX)");
        if (it.n_ops > 0) {
            if (!(it.ops && it.ops_host && it.sample_id))
                return fail(RSAF_ERR_ARG, __func__, k, "ops, ops_host and sample_id must not be NULL when n_ops > 0");
            for (int s = 0; s < it.n_ops; ++s) {
                const rsaf_augment_op& op = it.ops_host[s];
                if (!(op.kind >= 0 && op.kind < rng::AUGMENT_KINDS))
                    return fail(RSAF_ERR_ARG, __func__, k, "op " + std::to_string(s) + ": unknown kind " + std::to_string(op.kind));
                if (!(std::isfinite(op.a) && std::isfinite(op.b)))
                    return fail(RSAF_ERR_ARG, __func__, k, "op " + std::to_string(s) + ": a and b must be finite");
            }
            if (!(it.epoch < (1ULL << 32))) return fail(RSAF_ERR_ARG, __func__, k, "epoch must be < 2^32");
            if (!((int64_t)it.T * width < (1LL << 34))) return fail(RSAF_ERR_ARG, __func__, k, "T * width must be < 2^34 with n_ops > 0");
        }
        g.item[k].ops = it.n_ops > 0 ? it.ops : nullptr;
        g.item[k].sample_id = it.n_ops > 0 ? reinterpret_cast<const long long*>(it.sample_id) : nullptr;
        g.item[k].seed = it.seed;
        g.item[k].epoch = (unsigned)it.epoch;
        g.item[k].n_ops = it.n_ops;
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_collate_augment", s, 0.0, 4.0 * plan.floats);
    hipLaunchKernelGGL(aggregate::collate_augment_group_kernel, dim3((unsigned)plan.blocks), dim3(256), 0, s, g);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

}  // extern "C"
