// Dropout masks of a group training step from the counter-based generator of dropout_rng.h: every mask of every replica
// in ONE launch (rsaf_dropout_masks_group, include/rsaf.h).
//
// A segment is one mask of one replica.  A thread computes one Philox block (four words) and writes the four floats as one
// 16-byte store; a workgroup covers DROP_WG_BLOCKS consecutive blocks of its segment in DROP_ITERS sweeps of 256 threads,
// so that a wave's store is 1 KiB of contiguous memory.  The workgroups of a launch are dealt to the segments by the
// prefix `wg_end`, which a workgroup searches with its (uniform) blockIdx: the lookup is scalar work on the kernel arguments.
// No LDS, no atomics; the floats at and beyond mask + n are never written (of the last block of a segment whose n is no
// multiple of 4, one thread stores n & 3 single floats).
#include <cmath>

#include "dropout_rng.h"
#include "rsaf_common.h"

namespace rsaf {
namespace dropout {

static const int DROP_MAX_SEGS = RSAF_CNNLSTM_GROUP_MAX * RSAF_DROPOUT_SLOTS;
static const int DROP_ITERS = 8;
static const unsigned DROP_WG_BLOCKS = 256u * DROP_ITERS;       // Philox blocks per workgroup: 32 KiB of mask

struct DropSeg {
    float* mask;
    unsigned nblk;                      // Philox blocks: ceil(n / 4) <= 2^30
    unsigned thr;
    float keep;                         // 0: p >= 1, the segment is zero-filled
    unsigned char item, slot, rem, pad; // rem = n & 3
};
struct DropGroup {
    DropSeg seg[DROP_MAX_SEGS];
    unsigned long long seed[RSAF_CNNLSTM_GROUP_MAX], step[RSAF_CNNLSTM_GROUP_MAX];
    unsigned wg_end[DROP_MAX_SEGS];     // one past the last workgroup of segment i (ascending; segment i starts at wg_end[i - 1])
    int nseg;
};
static_assert(sizeof(DropGroup) <= 3584, "the descriptors must fit the kernel argument segment");

__device__ __forceinline__ float4 dropout_float4(unsigned long long seed, unsigned long long step, unsigned slot, unsigned j,
                                                 unsigned thr, float keep) {
    if (keep == 0.0f) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t w[4];
    rng::dropout_block(seed, step, slot, j, w);
    return make_float4(rng::dropout_value(w[0], thr, keep), rng::dropout_value(w[1], thr, keep),
                       rng::dropout_value(w[2], thr, keep), rng::dropout_value(w[3], thr, keep));
}

__global__ __launch_bounds__(256) void dropout_masks_group_kernel(const DropGroup g) {
    // first segment whose end lies beyond this workgroup (uniform: blockIdx and kernel arguments only)
    int lo = 0, hi = g.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g.wg_end[mid] > blockIdx.x) hi = mid; else lo = mid + 1;
    }
    const DropSeg& sg = g.seg[lo];
    const unsigned wg0 = lo ? g.wg_end[lo - 1] : 0u;
    const unsigned long long seed = g.seed[sg.item], step = g.step[sg.item];
    const unsigned thr = sg.thr, slot = sg.slot, rem = sg.rem;
    const unsigned nfull = sg.nblk - (rem ? 1u : 0u);           // blocks whose four floats all lie below mask + n
    const float keep = sg.keep;
    float4* const mask4 = reinterpret_cast<float4*>(sg.mask);
    const unsigned first = (blockIdx.x - wg0) * DROP_WG_BLOCKS + threadIdx.x;
#pragma unroll 1
    for (int i = 0; i < DROP_ITERS; ++i) {
        const unsigned j = first + (unsigned)i * 256u;          // < 2^30 + 2048: no wrap
        if (j >= nfull) break;
        mask4[j] = dropout_float4(seed, step, slot, j, thr, keep);
    }
    // the n & 3 floats of the last block, by one thread of the segment's last workgroup: the only stores that are no
    // float4, kept out of the loop so that the loop's store stays one 16-byte instruction
    if (rem != 0 && blockIdx.x + 1 == g.wg_end[lo] && threadIdx.x == 0) {
        const float4 v = dropout_float4(seed, step, slot, nfull, thr, keep);
        float* dst = sg.mask + (size_t)nfull * 4;
        dst[0] = v.x;
        if (rem > 1) dst[1] = v.y;
        if (rem > 2) dst[2] = v.z;
    }
}

static int fail(const char* who, int item, int slot, const std::string& msg) {
    set_error(std::string(who) + ": item " + std::to_string(item) + ": slot " + std::to_string(slot) + ": " + msg);
    return RSAF_ERR_ARG;
}

}  // namespace dropout
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::dropout;

extern "C" int rsaf_dropout_masks_group(const rsaf_dropout_item* items_host, int K, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(K >= 1 && K <= RSAF_CNNLSTM_GROUP_MAX, "K must be in [1, 16] (rsaf_cnnlstm_train_group_max)");
    RSAF_CHECK_ARG(items_host, "items_host is NULL");
    DropGroup g{};
    struct Range { uintptr_t lo, hi; int item, slot; } ranges[DROP_MAX_SEGS];     // bytes [lo, hi) of every drawn mask
    uint64_t wgs = 0;
    double bytes = 0.0;
    for (int k = 0; k < K; ++k) {
        const rsaf_dropout_item& it = items_host[k];
        g.seed[k] = it.seed;
        g.step[k] = it.step;
        for (int s = 0; s < RSAF_DROPOUT_SLOTS; ++s) {
            const int64_t n = it.n[s];
            const double p = it.p[s];
            if (!(n >= 0 && n <= (int64_t)1 << 32)) return fail(__func__, k, s, "n must be in [0, 2^32]");
            if (std::isnan(p)) return fail(__func__, k, s, "p is NaN");
            if (!it.mask[s]) continue;
            if (n < 1) return fail(__func__, k, s, "a mask pointer needs n >= 1");
            if (!(p > 0.0)) return fail(__func__, k, s, "a mask pointer needs p > 0 (a slot with p <= 0 is not drawn: pass NULL)");
            if (reinterpret_cast<uintptr_t>(it.mask[s]) & 15) return fail(__func__, k, s, "mask must be 16-byte aligned");
            const uintptr_t lo = reinterpret_cast<uintptr_t>(it.mask[s]), hi = lo + (uintptr_t)n * 4;
            for (int r = 0; r < g.nseg; ++r)
                if (lo < ranges[r].hi && ranges[r].lo < hi)
                    return fail(__func__, k, s, "overlaps the mask of item " + std::to_string(ranges[r].item) + ", slot " +
                                                    std::to_string(ranges[r].slot));
            ranges[g.nseg] = Range{lo, hi, k, s};
            DropSeg& sg = g.seg[g.nseg];
            sg.mask = it.mask[s];
            sg.nblk = (unsigned)((n + 3) >> 2);
            sg.rem = (unsigned char)(n & 3);
            sg.keep = rng::dropout_keep_value(p);
            sg.thr = p >= 1.0 ? 0xffffffffu : rng::dropout_threshold(p);
            sg.item = (unsigned char)k;
            sg.slot = (unsigned char)s;
            wgs += (sg.nblk + DROP_WG_BLOCKS - 1) / DROP_WG_BLOCKS;      // <= 96 * 2^19
            g.wg_end[g.nseg] = (unsigned)wgs;
            ++g.nseg;
            bytes += (double)n * 4;
        }
    }
    if (g.nseg == 0) return RSAF_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_dropout_masks", s, 0.0, bytes);
    hipLaunchKernelGGL(dropout_masks_group_kernel, dim3((unsigned)wgs), dim3(256), 0, s, g);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}
