// Layout of the learned mix of encoder layers (layer_mix.hip), stated once for the kernels and the host code that sizes the
// scratch: how h [B][L][T][D] is addressed from a position of x [B][T][D], and the partition and summation order of the
// backward's L sums.  Plain C++ (no HIP include): tests/host/layer_mix_replay.cpp compiles it with g++ and replays both.
//
// Positions are counted in float4 (D % 4 == 0): n4 = B T D / 4 of them, position i of x lies in batch row b = i / td4
// (td4 = T D / 4) at r = i % td4, and layer l of it is float4 (b L + l) td4 + r of h.
//
// Backward, dp[l] = sum_i h_l[i] . dx[i]: the positions are cut into `parts` runs of `per` consecutive positions (the last
// ones ragged or empty), one workgroup of MIX_THREADS threads each.  Thread t of part q adds, in double and in ascending
// order, the products of positions q per + t, q per + t + MIX_THREADS, ... (components x, y, z, w of a float4 in this
// order; a product of two floats is exact in double).  The 64 lanes of a wave are added by the xor butterfly of
// wave_sum_f64 (v[i] += v[i ^ o], o = 32, 16, .., 1), the four waves as ((w0 + w1) + w2) + w3 -> partials[q][l].  The final
// launch gives every l one wave: lane j adds parts j, j + 64, ... in ascending order, then the same butterfly, then one
// rounding to float.  `parts` depends on the shape alone, so equal inputs give equal bits.
//
// The mix inside the collate launch (rsaf_collate_mix_group / rsaf_collate_mix_backward_group): the stack of a sequence of
// n frames lies in the arena as L n rows, layer-major, from row `start` on: frame t of layer l is arena row
// start + l n + t (block_row).  Member b of a batch padded to T frames mixes its frames t < min(n, T); everything else of
// out[b] is +0.0, and a member whose block does not lie wholly inside the arena (block_inside) is zeros throughout.  The
// forward cuts every member's T width / 4 float4 into chunks of MIXC_CHUNK consecutive ones, one workgroup each, lane j of
// which holds float4 chunk * MIXC_CHUNK + j + 256 i, i < MIXC_PER_THREAD.  The arithmetic of one position is mix_term, for
// that kernel and layer_mix_fwd_kernel alike.  The backward keeps the partition and the order of the dense backward for the
// padded shape (B, L, T, width) and skips the positions whose frame does not exist: a skipped term is a product with a
// zero of the padded stack, an exact +-0 added to a sum that starts at +0.0, so the sums keep their bits.
#pragma once
#include <algorithm>
#include <cstdint>

#include "rsaf.h"

namespace rsaf {
namespace layermix {

constexpr int MIX_THREADS = 256;
constexpr int64_t MIX_PART_MIN = 4096;        // float4 positions of a part before a second part is opened
constexpr int64_t MIX_PARTS_MAX = 2048;       // 8 workgroups per CU on 256 CUs
constexpr int64_t MIX_N_MAX = int64_t(1) << 40;

struct Shape {
    int B, L, T, D;
};

inline const char* shape_problem(const Shape& s) {
    if (!(s.L >= 1 && s.L <= RSAF_LAYER_MIX_MAX)) return "num_layers must be in [1, 32] (RSAF_LAYER_MIX_MAX)";
    if (!(s.B >= 1 && s.T >= 1)) return "B and T must be positive";
    if (!(s.D >= 4 && s.D % 4 == 0)) return "D must be a positive multiple of 4";
    if (!((int64_t)s.B * s.T * s.D < MIX_N_MAX)) return "B*T*D must be below 2^40";
    return nullptr;
}

struct Parts {
    int64_t td4, n4, parts, per;
};

inline Parts make_parts(const Shape& s) {
    Parts p;
    p.td4 = (int64_t)s.T * (s.D / 4);
    p.n4 = (int64_t)s.B * p.td4;
    p.parts = std::min<int64_t>(std::max<int64_t>((p.n4 + MIX_PART_MIN - 1) / MIX_PART_MIN, 1), MIX_PARTS_MAX);
    p.per = (p.n4 + p.parts - 1) / p.parts;
    return p;
}

// float4 index into h of layer l at position i of x (constexpr: the kernels call it too)
constexpr int64_t h_index(const Parts& p, int L, int64_t i, int l) {
    const int64_t b = i / p.td4;
    return (b * L + l) * p.td4 + (i - b * p.td4);
}

#ifdef __HIPCC__
#define RSAF_MIX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RSAF_MIX_HD inline
#endif

// one layer's term of one position: a = p0 v0 for the first layer, a += p_l v_l after it, float32, l ascending.  V: four
// floats x, y, z, w (float4 in the kernels).  `first` is a constant wherever the call is unrolled.
template <typename V>
RSAF_MIX_HD void mix_term(V& a, float pl, const V& v, bool first) {
    if (first) {
        a.x = pl * v.x; a.y = pl * v.y; a.z = pl * v.z; a.w = pl * v.w;
    } else {
        a.x += pl * v.x; a.y += pl * v.y; a.z += pl * v.z; a.w += pl * v.w;
    }
}

// ---- the mix inside the collate launch ----
constexpr int MIXC_PER_THREAD = 2;                       // float4 of out per lane
constexpr int MIXC_LAYERS_IN_FLIGHT = 4;                 // layers whose loads are issued before their adds
constexpr int64_t MIXC_CHUNK = (int64_t)MIX_THREADS * MIXC_PER_THREAD;

// arena row of frame t of layer l of a block of n frames per layer that starts at row `start`
constexpr int64_t block_row(int64_t start, int64_t n, int l, int64_t t) { return start + (int64_t)l * n + t; }

// the L n rows of the block all exist (n <= 0: no rows, nothing to read)
constexpr bool block_inside(int64_t start, int64_t n, int L, int64_t arena_rows) {
    return n > 0 && start >= 0 && start <= arena_rows && (int64_t)L * n <= arena_rows - start;      // L n < 2^36: n is an int32 count
}

// Where a lane of the backward stands in the padded batch: member b0 + db (b0: the member of the part's first position, the
// same for the whole workgroup), frame t, float4 c of the row.  The two 64-bit divisions are the part's; a lane adds its
// offset and steps by MIX_THREADS float4 in 32 bits (t < T < 2^31, c < width / 4).
struct MixPos {
    uint32_t db, t, c;
};

// part that starts at float4 i0 of the padded batch: *b0 and the position of lane `tid`'s first float4, i0 + tid
RSAF_MIX_HD MixPos mix_first_pos(const Parts& P, uint32_t w4, uint32_t T, int64_t i0, uint32_t tid, int64_t* b0) {
    *b0 = i0 / P.td4;
    const int64_t r0 = i0 - *b0 * P.td4;
    const uint32_t t0 = (uint32_t)(r0 / w4), c0 = (uint32_t)(r0 - (int64_t)t0 * w4);
    const uint32_t rl = c0 + tid, ql = rl / w4;
    MixPos p{0u, 0u, rl - ql * w4};
    uint64_t t = (uint64_t)t0 + ql;
    while (t >= T) { t -= T; ++p.db; }
    p.t = (uint32_t)t;
    return p;
}

// MIX_THREADS float4 further
RSAF_MIX_HD void mix_step_pos(MixPos& p, uint32_t w4, uint32_t T) {
    const uint32_t dt = MIX_THREADS / w4, dc = MIX_THREADS - dt * w4;
    p.c += dc;
    p.t += dt;
    if (p.c >= w4) { p.c -= w4; ++p.t; }
    while (p.t >= T) { p.t -= T; ++p.db; }
}

// workgroups of one member of the forward
constexpr int64_t mix_chunks(int T, int width) { return ((int64_t)T * (width / 4) + MIXC_CHUNK - 1) / MIXC_CHUNK; }

inline int64_t partials_doubles(const Shape& s) { return make_parts(s).parts * s.L; }

// workgroups of the forward: a grid-stride walk over the n4 positions
inline int64_t forward_blocks(const Parts& p) {
    return std::min<int64_t>(std::max<int64_t>((p.n4 + MIX_THREADS - 1) / MIX_THREADS, 1), MIX_PARTS_MAX);
}

}  // namespace layermix
}  // namespace rsaf
