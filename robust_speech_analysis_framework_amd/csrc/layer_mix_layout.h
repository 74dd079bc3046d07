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

inline int64_t partials_doubles(const Shape& s) { return make_parts(s).parts * s.L; }

// workgroups of the forward: a grid-stride walk over the n4 positions
inline int64_t forward_blocks(const Parts& p) {
    return std::min<int64_t>(std::max<int64_t>((p.n4 + MIX_THREADS - 1) / MIX_THREADS, 1), MIX_PARTS_MAX);
}

}  // namespace layermix
}  // namespace rsaf
