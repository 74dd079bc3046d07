// Counter-based generator of the dropout masks: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
// easy as 1, 2, 3", SC'11) and the mapping from (seed, step, slot, element) to a mask value that include/rsaf.h documents.
// Plain inline code: the kernel of dropout_masks.hip and a host compiler (tests/host/dropout_rng_replay.cpp) read the same
// functions, so what the host replays is what the device computes.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSAF_RNG_HD __host__ __device__
#else
#define RSAF_RNG_HD
#endif

namespace rsaf {
namespace rng {

static const uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;     // round multipliers
static const uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;     // Weyl constants of the key schedule

// out = Philox4x32-10(counter c, key k): ten rounds, the key bumped between rounds
RSAF_RNG_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                      uint32_t out[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The four words of block j of a slot: key = (seed low, seed high), counter = (j, slot, step low, step high).
// Element e of the slot's flat layout takes word e & 3 of block e >> 2.
RSAF_RNG_HD inline void dropout_block(uint64_t seed, uint64_t step, uint32_t slot, uint32_t j, uint32_t out[4]) {
    philox4x32_10(j, slot, (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

// thr = floor(p * 2^32) for 0 < p < 1: an element is kept iff its word >= thr
RSAF_RNG_HD inline uint32_t dropout_threshold(double p) { return (uint32_t)(p * 4294967296.0); }

// what a kept element holds: 1 / (1 - p), the subtraction in double, the division in float; 0 for p >= 1 (nothing is kept)
RSAF_RNG_HD inline float dropout_keep_value(double p) { return p >= 1.0 ? 0.0f : 1.0f / (float)(1.0 - p); }

RSAF_RNG_HD inline float dropout_value(uint32_t word, uint32_t thr, float keep) { return word >= thr ? keep : 0.0f; }

}  // namespace rng
}  // namespace rsaf
