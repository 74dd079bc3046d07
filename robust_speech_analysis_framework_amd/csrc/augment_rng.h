// Counter-based augmentations of the collate launch: the mapping from (seed, epoch, sample, op, element) to what an
// augmentation op does to a sequence, as include/rsaf.h documents it, over the Philox4x32-10 of dropout_rng.h.
// Plain inline code: the kernel of aggregate.hip and a host compiler (tests/host/augment_rng_replay.cpp) read the same
// functions, so what the host replays is what the device computes.  Everything but the normals is integer or
// single-rounded arithmetic; contraction is switched off where a product feeds a sum, so that no compiler fuses them.
#pragma once
#include <cmath>
#include <cstdint>

#include "dropout_rng.h"

#if defined(__clang__)
#define RSAF_RNG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RSAF_RNG_NO_CONTRACT
#endif

namespace rsaf {
namespace rng {

// rsaf_augment_op.kind
static const int AUGMENT_SCALE = 0, AUGMENT_GAUSSIAN_NOISE = 1, AUGMENT_TIME_MASK = 2, AUGMENT_FEATURE_MASK = 3;
static const int AUGMENT_KINDS = 4;
// op s of a pipeline draws its parameters from stream 0x100 + 2 s and its elements from 0x100 + 2 s + 1: above the slots
// of the dropout masks, so that a seed shared with a DropoutStream reuses none of them
static const uint32_t AUGMENT_STREAM0 = 0x100u;

// parameter block of op s: key = (seed low, seed high), counter = (0, 0x100 + 2 s, sample, epoch)
RSAF_RNG_HD inline void augment_param_block(uint64_t seed, uint32_t epoch, uint32_t sample, int s, uint32_t out[4]) {
    philox4x32_10(0u, AUGMENT_STREAM0 + 2u * (uint32_t)s, sample, epoch, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

// element block j of op s (elements 4 j .. 4 j + 3 of the sequence's own [T][D] layout): counter = (j, 0x100 + 2 s + 1, sample, epoch)
RSAF_RNG_HD inline void augment_element_block(uint64_t seed, uint32_t epoch, uint32_t sample, int s, uint32_t j, uint32_t out[4]) {
    philox4x32_10(j, AUGMENT_STREAM0 + 2u * (uint32_t)s + 1u, sample, epoch, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

// floor(p * 2^32) for 0 <= p < 1; p >= 1 travels as `always`
RSAF_RNG_HD inline uint32_t augment_fire_threshold(double p) { return p >= 1.0 ? 0xffffffffu : (uint32_t)(p * 4294967296.0); }

RSAF_RNG_HD inline bool augment_fires(int always, uint32_t fire_threshold, uint32_t w0) { return always || w0 < fire_threshold; }

// u(w) = (w >> 8) * 2^-24 in [0, 1)
RSAF_RNG_HD inline double augment_unit(uint32_t w) { return (double)(w >> 8) * (1.0 / 16777216.0); }

// float32(lo + (hi - lo) * u(w)): difference, product and sum each rounded in double, then one rounding to float
RSAF_RNG_HD inline float augment_uniform(double lo, double hi, uint32_t w) {
    RSAF_RNG_NO_CONTRACT
    const double span = (hi - lo) * augment_unit(w);
    return (float)(lo + span);
}

// the span [start, start + len) that a mask op zeroes out of n frames (or columns): len between floor(n * min_part) and
// floor(n * max_part) by w1, start in [0, n - len] by w2; n >= 0, 0 <= min_part <= max_part <= 1
RSAF_RNG_HD inline void augment_span(int64_t n, double min_part, double max_part, uint32_t w1, uint32_t w2, int64_t* start,
                                     int64_t* len) {
    const int64_t lo = (int64_t)((double)n * min_part), hi = (int64_t)((double)n * max_part);
    *len = lo + (int64_t)(((uint64_t)w1 * (uint64_t)(hi - lo + 1)) >> 32);
    *start = (int64_t)(((uint64_t)w2 * (uint64_t)(n - *len + 1)) >> 32);
}

// two standard normals out of two words (Box-Muller): u1 = ((a >> 8) + 1) * 2^-24 in (0, 1], u2 = (b >> 8) * 2^-24,
// r = sqrt(-2 ln u1), z0 = r cos 2 pi u2, z1 = r sin 2 pi u2.  The accurate library functions, no fast intrinsics.
RSAF_RNG_HD inline void augment_normal_pair(uint32_t a, uint32_t b, float* z0, float* z1) {
    const float u1 = (float)((a >> 8) + 1u) * (1.0f / 16777216.0f);       // exact: an integer <= 2^24 times a power of two
    const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospif(2.0f * u2, &sn, &cs);
#else
    const double angle = 6.283185307179586476925 * (double)u2;
    sn = (float)sin(angle);
    cs = (float)cos(angle);
#endif
    *z0 = r * cs;
    *z1 = r * sn;
}

// normal e & 3 of a block is normal (e & 1) of the pair made of words (0, 1) or (2, 3)
RSAF_RNG_HD inline float augment_normal_of(const uint32_t w[4], unsigned which) {
    const bool upper = (which & 2u) != 0;
    float z0, z1;
    augment_normal_pair(upper ? w[2] : w[0], upper ? w[3] : w[1], &z0, &z1);
    return (which & 1u) ? z1 : z0;
}

}  // namespace rng
}  // namespace rsaf
