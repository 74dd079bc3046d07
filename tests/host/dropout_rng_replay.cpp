// csrc/dropout_rng.h under a host compiler: prints what the mask kernel computes, for tests/test_dropout_rng_host.py.
//
//   dropout_rng_replay kat c0 c1 c2 c3 k0 k1        (hex)  -> the four output words of Philox4x32-10
//   dropout_rng_replay seed step slot n p [seed step slot n p ...]
//       per case two lines: "words" + the raw word of every element, "mask" + the bits of every mask float (hex)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dropout_rng.h"

using namespace rsaf::rng;

int main(int argc, char** argv) {
    if (argc == 8 && !std::strcmp(argv[1], "kat")) {
        uint32_t v[6], out[4];
        for (int i = 0; i < 6; ++i) v[i] = (uint32_t)std::strtoul(argv[2 + i], nullptr, 16);
        philox4x32_10(v[0], v[1], v[2], v[3], v[4], v[5], out);
        std::printf("%08x %08x %08x %08x\n", out[0], out[1], out[2], out[3]);
        return 0;
    }
    if (argc < 6 || (argc - 1) % 5 != 0) {
        std::fprintf(stderr, "usage: %s kat c0 c1 c2 c3 k0 k1 | %s seed step slot n p [...]\n", argv[0], argv[0]);
        return 2;
    }
    for (int a = 1; a < argc; a += 5) {
        const uint64_t seed = std::strtoull(argv[a], nullptr, 0), step = std::strtoull(argv[a + 1], nullptr, 0);
        const uint32_t slot = (uint32_t)std::strtoul(argv[a + 2], nullptr, 0);
        const uint64_t n = std::strtoull(argv[a + 3], nullptr, 0);
        const double p = std::strtod(argv[a + 4], nullptr);
        const uint32_t thr = dropout_threshold(p);
        const float keep = dropout_keep_value(p);
        uint32_t w[4];
        std::printf("words");
        for (uint64_t e = 0; e < n; ++e) {
            if ((e & 3) == 0) dropout_block(seed, step, slot, (uint32_t)(e >> 2), w);
            std::printf(" %08x", w[e & 3]);
        }
        std::printf("\nmask");
        for (uint64_t e = 0; e < n; ++e) {
            if ((e & 3) == 0) dropout_block(seed, step, slot, (uint32_t)(e >> 2), w);
            const float v = p >= 1.0 ? 0.0f : dropout_value(w[e & 3], thr, keep);
            uint32_t bits;
            std::memcpy(&bits, &v, 4);
            std::printf(" %08x", bits);
        }
        std::printf("\n");
    }
    return 0;
}
