// csrc/augment_rng.h under a host compiler: prints what the collate kernel decides, for tests/test_augment_host.py.
//
//   augment_rng_replay params seed epoch sample s kind a b p n [seed epoch sample s kind a b p n ...]
//       per case one line: "fires <0|1> value <float bits, hex>" for Scale (kind 0) and GaussianNoise (1),
//       "fires <0|1> span <start> <len>" for TimeMask (2) and FeatureMask (3), n the frames or columns the span is taken from
//   augment_rng_replay normals seed epoch sample s n [seed epoch sample s n ...]
//       per case one line: the normals of elements 0 .. n - 1 of op s, as the header's float functions give them on the host
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "augment_rng.h"

using namespace rsaf::rng;

static int usage(const char* me) {
    std::fprintf(stderr, "usage: %s params seed epoch sample s kind a b p n [...] | %s normals seed epoch sample s n [...]\n", me, me);
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return usage(argv[0]);
    if (!std::strcmp(argv[1], "params")) {
        if (argc < 11 || (argc - 2) % 9 != 0) return usage(argv[0]);
        for (int a = 2; a < argc; a += 9) {
            const uint64_t seed = std::strtoull(argv[a], nullptr, 0);
            const uint32_t epoch = (uint32_t)std::strtoull(argv[a + 1], nullptr, 0), sample = (uint32_t)std::strtoull(argv[a + 2], nullptr, 0);
            const int s = std::atoi(argv[a + 3]), kind = std::atoi(argv[a + 4]);
            const double lo = std::strtod(argv[a + 5], nullptr), hi = std::strtod(argv[a + 6], nullptr), p = std::strtod(argv[a + 7], nullptr);
            const int64_t n = std::strtoll(argv[a + 8], nullptr, 0);
            uint32_t w[4];
            augment_param_block(seed, epoch, sample, s, w);
            const int fired = augment_fires(p >= 1.0, augment_fire_threshold(p), w[0]);
            if (kind == AUGMENT_SCALE || kind == AUGMENT_GAUSSIAN_NOISE) {
                const float v = augment_uniform(lo, hi, w[1]);
                uint32_t bits;
                std::memcpy(&bits, &v, 4);
                std::printf("fires %d value %08x\n", fired, bits);
            } else {
                int64_t start, len;
                augment_span(n, lo, hi, w[1], w[2], &start, &len);
                std::printf("fires %d span %" PRId64 " %" PRId64 "\n", fired, start, len);
            }
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "normals")) {
        if (argc < 7 || (argc - 2) % 5 != 0) return usage(argv[0]);
        for (int a = 2; a < argc; a += 5) {
            const uint64_t seed = std::strtoull(argv[a], nullptr, 0);
            const uint32_t epoch = (uint32_t)std::strtoull(argv[a + 1], nullptr, 0), sample = (uint32_t)std::strtoull(argv[a + 2], nullptr, 0);
            const int s = std::atoi(argv[a + 3]);
            const uint64_t n = std::strtoull(argv[a + 4], nullptr, 0);
            uint32_t w[4];
            for (uint64_t e = 0; e < n; ++e) {
                if ((e & 3) == 0) augment_element_block(seed, epoch, sample, s, (uint32_t)(e >> 2), w);
                std::printf("%s%.9g", e ? " " : "", (double)augment_normal_of(w, (unsigned)(e & 3)));
            }
            std::printf("\n");
        }
        return 0;
    }
    return usage(argv[0]);
}
