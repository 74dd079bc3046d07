// csrc/layer_mix_layout.h on the host: the addressing of h from a position of x, the partition of the backward and the order
// of its sums, replayed as the comment at the head of that file states them (layer_mix.hip follows the same statement).
// Per shape: (1) every float4 position of x lies in exactly one part, no part is empty, and the parts are the runs of `per`
// consecutive positions; (2) h_index maps the (position, layer) pairs one to one onto the float4 of h; (3) for the shapes
// small enough to sum, the replayed dp[l] (thread-strided double sums, xor butterfly over the 64 lanes, four waves left to
// right, parts by lane then butterfly, one rounding to float) lies within 2^-24 |dp64| + 2 n 2^-53 sum|h dx| of a long double
// sum over the same data.  Prints "ok B L T D parts per partials" per shape, then "dx D C floats" for the input-gradient
// scratch of the geometry rows (cnnlstm_layout.h), which tests/test_layer_mix_host.py compares with the library's entries.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cnnlstm_layout.h"
#include "layer_mix_layout.h"

using namespace rsaf::layermix;

static std::string g_row;
static void fail(const std::string& what) {
    std::printf("FAIL %s: %s\n", g_row.c_str(), what.c_str());
    std::exit(1);
}

static uint64_t g_state;
static float next_float() {                     // uniform in (-1, 1) with a few exact zeros, from a 64-bit LCG
    g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
    const int32_t v = (int32_t)(g_state >> 40) - (1 << 23);
    return (float)v / (float)(1 << 23);
}

static void butterfly(std::vector<double>& v) {  // wave_sum_f64: every lane ends with the same sum
    for (int o = 32; o >= 1; o >>= 1) {
        std::vector<double> n(64);
        for (int i = 0; i < 64; ++i) n[i] = v[i] + v[i ^ o];
        v = n;
    }
}

static void check_shape(const Shape& s, bool sums) {
    g_row = std::to_string(s.B) + " " + std::to_string(s.L) + " " + std::to_string(s.T) + " " + std::to_string(s.D);
    if (shape_problem(s)) fail(shape_problem(s));
    const Parts P = make_parts(s);
    if (P.n4 != (int64_t)s.B * s.T * s.D / 4 || P.td4 != (int64_t)s.T * s.D / 4) fail("n4 / td4");
    if (P.parts < 1 || P.parts > MIX_PARTS_MAX) fail("parts out of range");
    // (1) partition
    std::vector<unsigned char> seen(P.n4, 0);
    for (int64_t q = 0; q < P.parts; ++q) {
        const int64_t i0 = q * P.per, i1 = std::min(P.n4, i0 + P.per);
        if (i1 <= i0) fail("part " + std::to_string(q) + " is empty");
        for (int t = 0; t < MIX_THREADS; ++t)
            for (int64_t i = i0 + t; i < i1; i += MIX_THREADS) ++seen[i];
    }
    for (int64_t i = 0; i < P.n4; ++i)
        if (seen[i] != 1) fail("position " + std::to_string(i) + " is in " + std::to_string(seen[i]) + " parts");
    if (partials_doubles(s) != P.parts * s.L) fail("partials_doubles");
    if (forward_blocks(P) < 1 || forward_blocks(P) > MIX_PARTS_MAX) fail("forward_blocks");
    // (2) addressing
    if (P.n4 * s.L <= (int64_t)1 << 26) {
        std::vector<unsigned char> hit(P.n4 * s.L, 0);
        for (int64_t i = 0; i < P.n4; ++i)
            for (int l = 0; l < s.L; ++l) {
                const int64_t k = h_index(P, s.L, i, l);
                if (k < 0 || k >= P.n4 * s.L) fail("h_index leaves h");
                const int64_t b = i / P.td4;
                if (k != ((b * s.L + l) * (int64_t)s.T * s.D + (i - b * P.td4) * 4) / 4) fail("h_index is not [B][L][T][D]");
                ++hit[k];
            }
        for (int64_t k = 0; k < P.n4 * s.L; ++k)
            if (hit[k] != 1) fail("float4 " + std::to_string(k) + " of h is addressed " + std::to_string(hit[k]) + " times");
    }
    // (3) sums
    if (sums) {
        g_state = 0x9E3779B97F4A7C15ULL ^ (uint64_t)(P.n4 * 131 + s.L);
        std::vector<float> h(P.n4 * s.L * 4), dx(P.n4 * 4);
        for (float& v : h) v = next_float();
        for (float& v : dx) v = next_float() * 1e-3f;
        std::vector<double> partials(P.parts * s.L);
        for (int64_t q = 0; q < P.parts; ++q) {
            const int64_t i0 = q * P.per, i1 = std::min(P.n4, i0 + P.per);
            for (int l = 0; l < s.L; ++l) {
                double wave[4];
                for (int w = 0; w < 4; ++w) {
                    std::vector<double> lanes(64, 0.0);
                    for (int lane = 0; lane < 64; ++lane)
                        for (int64_t i = i0 + w * 64 + lane; i < i1; i += MIX_THREADS) {
                            const float* hv = &h[h_index(P, s.L, i, l) * 4];
                            for (int c = 0; c < 4; ++c) lanes[lane] += (double)hv[c] * (double)dx[i * 4 + c];
                        }
                    butterfly(lanes);
                    wave[w] = lanes[0];
                }
                partials[q * s.L + l] = ((wave[0] + wave[1]) + wave[2]) + wave[3];
            }
        }
        const double n = (double)P.n4 * 4;
        for (int l = 0; l < s.L; ++l) {
            std::vector<double> lanes(64, 0.0);
            for (int lane = 0; lane < 64; ++lane)
                for (int64_t q = lane; q < P.parts; q += 64) lanes[lane] += partials[q * s.L + l];
            butterfly(lanes);
            const float dp = (float)lanes[0];
            long double want = 0.0L, mag = 0.0L;
            for (int64_t i = 0; i < P.n4; ++i)
                for (int c = 0; c < 4; ++c) {
                    const long double pr = (long double)h[h_index(P, s.L, i, l) * 4 + c] * (long double)dx[i * 4 + c];
                    want += pr; mag += fabsl(pr);
                }
            const long double bar = ldexpl(fabsl(want), -24) + 2.0L * n * ldexpl(mag, -53);
            if (fabsl((long double)dp - want) > bar)
                fail("dp[" + std::to_string(l) + "] off by " + std::to_string((double)fabsl((long double)dp - want)) + ", bound " + std::to_string((double)bar));
        }
    }
    std::printf("ok %s %lld %lld %lld\n", g_row.c_str(), (long long)P.parts, (long long)P.per, (long long)partials_doubles(s));
}

int main() {
    const Shape summed[] = {
        {2, 13, 5, 20},        // fewer positions than one part, fewer than one workgroup has threads
        {1, 1, 1, 4},          // one position
        {3, 2, 9, 4},          // L = 2
        {1, 3, 4099, 4},       // two parts, the last one position short
        {2, 25, 37, 768},      // four parts at D = 768, L above 16
        {5, 4, 1000, 12},      // B > 1 with parts that straddle batch rows
    };
    for (const Shape& s : summed) check_shape(s, true);
    const Shape walked[] = {{4, 13, 4378, 768}, {4, 13, 20000, 768}, {1, 32, 8191, 8}};   // the part count at its cap
    for (const Shape& s : walked) check_shape(s, false);
    const int geo[][2] = {{4, 4}, {20, 20}, {16, 48}, {64, 16}, {64, 64}, {48, 100}, {36, 272}, {16, 272}, {32, 96}, {192, 144}, {100, 20},
                          {16, 528}, {768, 128}};
    for (const auto& g : geo) {
        const rsaf::cnnlstm::Dims d{g[0], g[1], 64, 2, 1, rsaf::cnnlstm::DIMS_ACT_SILU};
        const int64_t n = rsaf::cnnlstm::dx_scratch_floats(d);
        if (n < (int64_t)g[0] * 3 * g[1] || n % 4 || n >= (int64_t)g[0] * 3 * g[1] + 4) {
            g_row = "dx";
            fail("dx_scratch_floats");
        }
        std::printf("dx %d %d %lld\n", g[0], g[1], (long long)n);
    }
    return 0;
}
