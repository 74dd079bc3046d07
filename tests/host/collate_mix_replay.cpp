// The mix inside the collate launch (csrc/layer_mix_layout.h, second half) on the host: layer stacks that lie in an arena as
// blocks of L T_b rows, layer-major, mixed into a batch padded to T frames, and dL/dp from the same blocks.
// Per case (the members' frame counts, L, D):
// (1) block_row maps the (b, l, t) of all members one to one onto the arena rows, and block_inside holds for every member
//     that has frames; a block moved past the end of the arena, or before its start, is not inside;
// (2) the forward's chunk walk (mix_chunks workgroups per member, MIXC_PER_THREAD float4 per lane) writes every float4 of
//     out exactly once, a ragged last chunk and a member shorter than one chunk included, and what it writes (mix_term over
//     the block, +0.0 elsewhere) has the bits of the dense forward (h_index, mix_term) on the zero-padded stack;
// (3) the backward's skipping sum, replayed in the stated order with the kernel's stepping of (b, t, c) and dx non-zero on
//     the padded frames too, equals the dense sum over the zero-padded stack bit for bit: every partial double and the
//     float after the final rounding.
// Prints "ok <B> <L> <T> <D> <parts> <chunks per member>" per case.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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

struct V4 {
    float x, y, z, w;
};

static void butterfly(std::vector<double>& v) {  // wave_sum_f64: every lane ends with the same sum
    for (int o = 32; o >= 1; o >>= 1) {
        std::vector<double> n(64);
        for (int i = 0; i < 64; ++i) n[i] = v[i] + v[i ^ o];
        v = n;
    }
}

static bool same_bits(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

// the lanes of one part -> partials[l] as the kernels reduce them
static double reduce_part(const std::vector<double>& lanes256) {
    double wave[4];
    for (int w = 0; w < 4; ++w) {
        std::vector<double> lanes(lanes256.begin() + w * 64, lanes256.begin() + (w + 1) * 64);
        butterfly(lanes);
        wave[w] = lanes[0];
    }
    return ((wave[0] + wave[1]) + wave[2]) + wave[3];
}

static float final_sum(const std::vector<double>& partials, int64_t parts, int L, int l) {
    std::vector<double> lanes(64, 0.0);
    for (int lane = 0; lane < 64; ++lane)
        for (int64_t q = lane; q < parts; q += 64) lanes[lane] += partials[q * L + l];
    butterfly(lanes);
    return (float)lanes[0];
}

static void check_case(const std::vector<int>& len, int L, int D) {
    const int B = (int)len.size();
    int T = 0;
    for (int n : len) T = std::max(T, n);
    g_row = std::to_string(B) + " " + std::to_string(L) + " " + std::to_string(T) + " " + std::to_string(D);
    const Shape s{B, L, T, D};
    if (shape_problem(s)) fail(shape_problem(s));
    const Parts P = make_parts(s);
    const int64_t w4 = D / 4;
    // the store: blocks back to back, frame offsets in frames
    std::vector<int64_t> start(B);
    int64_t frames = 0;
    for (int b = 0; b < B; ++b) { start[b] = (int64_t)L * frames; frames += len[b]; }
    const int64_t arena_rows = (int64_t)L * frames;
    // (1) addressing
    std::vector<unsigned char> hit(arena_rows, 0);
    for (int b = 0; b < B; ++b) {
        if (block_inside(start[b], len[b], L, arena_rows) != (len[b] > 0)) fail("block_inside of member " + std::to_string(b));
        if (len[b] > 0 && (block_inside(start[b] + 1 + arena_rows - (start[b] + (int64_t)L * len[b]), len[b], L, arena_rows) ||
                           block_inside(-1, len[b], L, arena_rows) || block_inside(start[b], len[b], L, start[b] + (int64_t)L * len[b] - 1)))
            fail("a block that leaves the arena counts as inside");
        for (int l = 0; l < L; ++l)
            for (int t = 0; t < len[b]; ++t) {
                const int64_t r = block_row(start[b], len[b], l, t);
                if (r < 0 || r >= arena_rows) fail("block_row leaves the arena");
                ++hit[r];
            }
    }
    for (int64_t r = 0; r < arena_rows; ++r)
        if (hit[r] != 1) fail("arena row " + std::to_string(r) + " is addressed " + std::to_string(hit[r]) + " times");
    // data: the arena, its zero-padded stack h [B][L][T][D], p and dx (non-zero on padded frames too)
    g_state = 0x9E3779B97F4A7C15ULL ^ (uint64_t)(P.n4 * 131 + L);
    std::vector<float> arena(arena_rows * D), h((size_t)P.n4 * L * 4, 0.0f), p(L), dx((size_t)P.n4 * 4);
    for (float& v : arena) v = next_float();
    for (float& v : p) v = 0.5f * (next_float() + 1.0f);
    for (float& v : dx) v = next_float() * 1e-3f;
    for (int b = 0; b < B; ++b)
        for (int l = 0; l < L; ++l)
            for (int t = 0; t < len[b]; ++t)
                std::memcpy(&h[(((size_t)b * L + l) * T + t) * D], &arena[block_row(start[b], len[b], l, t) * D], sizeof(float) * D);
    // (2) forward: the chunk walk of every member against the dense forward
    const int64_t chunks = mix_chunks(T, D), end = (int64_t)T * w4;
    if (chunks != (end + MIXC_CHUNK - 1) / MIXC_CHUNK) fail("mix_chunks");
    std::vector<V4> out((size_t)P.n4);
    std::vector<unsigned char> wrote((size_t)P.n4, 0);
    for (int b = 0; b < B; ++b) {
        const bool inside = block_inside(start[b], len[b], L, arena_rows);
        const int64_t n = inside ? std::min<int64_t>(len[b], T) : 0, hi = n * w4, stride = (int64_t)len[b] * w4;
        const V4* src = reinterpret_cast<const V4*>(arena.data()) + (inside ? start[b] : 0) * w4;
        for (int64_t chunk = 0; chunk < chunks; ++chunk)
            for (int lane = 0; lane < MIX_THREADS; ++lane)
                for (int j = 0; j < MIXC_PER_THREAD; ++j) {
                    const int64_t e = chunk * MIXC_CHUNK + lane + (int64_t)j * MIX_THREADS;
                    V4 a{0.f, 0.f, 0.f, 0.f};
                    if (e < hi)
                        for (int l = 0; l < L; ++l) mix_term(a, p[l], src[(int64_t)l * stride + e], l == 0);
                    if (e < end) {
                        out[(size_t)b * end + e] = a;
                        ++wrote[(size_t)b * end + e];
                    }
                }
    }
    const V4* h4 = reinterpret_cast<const V4*>(h.data());
    for (int64_t i = 0; i < P.n4; ++i) {
        if (wrote[i] != 1) fail("float4 " + std::to_string(i) + " of out is written " + std::to_string(wrote[i]) + " times");
        V4 a;
        for (int l = 0; l < L; ++l) mix_term(a, p[l], h4[h_index(P, L, i, l)], l == 0);
        if (!same_bits(&a, &out[i], sizeof a)) fail("float4 " + std::to_string(i) + " of out differs from the dense forward");
        const int64_t t = (i % P.td4) / w4;
        const V4 zero{0.f, 0.f, 0.f, 0.f};
        if (t >= len[i / P.td4] && !same_bits(&out[i], &zero, sizeof zero)) fail("padding is not +0.0");
    }
    // (3) backward: dense over the padded stack, and skipping over the blocks with the kernel's stepping
    std::vector<double> dense(P.parts * L), skip(P.parts * L);
    const V4* g4 = reinterpret_cast<const V4*>(dx.data());
    for (int64_t q = 0; q < P.parts; ++q) {
        const int64_t i0 = q * P.per, i1 = std::min(P.n4, i0 + P.per);
        for (int l = 0; l < L; ++l) {
            std::vector<double> a(MIX_THREADS, 0.0), c(MIX_THREADS, 0.0);
            for (int tid = 0; tid < MIX_THREADS; ++tid) {
                for (int64_t i = i0 + tid; i < i1; i += MIX_THREADS) {
                    const V4 v = h4[h_index(P, L, i, l)], g = g4[i];
                    double sum = a[tid];
                    sum += (double)v.x * (double)g.x; sum += (double)v.y * (double)g.y;
                    sum += (double)v.z * (double)g.z; sum += (double)v.w * (double)g.w;
                    a[tid] = sum;
                }
                int64_t i = i0 + tid;
                if (i >= i1) continue;
                int64_t b0;
                MixPos pos = mix_first_pos(P, (uint32_t)w4, (uint32_t)T, i0, (uint32_t)tid, &b0);
                if (b0 != i0 / P.td4) fail("b0 of the part");
                for (; i < i1; i += MIX_THREADS) {
                    const int64_t b = b0 + pos.db, t = pos.t, cc = pos.c;
                    if (b >= B) fail("the stepping leaves the batch");
                    if (b != i / P.td4 || t != (i % P.td4) / w4 || cc != i % w4) fail("the stepping of (b, t, c) loses position " + std::to_string(i));
                    const bool inside = block_inside(start[b], len[b], L, arena_rows);
                    const int64_t n = inside ? std::min<int64_t>(len[b], T) : 0;
                    if (t < n) {
                        const V4 v = reinterpret_cast<const V4*>(arena.data())[block_row(start[b], len[b], l, t) * w4 + cc], g = g4[i];
                        double sum = c[tid];
                        sum += (double)v.x * (double)g.x; sum += (double)v.y * (double)g.y;
                        sum += (double)v.z * (double)g.z; sum += (double)v.w * (double)g.w;
                        c[tid] = sum;
                    }
                    mix_step_pos(pos, (uint32_t)w4, (uint32_t)T);
                }
            }
            dense[q * L + l] = reduce_part(a);
            skip[q * L + l] = reduce_part(c);
        }
    }
    if (!same_bits(dense.data(), skip.data(), sizeof(double) * dense.size())) fail("a partial sum of the skipping backward differs from the dense one");
    for (int l = 0; l < L; ++l) {
        const float a = final_sum(dense, P.parts, L, l), c = final_sum(skip, P.parts, L, l);
        if (!same_bits(&a, &c, sizeof a)) fail("dp[" + std::to_string(l) + "] differs after the final rounding");
    }
    std::printf("ok %s %lld %lld\n", g_row.c_str(), (long long)P.parts, (long long)chunks);
}

int main() {
    check_case({5, 3, 0, 5}, 1, 4);            // a member of no frames, members shorter than one chunk, L = 1
    check_case({7, 2, 6}, 2, 20);              // D / 4 = 5: positions step over frames unevenly
    check_case({37, 11, 29, 1}, 13, 768);      // 14 chunks per member, the last one ragged; 7 104 float4 per member
    check_case({33}, 32, 20);                  // L at its cap
    check_case({1367, 900}, 2, 768);           // 129 parts, parts that straddle the two members
    return 0;
}
