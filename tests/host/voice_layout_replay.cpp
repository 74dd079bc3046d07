// Host replay of csrc/mshds_voice_layout.h (g++ -ffp-contract=off; driven by tests/test_voice_layout_host.py).
//   structs  prints "name offset" for every field of ResampleInfo and FormantFrame, and "sizeof.Name size"
//   tile     the resampler's tile at depths 3, 50, 500 and every spread 0..7: the fill loop and the tap loop replayed index
//            by index against the LDS request; the request at depth 500 and the table stride at depths 3..600 against the
//            parent's expressions (voice_layout_parent.inc); every tap index below the stride
//   pulses   PulseWorkspace against the parent's formula, bounds, overlap, alignment; 200 seeded voiced / unvoiced patterns
//            per max_frames against max_st and cap_slots
//   interp   stdin lines "n t1 dt ceiling t v0 .. v(n-1)" (hex floats, nan = undefined) -> "%a %a": value_at_time with
//            NaN as undefined, and pitch_value_at
//   mean     stdin lines "xmin xmax z0 .. z49" -> ltas_mean_rect over the 50 bands of 100 Hz
//   ltas     stdin lines "z0 .. z49" -> "%a %a": slope and tilt of ltas_slope_tilt
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "mshds_voice_layout.h"
#include "voice_layout_parent.inc"

using namespace rsaf::mshds;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static int structs() {
#define AT(S, f) printf(#S "." #f " %zu\n", offsetof(S, f))
    AT(ResampleInfo, sample_off); AT(ResampleInfo, out_off); AT(ResampleInfo, pos0); AT(ResampleInfo, x1o);
    AT(ResampleInfo, n_in); AT(ResampleInfo, n_out); AT(ResampleInfo, table); AT(ResampleInfo, pad);
    AT(FormantFrame, f); AT(FormantFrame, b);
#undef AT
    printf("sizeof.ResampleInfo %zu\nsizeof.FormantFrame %zu\n", sizeof(ResampleInfo), sizeof(FormantFrame));
    return 0;
}

static int tile() {
    for (int depth : {3, 50, 500}) {
        const int request = (int)(rs_lds_bytes(depth) / sizeof(double));
        for (int spread = 0; spread <= RS_MAX_SPREAD; ++spread) {
            const int span = rs_span(depth, spread), nkb = rs_tap_blocks(depth);
            CHECK(span <= rs_span_max(depth), "depth %d spread %d", depth, spread);
            int top = -1;
            for (int i = 0; i < span; ++i) top = rs_skew(i) > top ? rs_skew(i) : top;                  // the fill loop
            int top_tap = -1, top_w = -1;
            for (int ql = 0; ql < 64; ++ql)
                for (int off = 0; off <= spread; ++off) {                                              // pb[r] - bmin of a wave
                    const int i0 = 8 * RS_QL * ql + off;
                    for (int kb = 0; kb < nkb; ++kb)
                        for (int t = 0; t < 8; ++t) {
                            const int i = i0 + 8 * kb + t;
                            CHECK(i < span, "tap loop reads index %d the fill did not write (span %d)", i, span);
                            top_tap = rs_skew(i) > top_tap ? rs_skew(i) : top_tap;
                            top_w = 8 * kb + t > top_w ? 8 * kb + t : top_w;
                        }
                }
            CHECK(top < request && top_tap < request, "depth %d spread %d: %d %d of %d", depth, spread, top, top_tap, request);
            CHECK(top_w < rs_table_stride(depth) && top_w >= rs_taps(depth) - 1, "depth %d: tap %d, stride %d", depth, top_w,
                  rs_table_stride(depth));
        }
    }
    CHECK(rs_lds_bytes(500) == parent::resample_lds_bytes(500), "%zu %zu", rs_lds_bytes(500), parent::resample_lds_bytes(500));
    for (int depth = 3; depth <= 600; ++depth)
        CHECK(rs_table_stride(depth) == parent::table_stride(depth), "depth %d", depth);
    CHECK(rs_n_edge(500) == (int)((double)(500 + 2) * 0.625) + 3, "n_edge");
    printf("ok tile\nlds500 %zu\n", rs_lds_bytes(500));
    return 0;
}

static int pulses() {
    const double grids[3][2] = {{0.005, 500.0}, {0.0075, 250.0}, {0.0125, 600.0}};
    std::mt19937_64 rng(20261021);
    long patterns = 0;
    for (int n_clips : {1, 48, 65535})
        for (int max_frames : {0, 1, 7, 6000})
            for (const auto& g : grids) {
                const PulseWorkspace w(n_clips, max_frames, g[0], g[1]);
                int ms, cs;
                int64_t total;
                parent::pulses_layout(n_clips, max_frames, g[0], g[1], &ms, &cs, &total);
                CHECK(w.max_st == ms && w.cap_slots == cs && w.bytes == total, "%d %d: %d %d %lld / %d %d %lld", n_clips, max_frames,
                      w.max_st, w.cap_slots, (long long)w.bytes, ms, cs, (long long)total);
                const int64_t n = n_clips;
                const int64_t off[6] = {w.left, w.right, w.abs_peak, w.st, w.counts, w.n_st};
                const int64_t size[6] = {n * w.cap_slots * 16, n * w.cap_slots * 8, n * 8, n * w.max_st * (int64_t)sizeof(Stretch),
                                         n * w.max_st * 8, n * 4};
                const int64_t align[6] = {16, 8, 8, 4, 8, 4};
                for (int a = 0; a < 6; ++a) {
                    CHECK(off[a] >= 0 && off[a] + size[a] <= w.bytes, "array %d outside", a);
                    CHECK(off[a] % align[a] == 0, "array %d misaligned", a);
                    for (int b = a + 1; b < 6; ++b)
                        CHECK(off[a] + size[a] <= off[b] || off[b] + size[b] <= off[a], "arrays %d %d overlap", a, b);
                }
                if (n_clips != 1) continue;
                for (int p = 0; p < 200; ++p, ++patterns) {                   // voiced runs of every density, all-voiced and alternating
                    const double dens = p == 0 ? 1.0 : (p == 1 ? 0.5 : (double)(rng() % 1000) / 999.0);
                    int count = 0, slots = 0, run = 0;
                    for (int i = 0; i <= max_frames; ++i) {
                        const bool v = i < max_frames && (p == 1 ? (i & 1) == 0 : (double)(rng() % 1000) / 1000.0 < dens);
                        if (v) { ++run; continue; }
                        if (run) { ++count; slots += stretch_cap(run, g[0], g[1]); run = 0; }
                    }
                    CHECK(count <= w.max_st && slots <= w.cap_slots, "max_frames %d pattern %d: %d of %d stretches, %d of %d slots",
                          max_frames, p, count, w.max_st, slots, w.cap_slots);
                }
            }
    printf("ok pulses\npatterns %ld\n", patterns);
    return 0;
}

static bool read_doubles(std::vector<double>* v) {
    static char line[1 << 16];
    if (!fgets(line, sizeof line, stdin)) return false;
    v->clear();
    for (char* p = strtok(line, " \n"); p; p = strtok(nullptr, " \n")) v->push_back(strtod(p, nullptr));
    return true;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "structs") return structs();
    if (mode == "tile") return tile();
    if (mode == "pulses") return pulses();
    std::vector<double> v;
    while (read_doubles(&v)) {
        if (v.empty()) continue;
        if (mode == "interp") {
            const int n = (int)v[0];
            const double t1 = v[1], dt = v[2], ceiling = v[3], t = v[4];
            if ((int)v.size() != 5 + n) return 2;
            const double* f = v.data() + 5;
            const double a = value_at_time([f](int64_t i) { return f[i]; }, [](double x) { return x == x; }, n, t1, dt, t);
            printf("%a %a\n", a, pitch_value_at(f, n, t1, dt, ceiling, t));
        } else if (mode == "mean") {
            if ((int)v.size() != 2 + LTAS_NB) return 2;
            printf("%a\n", ltas_mean_rect(v.data() + 2, LTAS_NB, 0.5 * LTAS_BW, LTAS_BW, v[0], v[1]));
        } else if (mode == "ltas") {
            if ((int)v.size() != LTAS_NB) return 2;
            double slope, tilt;
            ltas_slope_tilt(v.data(), &slope, &tilt);
            printf("%a %a\n", slope, tilt);
        } else {
            return 2;
        }
    }
    return 0;
}
