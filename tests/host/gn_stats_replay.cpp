// csrc/gn_stats.h on the host: GroupNorm's statistics as conv0_kernel's statistics pass and gn_finalize_kernel form them,
// over seeded channel sequences, against a long double two-pass.
//
// A sequence is one channel of conv0's output: y_t = sum_j w_j x_{5 t + j} (+ bias), float32 FMAs in the kernel's order, the
// weights uniform in +-10^-1/2, the input DC + sd * white noise; 32 channels per row, T0 = 143, 2127 and 8271 frames (one
// partial slab, five slabs with a partial last one, seventeen).  Rows: the six (DC, sd, bias) settings below, a constant
// sequence and an all-zero one.
//
// Per sequence the figure is max_t |a y_t + b - n_t|, n_t = g (y_t - mean) / sqrt(var + 1e-5) + be from the long double
// two-pass, a and b the float coefficients, the expression evaluated in long double: what the statistics cost the normalised
// value.  Three columns:
//   new     the functions of gn_stats.h, driven as the kernels drive them (float sums per slab of STAT_SLAB frames; where
//           they do not suffice, the channel summed again in double); `again`: how many of the row's channels were
//   f32     float32 two-pass statistics (sequential float sums), the coefficients formed from them in the same way
//   parent  the form before: per slab float sum y and sum y^2, var = q / T0 - mean^2 in double.  Printed, not asserted.
// Condition, per row and T0: the worst channel of new <= 4 x the worst channel of f32.  (Channel against channel would be a
// lottery: rounding a and b to float puts a floor of about half an ulp of |b| ~ |mean| / sd under every column, and a single
// sequence of either column may land far below it by chance; `worst new/f32` prints the largest such ratio all the same.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gn_stats.h"
#include "w2v2_layout.h"

using namespace rsaf;
using rsaf::w2v2::STAT_SLAB;

struct Rng {                                                        // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }           // [0, 1)
    double normal() { const double u = 1.0 - uniform(), v = uniform(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); }
};

struct Row { const char* name; double dc, sd, bias; int kind; };   // kind 0: conv0 of DC + noise, 1: constant, 2: zeros
static const Row ROWS[] = {
    {"dc 0    sd 1     bias 0", 0.0, 1.0, 0.0, 0},   {"dc 0.05 sd 0.02  bias 0", 0.05, 0.02, 0.0, 0},
    {"dc 0.1  sd 0.01  bias 0", 0.1, 0.01, 0.0, 0},  {"dc 0.3  sd 0.01  bias 0", 0.3, 0.01, 0.0, 0},
    {"dc 0.5  sd 0.002 bias 0", 0.5, 0.002, 0.0, 0}, {"dc 0    sd 1     bias 3", 0.0, 1.0, 3.0, 0},
    {"constant", 0.0, 0.0, 0.0, 1},                  {"zeros", 0.0, 0.0, 0.0, 2},
};
constexpr int NCH = 32;
static const int FRAMES[] = {143, 2127, 8271};
static const float G = 1.1f, BE = 0.05f;

static long double err_of(const std::vector<float>& y, float a, float b, long double mean, long double var) {
    const long double rstd = 1.0L / sqrtl(var + 1e-5L);
    long double e = 0.0L;
    for (float v : y) {
        const long double n = (long double)G * ((long double)v - mean) * rstd + (long double)BE;
        const long double d = fabsl((long double)a * (long double)v + (long double)b - n);
        if (d > e) e = d;
    }
    return e;
}

int main() {
    bool ok = true;
    int row_id = 0;
    for (const Row& r : ROWS) {
        ++row_id;
        for (int T0 : FRAMES) {
            long double worst_new = 0, worst_f32 = 0, worst_parent = 0, worst_ratio = 0, worst_m2v = 0;
            int n_again = 0;
            for (int c = 0; c < NCH; ++c) {
                Rng rng{(uint64_t)row_id * 1000003u + (uint64_t)T0 * 101u + (uint64_t)c};
                std::vector<float> y((size_t)T0);
                if (r.kind == 0) {
                    float w[10];
                    for (float& v : w) v = (float)((2.0 * rng.uniform() - 1.0) * 0.31622776601683794);
                    const float bias = (float)(r.bias * (0.5 + 0.5 * rng.uniform()));
                    std::vector<float> x((size_t)5 * T0 + 5);
                    for (float& v : x) v = (float)(r.dc + r.sd * rng.normal());
                    for (int t = 0; t < T0; ++t) {
                        float acc = 0.f;
                        for (int j = 0; j < 10; ++j) acc = fmaf(w[j], x[(size_t)5 * t + j], acc);
                        y[(size_t)t] = r.bias != 0.0 ? acc + bias : acc;
                    }
                } else {
                    const float v0 = r.kind == 1 ? (float)(0.25 * (1.0 + rng.uniform())) : 0.f;
                    for (float& v : y) v = v0;
                }
                // the reference: long double two-pass over the float values
                long double mean = 0, var = 0;
                for (float v : y) mean += v;
                mean /= T0;
                for (float v : y) var += ((long double)v - mean) * ((long double)v - mean);
                var /= T0;
                const long double m2v = mean * mean / (var + 1e-5L);
                if (m2v > worst_m2v) worst_m2v = m2v;
                // new: gn_stats.h as the kernels drive it: float sums per slab (+ one slab past the end, as a shorter window of a
                // ragged call sees), added in double; the channel summed again in double where the sums do not suffice
                const int slabs = (T0 + STAT_SLAB - 1) / STAT_SLAB + 1;
                double ss = 0.0, qq = 0.0;
                float mx = 0.f, ymax = 0.f;
                for (int sl = 0; sl < slabs; ++sl) {
                    const int t0 = sl * STAT_SLAB, t1 = T0 < t0 + STAT_SLAB ? T0 : t0 + STAT_SLAB;
                    float s = 0.f, q = 0.f, m = 0.f;
                    for (int t = t0; t < t1; ++t) gn::slab_add(y[(size_t)t], s, q, m);
                    ss += (double)s; qq += (double)q; mx = fmaxf(mx, m);
                }
                for (float v : y) ymax = fmaxf(ymax, fabsf(v));
                if (mx != ymax) { std::printf("FAIL %s T0 %d ch %d: max %g vs %g\n", r.name, T0, c, mx, ymax); ok = false; }
                gn::Moments mo = gn::moments_of_sums(ss, qq, T0);
                const bool again = !gn::sums_suffice(mo);
                if (again) {
                    gn::Sums64 acc;
                    for (float v : y) acc.add(v);
                    mo = gn::moments_of_sums(acc.s, acc.q, T0);
                }
                n_again += again;
                float a, b;
                gn::coefficients(mo, G, BE, a, b);
                const long double e_new = err_of(y, a, b, mean, var);
                // f32: float two-pass, sequential sums
                float s32 = 0.f, q32 = 0.f;
                for (float v : y) s32 += v;
                const float mean32 = s32 / (float)T0;
                for (float v : y) { const float d = v - mean32; q32 += d * d; }
                gn::coefficients(gn::Moments{(double)mean32, (double)(q32 / (float)T0)}, G, BE, a, b);
                const long double e_f32 = err_of(y, a, b, mean, var);
                // parent: sum y and sum y^2 per slab in float, combined in double, var = q / T0 - mean^2
                double ps = 0.0, pq = 0.0;
                for (int t0 = 0; t0 < T0; t0 += STAT_SLAB) {
                    float s = 0.f, q = 0.f;
                    for (int t = t0; t < T0 && t < t0 + STAT_SLAB; ++t) { s += y[(size_t)t]; q += y[(size_t)t] * y[(size_t)t]; }
                    ps += (double)s; pq += (double)q;
                }
                const double pmean = ps / T0;
                double pvar = pq / T0 - pmean * pmean;
                if (pvar < 0.0) pvar = 0.0;
                const double pa = (double)G / std::sqrt(pvar + 1e-5);
                const long double e_parent = err_of(y, (float)pa, (float)((double)BE - pmean * pa), mean, var);
                if (e_new > worst_new) worst_new = e_new;
                if (e_f32 > worst_f32) worst_f32 = e_f32;
                if (e_parent > worst_parent) worst_parent = e_parent;
                const long double ratio = e_f32 > 0 ? e_new / e_f32 : (e_new > 0 ? INFINITY : 0.0L);
                if (ratio > worst_ratio) worst_ratio = ratio;
            }
            std::printf("row %-24s T0 %5d  mean^2/var %9.3Lg  new %.3Le  f32 %.3Le  parent %.3Le  worst new/f32 %.3Lf  parent/f32 %.1Lf  again %d\n",
                        r.name, T0, worst_m2v, worst_new, worst_f32, worst_parent, worst_ratio,
                        worst_f32 > 0 ? worst_parent / worst_f32 : 0.0L, n_again);
            if (!(worst_new <= 4.0L * worst_f32)) {
                std::printf("FAIL %s T0 %d: new %.3Le > 4 x f32 %.3Le\n", r.name, T0, worst_new, worst_f32);
                ok = false;
            }
        }
    }
    std::printf(ok ? "ok gn_stats\n" : "FAILED gn_stats\n");
    return ok ? 0 : 1;
}
