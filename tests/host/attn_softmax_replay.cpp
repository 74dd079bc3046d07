// Host replay of csrc/attn_softmax.h (tests/test_attn_softmax_host.py): the arithmetic of attn_f16x3_kernel's softmax
// against float64, the kernel's form before it for comparison, the store map of a wave's output, the addresses of the
// transposed V reads, and the walk of the workgroups.  Prints one "ok ..." line per part, or the first failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "attn_softmax.h"

using namespace rsaf::attn;

static int fail(const char* what) { std::printf("FAIL %s\n", what); return 1; }

// ---- 1. arithmetic ----------------------------------------------------------------------------------------------------
// One probability of a row: raw score s under the raw row maximum m (both float accumulators), score scale sscale, row sum
// S of exp(scaled score - scaled maximum) over the row (exact in both forms: a float that either form's own sum rounds to).
// v_exp_f32 and the library's expf are modelled as the float64 function rounded to float (the hardware instruction is
// within 1 ulp of that, the library within 1 ulp too).
// The form before: v = s * sscale, mm = m * sscale, e = expf(v - mm), P = e * (2^14 / S) split; p = (hi + lo) 2^-14.
static double parent_form(float s, float m, float sscale, float S) {
    const float v = s * sscale, mm = m * sscale;
    const float e = (float)std::exp((double)(v - mm));
    const float inv = 16384.0f / S;
    float hi, lo;
    split_value(e * inv, hi, lo);
    return ((double)hi + (double)lo) / 16384.0;
}
// The new form: e = 2^((s - m) c), e 2^14 split; p = (hi + lo) 2^-14 / S.
static double new_form(float s, float m, float sscale, float S) {
    float hi, lo;
    split_value(exp2_bare(exp2_arg(s, m, exp2_scale(sscale))) * P_SCALE, hi, lo);
    return ((double)hi + (double)lo) / 16384.0 / (double)S;
}

static int arithmetic() {
    const float sums[] = {1.0f, 1.0000001f, 1.37f, 2.0f, 3.0f, 7.3f, 16.0f, 17.11f, 100.0f, 255.9f, 256.0f};
    const float maxima[] = {0.0f, 0.7f, -3.3f, 13.37f, 60.0f};                  // the scaled row maximum
    double worst_parent = 0.0, worst_new = 0.0;
    long cases = 0;
    for (int ls = -20; ls <= 4; ++ls) {
        const float sscale = std::ldexp(1.0f, ls);
        double wp = 0.0, wn = 0.0;
        for (float mm : maxima) {
            const float m = mm / sscale;
            for (int gi = 0; gi <= 3600; ++gi) {                                 // gaps 0 .. 133: exp underflows at 87.3 (103.3 with denormals)
                const double gap = gi == 0 ? 0.0 : gi * 0.03711 + (gi % 7) * 1e-4;
                const float s = (float)((double)m - gap / (double)sscale);
                const double g = ((double)m - (double)s) * (double)sscale;       // the gap these two floats stand for
                for (float S : sums) {
                    if (g > 0.0 && (double)S < 1.0 + std::exp(-g)) continue;     // the row holds its maximum and this score
                    const double p = std::exp(-g) / (double)S;
                    const double a = parent_form(s, m, sscale, S), b = new_form(s, m, sscale, S);
                    if (!(a == a) || !(b == b)) return fail("NaN");
                    wp = std::fmax(wp, std::fabs(a - p));
                    wn = std::fmax(wn, std::fabs(b - p));
                    ++cases;
                }
            }
        }
        std::printf("sscale 2^%d: worst |p - p64| parent %.4e new %.4e\n", ls, wp, wn);
        worst_parent = std::fmax(worst_parent, wp);
        worst_new = std::fmax(worst_new, wn);
    }
    // a masked key and a score far below the maximum give exactly 0, never a NaN
    float hi, lo;
    split_value(exp2_bare(exp2_arg(-INFINITY, 3.0f, exp2_scale(0.125f))) * P_SCALE, hi, lo);
    if (hi != 0.0f || lo != 0.0f) return fail("masked key");
    split_value(exp2_bare(exp2_arg(-3.0e38f, 3.0e38f, exp2_scale(16.0f))) * P_SCALE, hi, lo);
    if (hi != 0.0f || lo != 0.0f) return fail("far score");
    // the maximum itself is exactly 2^14
    split_value(exp2_bare(exp2_arg(5.5f, 5.5f, exp2_scale(0.125f))) * P_SCALE, hi, lo);
    if (hi != 16384.0f || lo != 0.0f) return fail("maximum");
    std::printf("worst over the sweep (%ld cases): parent %.6e new %.6e ratio %.4f\n", cases, worst_parent, worst_new,
                worst_new / worst_parent);
    if (!(worst_new <= 1.25 * worst_parent)) return fail("new form farther from float64 than 1.25 x the parent's");
    std::printf("ok arithmetic\n");
    return 0;
}

// ---- 2. store map --------------------------------------------------------------------------------------------------------
static int store_map() {
    // word[lane][ct][gp][w] = the two (query, column) a lane packs into pair word w before the exchange
    typedef std::pair<int, int> QC;
    std::map<std::tuple<int, int, int>, int> written;                            // (query, column, plane) -> times
    for (int ct = 0; ct < 2; ++ct)
        for (int gp = 0; gp < 2; ++gp) {
            std::set<long> bytes[2];
            for (int lane = 0; lane < 64; ++lane) {
                for (int w = 0; w < 4; ++w) {
                    const WordSrc src = swap_source(lane, w);
                    // v_permlane32_swap(word j, word j + 2): lanes 32-63 of the first change places with lanes 0-31 of the second
                    const WordSrc back = swap_source(src.lane, src.word);
                    if (back.lane != lane || back.word != w) return fail("exchange is not an involution");
                    if (src.lane != lane && !((lane >> 5) == 0 ? (src.lane == lane + 32 && w >= 2 && src.word == w - 2)
                                                               : (src.lane == lane - 32 && w < 2 && src.word == w + 2)))
                        return fail("exchange is not the half swap of words (w, w + 2)");
                    if ((src.lane & 31) != (lane & 31)) return fail("exchange crosses queries");
                    for (int half = 0; half < 2; ++half) {
                        const int e = 8 * gp + 2 * src.word + half;               // the register the source lane packed there
                        const QC tag(src.lane & 31, acc_column(src.lane, ct, e));
                        const int k = store_k0(lane) + 2 * w + half, panel = store_panel(ct, gp);
                        if (k < 0 || k > 15 || panel < 0 || panel > 3) return fail("store outside the head's panels");
                        if (tag.second != 16 * panel + k) return fail("a column lands at another column's place");
                        for (int plane = 0; plane < 2; ++plane) ++written[std::make_tuple(lane & 31, tag.second, plane)];
                    }
                }
                // the 16 bytes of this lane within the panel's 32 rows x 32 bytes
                const long at = (long)(lane & 31) * 32 + 2 * store_k0(lane);
                if (at % 16) return fail("store not 16-byte aligned");
                for (int b = 0; b < 16; ++b)
                    if (!bytes[0].insert(at + b).second) return fail("two lanes of one store overlap");
            }
            if (bytes[0].size() != 1024 || *bytes[0].begin() != 0 || *bytes[0].rbegin() != 1023)
                return fail("a store instruction does not cover 1 KB without a gap");
        }
    if (written.size() != 32 * 64 * 2) return fail("not every (query, column, plane) is written");
    for (const auto& kv : written)
        if (kv.second != 1) return fail("a (query, column, plane) is written twice");
    std::printf("ok store map: 32 x 64 x 2 written once, 8 stores of 16 bytes per lane, 1 KB per instruction\n");
    return 0;
}

// ---- 3. transposed V reads ---------------------------------------------------------------------------------------------
// Every read of the immediate-offset form lies inside the staged block and equals the address the kernel computed per step
// before (row, swizzled chunk and column pair from the step's keys).
static int v_reads() {
    if (V_BLOCK != 32768) return fail("block size");
    for (int step = 0; step < 16; ++step) {
        const int t4 = step >> 2, s2 = (step >> 1) & 1, ct = step & 1;
        std::set<int> banks_seen;
        for (int lane = 0; lane < 64; ++lane) {
            const int gq = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
            for (int r8 = 0; r8 < 2; ++r8)
                for (int pl = 0; pl < 2; ++pl) {
                    const int got = (v_lane_bytes(lane) ^ (64 * ct)) + v_step_bytes(step) + r8 * V_ROWS8 + pl * V_LO;
                    const int row = 32 * t4 + 16 * s2 + 4 * (gq >> 1) + tq + 8 * r8;
                    const int ch = (4 * ct + 2 * (gq & 1) + (tp >> 1)) ^ (((row >> 1) & 1) << 2);
                    const int want = 2 * (pl * V_KB * V_HD + row * V_HD + 8 * ch + 4 * (tp & 1));
                    if (got != want) return fail("read address differs from the per-step form");
                    if (got < 0 || got + 8 > V_BLOCK || got % 8) return fail("read outside the block or unaligned");
                }
        }
        // conflict-free within each half of the wave: 32 lanes x 2 words on 64 distinct banks
        for (int hf = 0; hf < 2; ++hf) {
            std::set<int> banks;
            for (int lane = 32 * hf; lane < 32 * hf + 32; ++lane) {
                const int a = (v_lane_bytes(lane) ^ (64 * ct)) + v_step_bytes(step);
                banks.insert((a / 4) % 64);
                banks.insert((a / 4 + 1) % 64);
            }
            if (banks.size() != 64) return fail("bank conflict in a transposed read");
        }
    }
    if (v_step_bytes(15) + V_ROWS8 + V_LO + 64 >= 65536) return fail("immediate offset beyond 16 bits");
    std::printf("ok transposed reads: 16 steps x 64 lanes x 4 reads inside the block, conflict-free\n");
    return 0;
}

// ---- 4. workgroup walk ---------------------------------------------------------------------------------------------------
static int walk() {
    const long sizes[] = {1, 2, 7, 8, 9, 15, 16, 17, 24, 1000, 21024, 24000, 24001};
    for (long pairs : sizes)
        for (int halves = 1; halves <= 2; ++halves) {
            const long grid = grid_size(pairs, halves);
            std::vector<int> seen((size_t)pairs * 2, 0);
            for (long id = 0; id < grid; ++id) {
                const WgSlot sl = wg_slot(id, halves);
                if (sl.half < 0 || sl.half >= halves || sl.pair < 0) return fail("slot out of range");
                if (sl.pair >= pairs) continue;                                   // padding
                ++seen[(size_t)sl.pair * 2 + sl.half];
                if (halves == 2) {                                                // the other half: 8 ids away, same id mod 8
                    const long other = sl.half ? id - 8 : id + 8;
                    const WgSlot so = wg_slot(other, halves);
                    if (other < 0 || other >= grid || so.pair != sl.pair || so.half == sl.half || other % 8 != id % 8)
                        return fail("the halves of a pair are not 8 ids apart");
                }
            }
            for (long p = 0; p < pairs; ++p)
                for (int hf = 0; hf < 2; ++hf)
                    if (seen[(size_t)p * 2 + hf] != (hf < halves ? 1 : 0)) return fail("a (pair, half) is not visited exactly once");
            if (grid >= (1L << 31)) return fail("grid too large");
        }
    std::printf("ok workgroup walk\n");
    return 0;
}

int main(int argc, char** argv) {
    const bool all = argc < 2;
    const std::string which = all ? "" : argv[1];
    int rc = 0;
    if (all || which == "arithmetic") rc |= arithmetic();
    if (all || which == "layout") rc |= store_map() | v_reads() | walk();
    return rc;
}
