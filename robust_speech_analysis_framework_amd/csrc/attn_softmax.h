// Lane functions of attn_f16x3_kernel's softmax and its workgroup walk (w2v2_encoder.hip).  Plain C++ (no HIP include):
// tests/test_attn_softmax_host.py compiles it with g++ and replays the arithmetic against float64
// (tests/host/attn_softmax_replay.cpp).
//
// The softmax of one query over its keys, as the kernel runs it:
//   m = max over the keys of the raw score accumulators (the scale is > 0, so it commutes with the max)
//   e = 2^((s - m) * c),  c = scale * log2(e) rounded to float: the subtraction first (exact for the scores near the
//       maximum, the only ones whose probability is not negligible), one multiply, the bare v_exp_f32.  (Folding the 2^14
//       below into the argument as + 14 rounds the argument to 2^-21 absolutely and costs 3.5 x the error: the replay.)
//   P = e * 2^14 split into two fp16 (hi + lo), an operand of the second product.
//       e lies in (0, 1]; the 1 / sum of the normalisation is applied to O together with the 2^-14, so the row sum is not
//       needed before the first MFMA.
// A masked key carries s = -inf: (-inf - m) * c = -inf and 2^-inf = 0.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ATTN_HD __host__ __device__ __forceinline__
#else
#define ATTN_HD inline
#endif

namespace rsaf {
namespace attn {

constexpr float LOG2E = 1.44269504088896340736f;
constexpr int P_SHIFT = 14;
constexpr float P_SCALE = 16384.0f;              // probabilities travel as e * 2^14: |hi + lo| <= 16384 < fp16's 65504

// c of a score scale (q and k both carry the window's power of two, and head width 64 makes the whole scale one)
ATTN_HD float exp2_scale(float sscale) { return sscale * LOG2E; }

// the argument of the base-2 exponential of a score s under the row maximum m
ATTN_HD float exp2_arg(float s, float m, float c) { return (s - m) * c; }

// v_exp_f32: 2^x, within 1 ulp, denormal results flushed (they are below 2^-126: nothing of them reaches an fp16 plane)
ATTN_HD float exp2_bare(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(x);
#else
    return (float)std::exp2((double)x);          // the host model: float64 exp2 rounded to float
#endif
}

// The nearest fp16 value of x (ties to even, fp16 denormals kept), as a float; |x| < 65520.  Plain arithmetic, so that a
// host compiler without an fp16 type can replay the splits.
ATTN_HD float half_round(float x) {
    if (x == 0.0f || !(x - x == 0.0f)) return x;
    int e;
    std::frexp(x, &e);                                       // |x| = f 2^e, f in [0.5, 1): 11 significant bits end at 2^(e - 11)
    const float q = std::ldexp(1.0f, (e < -13 ? -13 : e) - 11);   // below 2^-14 the grid stays at 2^-24
    return std::nearbyint(x / q) * q;
}
// x -> hi + lo, both fp16 values: hi = fp16(x), lo = fp16(x - hi); x - hi is exact in float, so each is rounded once
ATTN_HD void split_value(float x, float& hi, float& lo) {
    hi = half_round(x);
    lo = half_round(x - hi);
}
#if defined(__HIPCC__)
// split_value of two floats, packed (x in the low halves of hi2 and lo2): the packed convert, then per element one
// mixed-precision fma fp16(hi * -1 + x), which reads hi as fp16 and writes one half of lo2.  The convert is the
// compiler's, so that it keeps the wait states between whatever produced x and y (a v_exp_f32, an MFMA) and their first
// reader; the fmas are asm (the compiler folds the expression into convert-back, subtract, convert), and the s_nop covers
// the two wait states a reader of the half-written lo2 may need (v_permlane32_swap), which the compiler cannot see.
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split2(float x, float y, unsigned& hi2, unsigned& lo2) {
    hi2 = __builtin_bit_cast(unsigned, __builtin_convertvector(float2_t{x, y}, half2_t));
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lo2) : "v"(hi2), "v"(x));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\ts_nop 1" : "+v"(lo2) : "v"(hi2), "v"(y));
}
#endif

// The transposed reads of the V fragments (ds_read_b64_tr_b16: per group of 16 lanes 4 keys x 16 columns).  A staged block
// holds 128 keys x 64 halfs per plane, the 16-byte chunk c of key row r at chunk c ^ (((r >> 1) & 1) << 2).  Step
// 4 t4 + 2 s2 + ct of a block reads keys 32 t4 + 16 s2 .. + 15 of column tile ct: lane group gq = lane >> 4 takes keys
// 4 (gq >> 1) + tq (and the same + 8) and columns 16 (gq & 1) + 4 tp .. + 3, tq = (lane & 15) >> 2, tp = lane & 3.  The
// swizzle term depends on tq alone, so a read's byte address within the block is
//   (v_lane_bytes(lane) ^ (64 ct)) + v_step_bytes(step) + {0, V_ROWS8} + {0, V_LO}.
constexpr int V_HD = 64, V_KB = 128;                                             // AttnLds::HD, AttnLds::KB (w2v2_layout.h)
constexpr int V_ROWS8 = 2 * 8 * V_HD, V_LO = 2 * V_KB * V_HD, V_BLOCK = 2 * V_LO;   // bytes: 8 keys on, the lo plane, a block
ATTN_HD int v_lane_bytes(int lane) {
    const int gq = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
    return 2 * ((4 * (gq >> 1) + tq) * V_HD + 8 * ((2 * (gq & 1) + (tp >> 1)) + (((tq >> 1) & 1) << 2)) + 4 * (tp & 1));
}
constexpr int v_step_bytes(int step) { return 2 * (32 * (step >> 2) + 16 * ((step >> 1) & 1)) * V_HD; }

// The store map of a wave's 32 queries x 64 columns.  The accumulator of O^T (v_mfma_f32_32x32x16 C layout) holds on lane
// (query l = lane & 31, half h = lane >> 5) in register e of column tile ct the column acc_column(): four consecutive
// columns per group of four registers.  Registers 8 gp .. 8 gp + 7 of tile ct are k = 4 h .. 4 h + 3 (pair words 0, 1) and
// k = 8 + 4 h .. + 3 (words 2, 3) of the k16 panel 2 ct + gp of the head.  The halves then exchange: words 0, 1 of the upper
// half change places with words 2, 3 of the lower one (swap_source() names where a lane's word comes from), after which
// the lane holds the 8 consecutive k from store_k0() of its query's row: 16 bytes per plane, one store each.
ATTN_HD int acc_column(int lane, int ct, int e) { return 32 * ct + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }
ATTN_HD int store_panel(int ct, int gp) { return 2 * ct + gp; }                 // of the head's four
ATTN_HD int store_k0(int lane) { return 8 * (lane >> 5); }
struct WordSrc { int lane, word; };
ATTN_HD WordSrc swap_source(int lane, int word) {                                // v_permlane32_swap(word w, word w + 2), w = 0, 1
    const int h = lane >> 5;
    if (h == 0 && word >= 2) return WordSrc{lane + 32, word - 2};
    if (h == 1 && word < 2) return WordSrc{lane - 32, word + 2};
    return WordSrc{lane, word};
}

// The walk of the workgroups over (window x head, query half).  The hardware deals consecutive workgroup ids to the 8
// XCDs in turn, each with an L2 of its own; the two query halves of a (window, head) read the same K and V, so they are
// given ids 8 apart: same XCD, dispatched one after the other, and the second one's K / V reads find the first one's
// lines in that L2 instead of going to HBM again.  Ids come in groups of 16 = 8 pairs x 2 halves; grid_size() pads the
// last group, and a workgroup whose pair is >= pairs has nothing to do.
struct WgSlot { int64_t pair; int half; };
ATTN_HD WgSlot wg_slot(int64_t id, int halves) {
    if (halves == 1) return WgSlot{id, 0};
    return WgSlot{(id >> 4) * 8 + (id & 7), (int)((id >> 3) & 1)};
}
ATTN_HD int64_t grid_size(int64_t pairs, int halves) { return halves == 1 ? pairs : 16 * ((pairs + 7) / 8); }

}  // namespace attn
}  // namespace rsaf
