// What more than one MSHDS translation unit uses (mshds.hip, mshds_pitch.hip, mshds_formant.hip, mshds_pulses.hip,
// mshds_ltas.hip, mshds_cpp.hip): the clip table rows, Praat's sample-index rounding, the wave / lane-group helpers of the
// sinc interpolation, and Brent's search for a maximum (pitch candidates, syllable nuclei).
// Every MSHDS .hip includes this header before any code of its own: the three headers below are compiled with FMA
// contraction on, everything after the pragma (the rest of this header and the including file) with it off.
#pragma once
#include "praat_interp.h"
#include "rsaf_common.h"
#include "wave_fft.h"

// Frame times sit exactly on half-sample positions, where Praat's nearest/low index rounding is
// decided by the last bit: evaluate t1 + f*dt etc. as separately rounded IEEE operations (no FMA
// contraction), exactly like the float64 host arithmetic of the oracle.
#pragma clang fp contract(off)

namespace rsaf {
namespace mshds {

constexpr double DXS = 1.0 / 16000.0;
constexpr double PI = 3.14159265358979323846;
constexpr double GOLD = 0.38196601125010515180;   // (3 - sqrt 5) / 2

struct ClipInfo {       // one entry per clip of a launch (host-built)
    int64_t sample_off;
    int64_t frame_off;  // first frame of this clip in the per-launch frame buffers
    double t1;          // time of the first frame
    int n_samples;
    int n_frames;
    double x1;          // time of the first sample (0.5 dx for a sound read from a 16 kHz file; Praat's centred grid after Sound_resample)
    double xmax;        // end of the sound's time domain [0, xmax] (n dx for a file; the ORIGINAL duration after Sound_resample)
};

typedef double double2_t __attribute__((ext_vector_type(2)));

// Sampled_xToLowIndex / xToNearestIndex / xToHighIndex of the sound (0-based), x1 = time of its first sample
// (Praat rounds the 1-based real index (x - x1) / dx + 1; the + 1.0 stays a separately rounded operation: fp contract is off)
__device__ __forceinline__ int64_t low_index(double t, double x1) { return (int64_t)floor((t - x1) / DXS + 1.0) - 1; }
__device__ __forceinline__ int64_t nearest_index(double t, double x1) { return (int64_t)floor(((t - x1) / DXS + 1.0) + 0.5) - 1; }
__device__ __forceinline__ int64_t high_index(double t, double x1) { return (int64_t)ceil((t - x1) / DXS + 1.0) - 1; }

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// cos(x) for x in [0, pi] (all arguments of the sinc window are): fold to [0, pi/2] and evaluate the
// degree-18 Taylor polynomial in x^2 (remainder (pi/2)^20/20! = 3.4e-15).  The library cos/sincos cost
// ~1k cycles each in fp64 and dominated this kernel; this is ~12 FMAs.
__device__ __forceinline__ double cos_0_pi(double x) {
    const bool hi = x > 0.5 * PI;
    const double y = hi ? PI - x : x;
    const double z = y * y;
    double p = -1.0 / 6402373705728000.0;              // -1/18!
    p = p * z + 1.0 / 20922789888000.0;                // 1/16!
    p = p * z - 1.0 / 87178291200.0;                   // -1/14!
    p = p * z + 1.0 / 479001600.0;                     // 1/12!
    p = p * z - 1.0 / 3628800.0;                       // -1/10!
    p = p * z + 1.0 / 40320.0;                         // 1/8!
    p = p * z - 1.0 / 720.0;                           // -1/6!
    p = p * z + 1.0 / 24.0;
    p = p * z - 0.5;
    p = p * z + 1.0;
    return hi ? -p : p;
}
__device__ __forceinline__ double sin_0_pi(double x) { return cos_0_pi(fabs(0.5 * PI - x)); }

// 1/d for d > 0: hardware reciprocal estimate + two Newton steps (full double accuracy, ~5 ops instead
// of the ~15-op IEEE division sequence)
__device__ __forceinline__ double fast_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = r * (2.0 - d * r);
    r = r * (2.0 - d * r);
    return r;
}

// LDS that the lanes of ONE wave wrote becomes visible to its other lanes (a wave's LDS operations complete in order: this
// orders the compiler's accesses and keeps the wave's lanes together)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double readlane_f64(double v, int l) {      // l must be wave-uniform
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// Sum over each aligned group of G lanes, result in every lane of the group.  The 16-lane part is four DPP
// steps (xor 1, xor 2, half-row mirror, row mirror: VALU latency, no LDS crossbar); rows are then combined
// through scalar registers.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int G>
__device__ __forceinline__ double group_sum(double v) {
    v += dpp_f64<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);     // row_half_mirror
    v += dpp_f64<0x140>(v);     // row_mirror
    if (G == 16) return v;
    const double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
    if (G == 64) return (r0 + r1) + (r2 + r3);
    return (threadIdx.x & 32) ? r2 + r3 : r0 + r1;
}

// maximum over the wave in every lane, same DPP / readlane structure (a ds_bpermute butterfly costs six LDS-crossbar
// round trips per reduction: in the pitch frame kernels, three reductions per frame, that was a third of the time in
// front of the correlation)
__device__ __forceinline__ double wave_max_dpp(double v) {
    v = fmax(v, dpp_f64<0xB1>(v));
    v = fmax(v, dpp_f64<0x4E>(v));
    v = fmax(v, dpp_f64<0x141>(v));
    v = fmax(v, dpp_f64<0x140>(v));
    const double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
    return fmax(fmax(r0, r1), fmax(r2, r3));
}

// ---- sinc interpolation of an LDS array by a G-lane group (Praat NUM_interpolate_sinc) -----------------
// y: n samples (0-based); x: 0-based real position; only indices in [nz_lo, nz_hi] can be non-zero.
// Every lane of the wave must call this (the 64/G groups of a wave evaluate different x).
// RECUR: the raised-cosine window angle advances by a fixed step per term, so each lane rotates
// (cos, sin) by the group stride instead of evaluating the polynomial per term (pays for long kernels).
template <int G, bool RECUR>
__device__ double sinc_group(const double* __restrict__ y, int n, double x, int depth, int nz_lo, int nz_hi, int lg) {
    const double x1 = x + 1.0;
    const int midleft = (int)floor(x1), midright = midleft + 1;
    const bool special = (x1 > n) | (x1 < 1) | (x1 == (double)midleft);
    int si = x1 > n ? n - 1 : (x1 < 1 ? 0 : midleft - 1);
    si = si < 0 ? 0 : (si > n - 1 ? n - 1 : si);
    int d = depth;
    if (d > midright - 1) d = midright - 1;
    if (d > n - midleft) d = n - midleft;
    if (d < 0 || special) d = 0;
    const int left = midright - d, right = midleft + d;
    double acc = 0.0;
    const double a0l = PI * (x1 - midleft);               // in (0, pi) unless special
    const double hs = special ? 0.0 : 0.5 * sin_0_pi(a0l); // sin(pi - a) = sin(a): same for both halves
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        // left half: 1-based ix = midleft - k; right half: ix = midright + k; k = 0..d-1.  The window
        // angle (a0 + pi k) / den stays in (0, pi).  [kmin, kmax) drops the all-zero parts of y.
        const double a0 = half == 0 ? a0l : PI * (midright - x1);
        const double iden = fast_rcp(half == 0 ? x1 - left + 1.0 : right - x1 + 1.0);
        int kmin, kmax = d;
        if (half == 0) {
            kmin = midleft - 1 - nz_hi;
            if (midleft - kmax < nz_lo) kmax = midleft - nz_lo;
        } else {
            kmin = nz_lo - midright + 1;
            if (midright + kmax - 2 > nz_hi) kmax = nz_hi - midright + 2;
        }
        kmin = kmin < 0 ? 0 : kmin;
        const int k0 = kmin + lg;
        // G is even: every term of a lane has the sign of its first one, (-1)^k0 hs is applied once behind the loop
        double part = 0.0;
        if (RECUR) {
            const double th = (a0 + PI * k0) * iden, st = (PI * G) * iden;   // st < pi whenever a lane has 2+ terms
            double c = cos_0_pi(fmin(th, PI)), sn = sin_0_pi(fmin(th, PI));
            const double C = cos_0_pi(fmin(st, PI)), S = sin_0_pi(fmin(st, PI));
            for (int k = k0; k < kmax; k += G) {
                const int idx = half == 0 ? midleft - k - 1 : midright + k - 1;
                const double a = a0 + PI * k;
                part += y[idx] * (fast_rcp(a) * (1.0 + c));
                const double c2 = c * C - sn * S;
                sn = sn * C + c * S;
                c = c2;
            }
        } else {
            for (int k = k0; k < kmax; k += G) {
                const int idx = half == 0 ? midleft - k - 1 : midright + k - 1;
                const double a = a0 + PI * k;
                part += y[idx] * (fast_rcp(a) * (1.0 + cos_0_pi(a * iden)));
            }
        }
        acc += ((k0 & 1) ? -hs : hs) * part;
    }
    acc = group_sum<G>(acc);
    return special ? y[si] : acc;
}

// Praat NUMimproveMaximum: Brent's minimiser in the netlib fminbr form on f (= minus the interpolated curve, a function
// of the 1-based position) over [ix1 - 1, ix1 + 1], tolerance sqrt(eps)*|x| + tol/3 on the position, <= 60 iterations.
// Every lane of the wave evaluates f in every iteration (f may exchange data between lanes); `live` = this lane holds a
// real candidate, and the loop runs while any lane's candidate is still active.  Returns the 0-based position and the maximum.
template <class F>
__device__ __forceinline__ void brent_maximise(F f, double ix1, bool live, double& xm, double& ym) {
    const double SQRT_EPS = 1.4901161193847656e-08, TOL3 = 1e-10 / 3.0;
    double a = ix1 - 1.0, b = ix1 + 1.0;
    double v = a + GOLD * (b - a);
    double fv = f(v);
    double x = v, w = v, fx = fv, fw = fv;
    bool active = live;
    for (int it = 0; it < 60; ++it) {
        const double rng = b - a, mid = 0.5 * (a + b);
        const double tol_act = SQRT_EPS * fabs(x) + TOL3;
        if (fabs(x - mid) + 0.5 * rng <= 2.0 * tol_act) active = false;
        if (!__any(active)) break;
        double step = GOLD * (x < mid ? b - x : a - x);
        if (fabs(x - w) >= tol_act) {
            const double t = (x - w) * (fx - fv);
            double q = (x - v) * (fx - fw);
            double p = (x - v) * q - (x - w) * t;
            q = 2.0 * (q - t);
            if (q > 0.0) p = -p; else q = -q;
            if (fabs(p) < fabs(step * q) && p > q * (a - x + 2.0 * tol_act) && p < q * (b - x - 2.0 * tol_act))
                step = p / q;
        }
        if (fabs(step) < tol_act) step = step > 0.0 ? tol_act : -tol_act;
        const double tt = x + step;
        const double ft = f(tt);
        if (active) {
            if (ft <= fx) {
                if (tt < x) b = x; else a = x;
                v = w; w = x; x = tt;
                fv = fw; fw = fx; fx = ft;
            } else {
                if (tt < x) a = tt; else b = tt;
                if (ft <= fw || w == x) { v = w; w = tt; fv = fw; fw = ft; }
                else if (ft <= fv || v == x || v == w) { v = tt; fv = ft; }
            }
        }
    }
    xm = x - 1.0;
    ym = -fx;
}

// ... on the sinc interpolation of an LDS array around the 0-based position ix0.  One G-lane group per candidate;
// `live` = this group holds a real candidate (others just keep the wave's shuffles uniform).
template <int G, bool RECUR>
__device__ void improve_max_group(const double* __restrict__ y, int n, double ix0, int depth, int nz_lo, int nz_hi,
                                  int lg, bool live, double& xm, double& ym) {
    brent_maximise([&](double v1) { return -sinc_group<G, RECUR>(y, n, v1 - 1.0, depth, nz_lo, nz_hi, lg); }, ix0 + 1.0,
                   live, xm, ym);
}

}  // namespace mshds
}  // namespace rsaf
