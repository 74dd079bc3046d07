// GroupNorm statistics of conv0's output (w2v2_feat.hip): one channel of one window is T0 frames.  Plain C++ (no HIP
// include): tests/test_gn_stats_host.py compiles it with g++ and replays the arithmetic against a long double two-pass
// (tests/host/gn_stats_replay.cpp).
//
// The statistics pass (conv0_kernel<.., APPLY = false, ..>) takes sum y and sum y^2 per slab of frames in float32
// (slab_add); gn_finalize_kernel adds the slabs in double and forms var = q / T0 - mean^2 (moments_of_sums).  That
// subtraction cancels the digits the float sums kept as soon as mean^2 >> var: a DC offset on raw samples
// (do_normalize=False), a conv bias, a window that is all but silent.  The sums are kept for the channels they serve
// (sums_suffice: mean^2 <= var, where the subtraction costs at most one bit; speech under zero-mean normalisation sits below
// 1e-2) and these keep the bits they always had.  Every other channel is summed again by gn_finalize_kernel itself, which
// recomputes its conv0 outputs and accumulates them in double (Sums64: mean^2 / var = 1e5 then costs 1e5 x 2^-53).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GN_HD __host__ __device__ __forceinline__
#else
#define GN_HD inline
#endif

namespace rsaf {
namespace gn {

// one frame of the statistics pass
GN_HD void slab_add(float y, float& s, float& q, float& mx) {
    s += y;
    q += y * y;
    mx = fmaxf(mx, fabsf(y));
}

struct Moments { double mean, var; };

// s, q: the slabs' float sums added in double
GN_HD Moments moments_of_sums(double s, double q, int T0) {
    const double mean = s / T0;
    double var = q / T0 - mean * mean;
    if (var < 0.0) var = 0.0;
    return Moments{mean, var};
}

// whether the float sums gave these moments without cancellation (a NaN or an infinite sum says no)
GN_HD bool sums_suffice(const Moments& m) { return m.mean * m.mean <= m.var; }

// the channel summed again in double
struct Sums64 {
    double s = 0.0, q = 0.0;
    GN_HD void add(float y) { const double d = (double)y; s += d; q = fma(d, d, q); }
};

// GroupNorm (eps 1e-5, biased variance) of the channel as y -> a y + b
GN_HD void coefficients(const Moments& m, float g, float be, float& a, float& b) {
    const double rstd = 1.0 / sqrt(m.var + 1e-5);
    const double ad = (double)g * rstd;
    a = (float)ad;
    b = (float)((double)be - m.mean * ad);
}

}  // namespace gn
}  // namespace rsaf
