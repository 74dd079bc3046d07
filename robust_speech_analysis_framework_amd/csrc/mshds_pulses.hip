// MSHDS glottal pulses, float64 kernels for gfx950: Sound & Pitch: To PointProcess (cc), which _extract_Slope_Tilt (:227-251),
// _measureFormants (:303-338) of src/mshds_extractor.py and the cepstral part (mshds_cpp.hip) start from.
// Semantics = oracle/mshds_oracle.py.  The workspace and "value at time" of the pitch track: mshds_voice_layout.h.
//
// Mapping: one workgroup per clip for the voiced stretches, one wave per voiced stretch for the pulse walker and one wave
// per clip to merge them.
#include "mshds_common.h"
#include "mshds_voice_layout.h"

namespace rsaf {
namespace mshds {

// Sound_findMaximumCorrelation with the shifts spread over the lanes; returns corr, *tout, *peak (uniform).
// The samples come from a wave-private LDS window that SLIDES with the walk: the fixed window and the union of the
// shifted windows of one pulse span ~2.5 periods, the window holds PULSE_LDS samples, so it is refilled from global
// memory once per ~10-20 pulses (in the walking direction) instead of twice per pulse; every lane then reads the fixed
// window as a broadcast and its own shifted window with unit stride.  `win0` = sample index of the window's first
// entry (INT64_MIN: empty), kept by the caller across pulses; dir = -1 / +1: the walk goes left / right.
constexpr int PULSE_LDS = 3072;
constexpr int PULSE_FW = 128;         // pitch frames of the walker's sliding window
__device__ double max_correlation_wave(const float* __restrict__ x, int n, double x1, double t1, double window, double tmin2,
                                       double tmax2, int lane, double* tout, double* peak, float* pwin, int64_t* win0, int dir) {
    const double half = 0.5 * window;
    const int64_t ileft1 = nearest_index(t1 - half, x1);
    const int64_t iright1 = nearest_index(t1 + half, x1);
    const int64_t l2min = low_index(tmin2 - half, x1);
    const int64_t l2max = high_index(tmax2 - half, x1);
    double best = -1.0, r2 = 0.0, r3 = 0.0, r1b = 0.0, r3b = 0.0, ir = 0.0, pk = 0.0;
    const int wlen = (int)(iright1 - ileft1 + 1);
    const int slen = (int)(l2max - l2min) + wlen;
    const int64_t ulo = ileft1 < l2min ? ileft1 : l2min;                      // union of both ranges
    const int64_t uhi = (ileft1 + wlen > l2min + slen ? ileft1 + wlen : l2min + slen);
    const bool staged = wlen > 0 && slen > 0 && uhi - ulo <= PULSE_LDS;
    if (staged && (*win0 == INT64_MIN || ulo < *win0 || uhi > *win0 + PULSE_LDS)) {
        // refill: the needed span at the trailing end of the window, the rest ahead in the walking direction
        const int64_t w0 = dir < 0 ? uhi - PULSE_LDS : ulo;
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < PULSE_LDS; i += 64) { const int64_t j = w0 + i; pwin[i] = (j >= 0 && j < n) ? x[j] : 0.0f; }
        *win0 = w0;
        wave_lds_sync();
    }
    const float* ps1 = pwin + (staged ? (int)(ileft1 - *win0) : 0);
    const float* ps2 = pwin + (staged ? (int)(l2min - *win0) : 0);
    // Interior case (every sample of both windows lies inside the sound: all pulses but the ones at the very ends of a
    // clip): no pair is skipped, so the sum of squares of the fixed window is one number, the one of the shifted window
    // slides (norm2(s + 1) = norm2(s) - a[s]^2 + a[s + wlen]^2: one scan over the 64 shifts of a batch), and the local
    // peak is only needed for the one step that detects the maximum.  The loop over the window then carries the cross
    // product alone: 2 LDS reads, 2 conversions and 1 FMA per sample instead of 3 FMAs, a maximum and an absolute value more.
    const bool interior = staged && ulo >= 0 && uhi <= n;
    double n1_all = 0.0;
    if (interior) {
        for (int i = lane; i < wlen; i += 64) { const double a = ps1[i]; n1_all = fma(a, a, n1_all); }
        n1_all = group_sum<64>(n1_all);
    }
    for (int64_t b = l2min; b <= l2max; b += 64) {
        const int64_t ileft2 = b + lane;
        double norm1 = 0.0, norm2 = 0.0, prod = 0.0, lp = 0.0;
        if (interior) {
            const int ob = (int)(b - l2min);                       // window offset of the batch's first shift
            double n20 = 0.0;                                      // sum of squares of shift ob
            for (int i = lane; i < wlen; i += 64) { const double a = ps2[ob + i]; n20 = fma(a, a, n20); }
            n20 = group_sum<64>(n20);
            const bool in = ileft2 <= l2max;
            const int o2 = ob + lane;
            // d_t = a[t + wlen]^2 - a[t]^2 for shift t -> t + 1 (reads stay inside the union: the last lane that matters is cnt - 1)
            double dsc = 0.0;
            if (in && ileft2 < l2max) { const double lo_ = ps2[o2], hi_ = ps2[o2 + wlen]; dsc = hi_ * hi_ - lo_ * lo_; }
            double incl = dsc;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const double up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
            norm1 = n1_all;
            norm2 = n20 + (incl - dsc);                            // exclusive prefix of the differences
            // The sliding sum is exact for 16-bit PCM (the squares add exactly); on resampled or float clips it can cancel
            // when the energy drops sharply inside the batch.  A lane whose sum has lost its digits takes the direct sum.
            if (in && !(norm2 > 1e-9 * n20)) {
                double d2 = 0.0;
                for (int i = 0; i < wlen; ++i) { const double a = ps2[o2 + i]; d2 = fma(a, a, d2); }
                norm2 = d2;
            }
            if (in) {
                double p0 = 0.0, p1 = 0.0;
                int i = 0;
                for (; i + 1 < wlen; i += 2) {
                    p0 = fma((double)ps1[i], (double)ps2[o2 + i], p0);
                    p1 = fma((double)ps1[i + 1], (double)ps2[o2 + i + 1], p1);
                }
                if (i < wlen) p0 = fma((double)ps1[i], (double)ps2[o2 + i], p0);
                prod = p0 + p1;
            }
        } else if (ileft2 <= l2max) {
            if (staged) {
                const int o2 = (int)(ileft2 - l2min);
                // Praat skips pairs outside the sound: the pairs inside are one index range, worked out once per lag
                int64_t lo = -ileft1 > -ileft2 ? -ileft1 : -ileft2, hi = n - ileft1 < n - ileft2 ? n - ileft1 : n - ileft2;
                lo = lo < 0 ? 0 : lo;
                hi = hi > wlen ? wlen : hi;
                for (int i = (int)lo; i < (int)hi; ++i) {
                    const double a1 = ps1[i], a2 = ps2[o2 + i];
                    norm1 += a1 * a1; norm2 += a2 * a2; prod += a1 * a2;
                    lp = fmax(lp, fabs(a2));
                }
            } else {
                for (int64_t i1 = ileft1, i2 = ileft2; i1 <= iright1; ++i1, ++i2) {
                    if (i1 < 0 || i1 >= n || i2 < 0 || i2 >= n) continue;
                    const double a1 = x[i1], a2 = x[i2];
                    norm1 += a1 * a1; norm2 += a2 * a2; prod += a1 * a2;
                    lp = fmax(lp, fabs(a2));
                }
            }
        }
        const double rr = prod != 0.0 ? prod / sqrt(norm1 * norm2) : 0.0;
        const int cnt = (int)((l2max - b + 1) < 64 ? (l2max - b + 1) : 64);
        // Praat's scan (r1 = r2; r2 = r3; r3 = r[k]; a strictly better r2 that is >= both neighbours wins, the local peak
        // taken at the step that detects it) for the 64 shifts at once: lane k holds step k's (r1, r2, r3) = (r[k-2], r[k-1],
        // r[k]) (r2, r3 carry the two last values across batches, zeros in front of the first shift), the winner is the FIRST
        // lane whose r2 equals the maximum over the qualifying lanes, taken only if it beats the best so far
        const double up1 = __shfl_up(rr, 1, 64), up2 = __shfl_up(rr, 2, 64);
        const double s2 = lane == 0 ? r3 : up1;
        const double s1 = lane == 0 ? r2 : (lane == 1 ? r3 : up2);
        const bool ok = lane < cnt && s2 >= s1 && s2 >= rr;
        const double m = wave_max_dpp(ok ? s2 : -INFINITY);
        if (m > best) {
            const int kw = __ffsll((long long)__ballot(ok && s2 == m)) - 1;
            best = m;
            r1b = readlane_f64(s1, kw); r3b = readlane_f64(rr, kw);
            if (interior) {                                        // local peak of the detecting step's shifted window
                const int ok_ = (int)(b - l2min) + kw;
                double mx = 0.0;
                for (int i = lane; i < wlen; i += 64) mx = fmax(mx, fabs((double)ps2[ok_ + i]));
                pk = wave_max_dpp(mx);
            } else {
                pk = readlane_f64(lp, kw);
            }
            ir = (double)(b + kw - 1);
        }
        const double last = readlane_f64(rr, cnt - 1);
        r2 = cnt >= 2 ? readlane_f64(rr, cnt - 2) : r3;
        r3 = last;
    }
    *peak = pk;
    *tout = t1;
    if (best > -1.0) {
        const double d2r = 2.0 * best - r1b - r3b;
        if (d2r != 0.0) { const double dr = 0.5 * (r3b - r1b); best += 0.5 * dr * dr / d2r; ir += dr / d2r; }
        *tout = t1 + (ir - (double)ileft1) * DXS;
    }
    return best;
}

__device__ double find_extremum_wave(const float* __restrict__ x, int n, double x1, double tmin, double tmax, int lane) {
    int64_t imin = low_index(tmin, x1), imax = high_index(tmax, x1);
    imin = imin < 0 ? 0 : imin;
    imax = imax > n - 1 ? n - 1 : imax;
    const int cnt = (int)(imax - imin + 1);
    if (cnt <= 0) return 0.5 * (tmin + tmax);
    double ie;
    if (cnt == 1) ie = 1.0;
    else if (cnt == 2) {
        const double a = fabs((double)x[imin]), b = fabs((double)x[imin + 1]);
        ie = a > b ? 1.0 : (a < b ? 2.0 : 1.5);
    } else {
        // first minimum / first maximum (strict comparisons in index order) via (value, index) reductions
        double mn = INFINITY, mx = -INFINITY;
        int jmn = 0x7fffffff, jmx = 0x7fffffff;
        for (int j = lane; j < cnt; j += 64) {
            const double v = x[imin + j];
            if (v < mn) { mn = v; jmn = j; }
            if (v > mx) { mx = v; jmx = j; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double omn = __shfl_xor(mn, o, 64), omx = __shfl_xor(mx, o, 64);
            const int ojmn = __shfl_xor(jmn, o, 64), ojmx = __shfl_xor(jmx, o, 64);
            if (omn < mn || (omn == mn && ojmn < jmn)) { mn = omn; jmn = ojmn; }
            if (omx > mx || (omx == mx && ojmx < jmx)) { mx = omx; jmx = ojmx; }
        }
        if (mn == mx) ie = 0.5 * (cnt + 1.0);
        else {
            const int j = fabs(mn) > fabs(mx) ? jmn : jmx;
            if (j == 0) ie = 1.0;
            else if (j == cnt - 1) ie = (double)cnt;
            else {
                const double vm = x[imin + j], vl = x[imin + j - 1], vr = x[imin + j + 1];
                ie = (j + 1) + 0.5 * (vr - vl) / (2.0 * vm - vl - vr);
            }
        }
    }
    return x1 + ((double)imin + ie - 1.0) * DXS;
}

// ---- Sound & Pitch: To PointProcess (cc) -------------------------------------------------------------------
// Praat walks the voiced stretches one after the other; inside a stretch the pulses are found one by one (each
// search starts at the previous pulse), but the stretches only interact through `added_right` (the last pulse
// added while walking right), which merely vetoes left-going pulses of later stretches.  So: (1) one wave per
// clip lists the stretches, (2) one wave per stretch walks it and records its pulses with their veto margins,
// (3) one wave per clip applies the vetoes in order and writes the pulses in ascending time.
__device__ __forceinline__ bool voiced_at(const double* f, int nF, double ceiling, int i) {
    return i >= 0 && i < nF && pitch_voiced(f[i], ceiling);
}

// 256 threads: all four waves scan the samples for the absolute peak (a single wave took 7 500 dependent-ish rounds over a
// 30 s clip: most of this kernel's 3.2 ms), wave 0 then lists the stretches.
__global__ __launch_bounds__(256) void pulse_stretches_kernel(const float* __restrict__ wav, const ClipInfo* __restrict__ pci,
                                                              const double* __restrict__ sel_freq, double pdt, double ceiling,
                                                              Stretch* __restrict__ st, int max_st, int* __restrict__ n_st,
                                                              double* __restrict__ abs_peak) {
    __shared__ float s_pk[4];
    const ClipInfo c = pci[blockIdx.x];
    const int lane = threadIdx.x & 63, nF = c.n_frames;
    {   // Vector_getAbsoluteExtremum of the whole sound (no mean subtraction, unlike the pitch analysis)
        const float* x = wav + c.sample_off;
        float gp = 0.0f;                                      // |x| of float samples: exact in float
        const int n4 = c.n_samples >> 2;
        const bool al = (reinterpret_cast<uintptr_t>(x) & 15) == 0;   // 16-byte loads when the clip's first sample is 16-byte aligned
                                                                      // (the address itself: `wav` may be any float*, e.g. a sliced view)
        if (al) {
            const float4* x4 = reinterpret_cast<const float4*>(x);
            for (int i = threadIdx.x; i < n4; i += 256) {
                const float4 v = x4[i];
                gp = fmaxf(fmaxf(gp, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
            }
            for (int i = 4 * n4 + threadIdx.x; i < c.n_samples; i += 256) gp = fmaxf(gp, fabsf(x[i]));
        } else {
            for (int i = threadIdx.x; i < c.n_samples; i += 256) gp = fmaxf(gp, fabsf(x[i]));
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) gp = fmaxf(gp, __shfl_xor(gp, o, 64));
        if (lane == 0) s_pk[threadIdx.x >> 6] = gp;
        __syncthreads();
        if (threadIdx.x == 0) abs_peak[blockIdx.x] = (double)fmaxf(fmaxf(s_pk[0], s_pk[1]), fmaxf(s_pk[2], s_pk[3]));
        if (threadIdx.x >= 64) return;
    }
    const double* f = sel_freq + c.frame_off;
    Stretch* S = st + (int64_t)blockIdx.x * max_st;
    int count = 0;
    for (int base = 0; base < nF; base += 64) {
        const int i = base + lane;
        const bool v = voiced_at(f, nF, ceiling, i);
        const bool start = v && !voiced_at(f, nF, ceiling, i - 1), end = v && !voiced_at(f, nF, ceiling, i + 1);
        const unsigned long long ms = __ballot(start);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (start) { const int k = count + __popcll(ms & below); if (k < max_st) S[k].il = i; }
        if (end) {
            // the stretch that ends here is the last one started at or before this frame
            const int k = count + __popcll(ms & (below | (1ull << lane))) - 1;
            if (k >= 0 && k < max_st) S[k].irr = i;
        }
        count += __popcll(ms);
    }
    count = count < max_st ? count : max_st;
    __threadfence_block();
    // scratch slots of every stretch, one after the other
    int run = 0;
    for (int base = 0; base < count; base += 64) {
        const int k = base + lane;
        int cap = 0;
        if (k < count) cap = stretch_cap(S[k].irr - S[k].il + 1, pdt, ceiling);
        int inc = cap;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t2 = __shfl_up(inc, o, 64); if (lane >= o) inc += t2; }
        if (k < count) { S[k].off = run + inc - cap; S[k].cap = cap; }
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0) n_st[blockIdx.x] = count;
}

// scratch per clip: left[slot] = (time, veto margin 0.8/f0) in walking order (entry 0 = the middle pulse),
// right[slot] = time; counts[stretch] = (n_left, n_right)
__global__ __launch_bounds__(256) void pulse_walk_kernel(const float* __restrict__ wav, const ClipInfo* __restrict__ pci,
                                                         const double* __restrict__ sel_freq, double pdt, double ceiling,
                                                         const double* __restrict__ abs_peak, const Stretch* __restrict__ st,
                                                         int max_st, const int* __restrict__ n_st, double2* __restrict__ left,
                                                         double* __restrict__ right, int cap_slots, int2* __restrict__ counts) {
    __shared__ float s_ps[4][PULSE_LDS];
    __shared__ double s_fw[4][PULSE_FW];                       // sliding window of the pitch track (the walk reads it once per pulse)
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int clip = blockIdx.y, k = blockIdx.x * 4 + wv;
    if (k >= n_st[clip]) return;
    float* pwin = s_ps[wv];
    int64_t win0 = INT64_MIN;
    const ClipInfo c = pci[clip];
    const float* x = wav + c.sample_off;
    const int n = c.n_samples, nF = c.n_frames;
    const double* f = sel_freq + c.frame_off;
    const Stretch S = st[(int64_t)clip * max_st + k];
    double2* L = left + (int64_t)clip * cap_slots + S.off;
    double* R = right + (int64_t)clip * cap_slots + S.off;
    const int cap = S.cap;
    double* fw = s_fw[wv];
    int fw0 = -(1 << 30);                                     // frame index of fw[0]; far away = empty
    // Pitch "Get value at time" on the LDS window.  The two frames around t (either may lie outside the track: read as 0) are
    // brought into the window once, ahead of the interpolation (a refill inside its `read` is inlined at both reads: 74 more
    // instructions); the needed frames at the trailing end, the rest ahead in the walking direction.
    auto f0_at = [&](double t, int dir) -> double {
        const int64_t lo = (int64_t)floor(frame_real_index(c.t1, pdt, t)), hi = lo + 1;
        if (hi >= 0 && lo < nF && (lo < fw0 || hi >= fw0 + PULSE_FW)) {
            const int64_t w0 = dir < 0 ? hi - (PULSE_FW - 1) : lo;
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < PULSE_FW; i += 64) { const int64_t j = w0 + i; fw[i] = (j >= 0 && j < nF) ? f[j] : 0.0; }
            fw0 = (int)w0;
            wave_lds_sync();
        }
        return value_at_time([&](int64_t i) { return fw[i - fw0]; }, [&](double v) { return pitch_voiced(v, ceiling); }, nF, c.t1,
                             pdt, t);
    };
    const double duration = c.xmax;                          // Pitch_getVoicedIntervalAfter works on the Pitch's domain = the sound's
    const double gp = abs_peak[clip];
    int nl = 0, nr = 0;
    double tleft = c.t1 + S.il * pdt - 0.5 * pdt, tright = c.t1 + S.irr * pdt + 0.5 * pdt;
    bool skip = tleft >= duration - 0.5 * pdt;               // Praat stops here; every later stretch starts even later
    tleft = tleft < 0.0 ? 0.0 : tleft;
    tright = tright > duration ? duration : tright;
    const double tmid = 0.5 * (tleft + tright);
    const double f0mid = pitch_value_at(f, nF, c.t1, pdt, ceiling, tmid);
    if (!(f0mid == f0mid)) skip = true;
    if (!skip) {
        double tmax = find_extremum_wave(x, n, c.x1, tmid - 0.5 / f0mid, tmid + 0.5 / f0mid, lane);
        if (lane == 0) L[0] = make_double2(tmax, 0.0);
        nl = 1;
        const double tsave = tmax;
        for (int g2 = 0; g2 < 200000; ++g2) {                      // to the left
            const double f0 = f0_at(tmax, -1);
            if (!(f0 == f0)) break;
            double peak, tout;
            const double corr = max_correlation_wave(x, n, c.x1, tmax, 1.0 / f0, tmax - 1.25 / f0, tmax - 0.8 / f0, lane, &tout, &peak, pwin, &win0, -1);
            tmax = tout;
            if (corr == -1.0) tmax -= 1.0 / f0;
            if (tmax < tleft) {
                if (corr > 0.7 && peak > 0.023333 * gp && nl < cap) { if (lane == 0) L[nl] = make_double2(tmax, 0.8 / f0); ++nl; }
                break;
            }
            if (corr > 0.3 && (peak == 0.0 || peak > 0.01 * gp) && nl < cap) { if (lane == 0) L[nl] = make_double2(tmax, 0.8 / f0); ++nl; }
        }
        tmax = tsave;
        for (int g2 = 0; g2 < 200000; ++g2) {                      // to the right
            const double f0 = f0_at(tmax, +1);
            if (!(f0 == f0)) break;
            double peak, tout;
            const double corr = max_correlation_wave(x, n, c.x1, tmax, 1.0 / f0, tmax + 0.8 / f0, tmax + 1.25 / f0, lane, &tout, &peak, pwin, &win0, +1);
            tmax = tout;
            if (corr == -1.0) tmax += 1.0 / f0;
            if (tmax > tright) {
                if (corr > 0.7 && peak > 0.023333 * gp && nr < cap) { if (lane == 0) R[nr] = tmax; ++nr; }
                break;
            }
            if (corr > 0.3 && (peak == 0.0 || peak > 0.01 * gp) && nr < cap) { if (lane == 0) R[nr] = tmax; ++nr; }
        }
    }
    if (lane == 0) counts[(int64_t)clip * max_st + k] = make_int2(nl, nr);
}

__global__ __launch_bounds__(64) void pulse_merge_kernel(const Stretch* __restrict__ st, int max_st, const int* __restrict__ n_st,
                                                         const double2* __restrict__ left, const double* __restrict__ right,
                                                         int cap_slots, const int2* __restrict__ counts,
                                                         double* __restrict__ pulses, int max_pulses, int* __restrict__ n_pulses) {
    const int clip = blockIdx.x, lane = threadIdx.x;
    const int ns = n_st[clip];
    double* pts = pulses + (int64_t)clip * max_pulses;
    int np_ = 0;
    double added_right = -1e308;
    for (int k = 0; k < ns; ++k) {
        const Stretch S = st[(int64_t)clip * max_st + k];
        const int2 cn = counts[(int64_t)clip * max_st + k];
        const double2* L = left + (int64_t)clip * cap_slots + S.off;
        const double* R = right + (int64_t)clip * cap_slots + S.off;
        if (cn.x <= 0) continue;
        // left-going pulses in ascending time = walking order reversed; entry 0 (the middle pulse) is never vetoed
        for (int base = cn.x - 1; base >= 1; base -= 64) {
            const int i = base - lane;
            bool keep = false;
            double t = 0.0;
            if (i >= 1) { const double2 e = L[i]; t = e.x; keep = t - added_right > e.y; }
            const unsigned long long m = __ballot(keep);
            const int pos = np_ + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && pos < max_pulses) pts[pos] = t;
            np_ += __popcll(m);
        }
        if (np_ < max_pulses && lane == 0) pts[np_] = L[0].x;
        ++np_;
        for (int base = 0; base < cn.y; base += 64) {
            const int i = base + lane;
            if (i < cn.y && np_ + i < max_pulses) pts[np_ + i] = R[i];
        }
        if (cn.y > 0) added_right = R[cn.y - 1];
        np_ += cn.y;
    }
    if (lane == 0) n_pulses[clip] = np_ < max_pulses ? np_ : max_pulses;
}

}  // namespace mshds
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::mshds;

static_assert(sizeof(double2) == PulseWorkspace::LEFT_BYTES && sizeof(int2) == PulseWorkspace::COUNT_BYTES, "PulseWorkspace rows");

extern "C" {

int64_t rsaf_mshds_pulses_workspace_bytes(int n_clips, int max_frames, double pitch_dt, double pitch_ceiling) {
    return PulseWorkspace(n_clips, max_frames, pitch_dt, pitch_ceiling).bytes;
}

int rsaf_mshds_pulses(const float* wav, const void* pitch_clip_info, int n_clips, int max_frames, const double* sel_freq,
                      double pitch_dt, double pitch_ceiling, void* workspace, int64_t workspace_bytes, double* pulses,
                      int max_pulses, int* n_pulses, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0 && n_clips <= 65535 && max_pulses >= 1 && max_frames >= 0, "bad argument");
    if (n_clips == 0) return RSAF_OK;
    RSAF_CHECK_ARG(wav && pitch_clip_info && sel_freq && workspace && pulses && n_pulses, "NULL pointer");
    const PulseWorkspace ws(n_clips, max_frames, pitch_dt, pitch_ceiling);
    RSAF_CHECK_ARG(workspace_bytes >= ws.bytes, "workspace too small (rsaf_mshds_pulses_workspace_bytes)");
    char* w = (char*)workspace;
    double2* left = (double2*)(w + ws.left);
    double* right = (double*)(w + ws.right);
    double* abs_peak = (double*)(w + ws.abs_peak);
    Stretch* st = (Stretch*)(w + ws.st);
    int2* counts = (int2*)(w + ws.counts);
    int* n_st = (int*)(w + ws.n_st);
    const int max_st = ws.max_st, cap_slots = ws.cap_slots;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("mshds_pulses", s, 0.0, 0.0);
    hipLaunchKernelGGL(pulse_stretches_kernel, dim3(n_clips), dim3(256), 0, s, wav, (const ClipInfo*)pitch_clip_info, sel_freq,
                       pitch_dt, pitch_ceiling, st, max_st, n_st, abs_peak);
    RSAF_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(pulse_walk_kernel, dim3((max_st + 3) / 4, n_clips), dim3(256), 0, s, wav, (const ClipInfo*)pitch_clip_info,
                       sel_freq, pitch_dt, pitch_ceiling, abs_peak, st, max_st, n_st, left, right, cap_slots, counts);
    RSAF_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(pulse_merge_kernel, dim3(n_clips), dim3(64), 0, s, st, max_st, n_st, left, right, cap_slots, counts, pulses,
                       max_pulses, n_pulses);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

}  // extern "C"
