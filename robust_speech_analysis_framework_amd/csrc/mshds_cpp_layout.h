// Layouts and integer-deciding arithmetic of the cepstral-peak-prominence chain (mshds_cpp.hip), each stated once for the
// kernels, the host entry and the tests: the constants of the chain, the segment table row (Seg), the per-clip header
// (ClipHdr), the frame list that aliases the low-pass work buffer (FrameList), and the small functions that both forms of a
// per-frame kernel (one wave per frame / one workgroup per listed frame) must evaluate in the same operation order.
// Plain C++ (no HIP include): tests/test_cpp_layout_host.py compiles it with g++ -ffp-contract=off and replays round6,
// the interval geometry, find_seg, the frame list and the moving-average range on the host
// (tests/host/cpp_layout_replay.cpp).  Everything here is IEEE double arithmetic without contraction, so a host
// compiler evaluates it to the bits the device does (exp in gauss_window is the one library call: not compared).
#pragma once
#include <math.h>

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define CL_HD __host__ __device__ __forceinline__
#else
#define CL_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rsaf {
namespace mshds_cpp {

constexpr double DXS = 1.0 / 16000.0;     // sample period of the sounds (mshds::DXS)
constexpr double FS_OUT = 10000.0;
constexpr double DXO = 1.0 / FS_OUT;
constexpr int DEPTH = 50;                 // Sound_resample precision of Sound_to_PowerCepstrogram
constexpr double DT = 0.002;              // cepstrogram time step
constexpr double DQ = 1.0e-4;             // quefrency step = 1 / FS_OUT
constexpr int NFFT_MAX = 1024;            // 0.1 s window at 10 kHz = 1000 samples
constexpr int NQ_MAX = NFFT_MAX / 2 + 1;  // 513
constexpr int RS_TAPS = 2 * DEPTH;        // 100: weights of one phase of the polyphase resampler
constexpr int RS_WIN = 512;               // input window of a resampling workgroup: 255 * 1.6 + 100 samples
constexpr int CEP_FRAMES = 4;             // frames per wave of cepstrum_wave_kernel
constexpr int CPPF_FRAMES = 4;            // frames per wave of cpp_frame_wave_kernel
constexpr int ANTI_TURN_AROUND = 1000;    // zero padding on either side of Sound_resample's transform (resample::ANTI_TURN_AROUND)

// ---- the segment table: one voiced interval per row (all fields double so that the table is one plain array) -------------
struct Seg {
    double ix1, m_in, m_out, res_off, frame_off, nf, x1_seg, x1o, window, t1, nx, nfft;
    double work_off, item_off, lg;   // low-pass transform: first complex number, first work item, log2 of its length
};
constexpr int SEG_DOUBLES = 15;
static_assert(sizeof(Seg) == SEG_DOUBLES * sizeof(double), "Seg layout");
#define RSAF_SEG_AT(field, index) static_assert(offsetof(Seg, field) == (index) * sizeof(double), "Seg." #field)
RSAF_SEG_AT(ix1, 0); RSAF_SEG_AT(m_in, 1); RSAF_SEG_AT(m_out, 2); RSAF_SEG_AT(res_off, 3); RSAF_SEG_AT(frame_off, 4);
RSAF_SEG_AT(nf, 5); RSAF_SEG_AT(x1_seg, 6); RSAF_SEG_AT(x1o, 7); RSAF_SEG_AT(window, 8); RSAF_SEG_AT(t1, 9);
RSAF_SEG_AT(nx, 10); RSAF_SEG_AT(nfft, 11); RSAF_SEG_AT(work_off, 12); RSAF_SEG_AT(item_off, 13); RSAF_SEG_AT(lg, 14);
#undef RSAF_SEG_AT

// index of the segment that owns element g of a prefix-summed range; F = the range's offset field: res_off (resampled
// samples), frame_off (frames) or item_off (low-pass work items)
template <double Seg::*F>
CL_HD int find_seg(const Seg* s, int nseg, int g) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)(s[mid].*F) <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- the per-clip header the segment kernel leaves (int hdr[4 * n_clips] in the ABI) ----------------------------------------
struct ClipHdr {
    int n_seg, fail, total_frames, total_resampled;
    // (indexed as the int array: 4 * clip in 32 bits, the address arithmetic the kernels' instruction text was made with)
    static CL_HD ClipHdr* at(int* hdr, int clip) { return reinterpret_cast<ClipHdr*>(hdr + 4 * clip); }
    static CL_HD const ClipHdr* at(const int* hdr, int clip) { return reinterpret_cast<const ClipHdr*>(hdr + 4 * clip); }
};
static_assert(sizeof(ClipHdr) == 16 && offsetof(ClipHdr, n_seg) == 0 && offsetof(ClipHdr, fail) == 4 &&
              offsetof(ClipHdr, total_frames) == 8 && offsetof(ClipHdr, total_resampled) == 12, "ClipHdr layout");

// ---- the frame list ----------------------------------------------------------------------------------------------------------
// Frames a one-wave kernel leaves to its workgroup form, as (clip, frame) pairs.  The list lives in lp_work
// (n_clips * cap_work complex numbers), free once the intervals are resampled; the counter is the buffer's last 8-byte slot.
struct FrameList {
    int* entries;
    int* count;
    int cap;
    CL_HD FrameList(int* entries_, int* count_, int cap_) : entries(entries_), count(count_), cap(cap_) {}
    CL_HD FrameList(void* lp_work, int n_clips, int64_t cap_work) {
        const int64_t lp_doubles = (int64_t)n_clips * cap_work * 2;
        entries = reinterpret_cast<int*>(lp_work);
        count = entries + 2 * (lp_doubles - 1);
        cap = (int)(lp_doubles - 1 < 0x7fffffff ? lp_doubles - 1 : 0x7fffffff);
    }
    // every frame of every clip may be listed at most once per kernel: a list that holds them all drops nothing
    CL_HD bool holds(int64_t frames) const { return frames <= cap; }
#if defined(__HIPCC__)
    __device__ __forceinline__ void push(int clip, int frame) const {
        const int at = atomicAdd(count, 1);
        if (at < cap) { entries[2 * at] = clip; entries[2 * at + 1] = frame; }
    }
#endif
};

// ---- arithmetic that decides integers ------------------------------------------------------------------------------------------
// "%.6f" and back ("Down to Table" prints the interval times with 6 decimals, the reference parses them again).
// printf rounds the exact binary value; interval ends clipped to the sound's end are multiples of 62.5 us, i.e.
// sit within one ulp of a decimal tie, so the product t * 1e6 must not be rounded before the decision: the FMA
// recovers its rounding error exactly.
CL_HD double round6(double t) {
    const double p = t * 1.0e6;
    const double e = fma(t, 1.0e6, -p);                  // t * 1e6 == p + e exactly
    double q = floor(p);
    double f = (p - q) + e;                              // fractional part of the exact product
    if (f < 0.0) { q -= 1.0; f += 1.0; }
    const bool up = f > 0.5 || (f == 0.5 && fmod(q, 2.0) != 0.0);
    return (up ? q + 1.0 : q) / 1.0e6;
}

// One voiced interval [tmin, tmax], tmin < tmax (6-decimal times; the reference skips the others, :284), of a sound whose
// first sample lies at clip_x1: the extracted part, its 10 kHz grid, its cepstrogram frames and its low-pass transform.
// seg_geometry returns false where Praat raises outside the inner try (the clip's value is NaN): nothing of *out is valid then.
// (The kernel's instruction text depends on this shape: fields written through the pointer, the skip test at the call,
// exceeds() stated without a negation - profiles/r23/cpp_kernels_asm.txt.)
struct SegGeom {
    int64_t ix1, m_in, m_out, nf, nx;
    int nfft, lg;
    double dur, window, x1_seg, t1;
    // time of the first sample of the 10 kHz grid: m_out samples centred in the part's domain [0, dur]
    CL_HD double x1o() const { return 0.5 * (dur - (double)(m_out - 1) * DXO); }
    // complex numbers of the low-pass transform's work buffer
    CL_HD int64_t work_len() const { return (int64_t)1 << (lg - 1); }
    // what the per-frame kernels and the low-pass tables take
    CL_HD bool exceeds(int lg_max) const { return nx > NFFT_MAX || nx < 1 || nf < 1 || lg > lg_max; }
};
CL_HD bool seg_geometry(double tmin, double tmax, double clip_x1, double pitch_floor, SegGeom* out) {
    SegGeom& g = *out;
    g.ix1 = (int64_t)ceil((tmin - clip_x1) / DXS);
    const int64_t ix2 = (int64_t)floor((tmax - clip_x1) / DXS);
    g.dur = tmax - tmin;
    g.m_out = (int64_t)floor(g.dur * FS_OUT + 0.5);
    if (ix2 < g.ix1 || g.m_out < 1) return false;                        // Praat raises outside the inner try -> NaN
    g.m_in = ix2 - g.ix1 + 1;
    g.window = 2.0 * 3.0 / pitch_floor;
    const double my_duration = DXS * (double)g.m_in;
    if (g.window > my_duration) g.window = my_duration;
    g.nf = (int64_t)floor((my_duration - g.window) / DT) + 1;
    g.x1_seg = clip_x1 + (double)g.ix1 * DXS - tmin;
    const double mid = g.x1_seg - 0.5 * DXS + 0.5 * my_duration;
    g.t1 = mid - 0.5 * (double)g.nf * DT + 0.5 * DT;
    g.nx = (int64_t)floor(g.window * FS_OUT + 0.5);
    g.nfft = 2;
    while (g.nfft < g.nx) g.nfft *= 2;
    g.lg = 11;                                                           // Sound_resample: first power of two >= n + 2000
    while (((int64_t)1 << g.lg) < g.m_in + 2 * ANTI_TURN_AROUND) ++g.lg;
    return true;
}

// VECsmoothByMovingAverage with window w > 1 at element i of n: [i - w/2, i + w/2], one less on the right for even w, clipped
CL_HD void moving_average_range(int i, int w, int n, int* lo, int* hi) {
    const int a = i - w / 2, b = i + w / 2 - ((w & 1) == 0 ? 1 : 0);
    *lo = a < 0 ? 0 : a;
    *hi = b > n - 1 ? n - 1 : b;
}

// Gaussian window of nx samples at the 0-based sample i (Praat's: exp(-48 d^2 / (nx + 1)^2) brought to zero at the edges)
struct GaussWindow {
    double imid, edge;
    int nx;
    CL_HD explicit GaussWindow(int nx_) : imid(0.5 * (nx_ + 1)), edge(exp(-12.0)), nx(nx_) {}
    CL_HD double at(int i) const {
        const double d = (double)(i + 1) - imid;
        return (exp(-48.0 * (d * d) / (double)((nx + 1) * (nx + 1))) - edge) / (1.0 - edge);
    }
};
CL_HD double gauss_window(int i, int nx) { return GaussWindow(nx).at(i); }

// 0-based index on the interval's 10 kHz grid of the first sample of frame fl (Sampled_xToNearestIndex of the window's start)
template <class I>
CL_HD I frame_first_index(const Seg& s, int fl) {
    const double t = s.t1 + (double)fl * DT;
    return (I)floor((t - 0.5 * s.window - s.x1o) / DXO + 0.5);
}

// Theil's incomplete method over nq points: nc slopes between the points i and n2 + i
struct TheilN { int nc, n2; };
constexpr CL_HD TheilN theil_n(int nq) { return TheilN{nq / 2, (nq & 1) ? nq / 2 + 1 : nq / 2}; }

// median of a sorted even count plus one more value e, from the two middle values lo <= hi of the sorted part
CL_HD double median3_clamp(double e, double lo, double hi) { return e <= lo ? lo : (e >= hi ? hi : e); }

// quefrency bins of the peak search [qlo, qhi] among nq bins (0-based Sampled_getWindowSamples); empty when imax < imin
CL_HD void peak_bounds(double qlo, double qhi, int nq, int* imin, int* imax) {
    *imin = (int)ceil(qlo / DQ);
    const int b = (int)floor(qhi / DQ);
    *imax = b > nq - 1 ? nq - 1 : b;
}

// peak (value `best` at the real bin bx) minus the trend line at the peak's quefrency clamped to the search range; NaN
// when the range held no bin
CL_HD double cpp_value(double best, double bx, double slope, double icpt, double qlo, double qhi, bool any) {
    double out = __builtin_nan("");
    if (any) {
        double qpeak = bx * DQ;
        qpeak = qpeak < qlo ? qlo : (qpeak > qhi ? qhi : qpeak);
        out = best - (slope * qpeak + icpt);
    }
    return out;
}

}  // namespace mshds_cpp
}  // namespace rsaf
