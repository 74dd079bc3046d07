// Layouts and shared arithmetic of the MSHDS analyses that start from the pitch track and the glottal pulses
// (mshds_formant.hip, mshds_pulses.hip, mshds_ltas.hip), each stated once for the kernels, the host entries and the tests:
// the two structs the Python side mirrors (ResampleInfo, FormantFrame), the tile of the 16 -> 10 kHz resampler, the launch
// of the formant frames, the workspace of the pulse walker, "value at time t of a sampled track", and the scalar tail of
// the pitch-corrected Ltas ("Get slope", Theil tilt).
// Plain C++ (no HIP include): tests/test_voice_layout_host.py compiles it with g++ -ffp-contract=off and replays the tile,
// the workspace, the interpolation and the Ltas tail on the host (tests/host/voice_layout_replay.cpp).  Everything here is
// IEEE double arithmetic without contraction and without a library call, so a host compiler evaluates it to the bits the
// device does.
#pragma once
#include <math.h>

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VL_HD __host__ __device__ __forceinline__
#else
#define VL_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rsaf {
namespace mshds {

VL_HD double qnan() { return __builtin_nan(""); }         // "undefined" in every output of these analyses

// ---- structs the host builds or reads (mshds.RESAMPLE_INFO; the frames as rows of ten doubles) ----------------------------
struct ResampleInfo {        // per clip of the 16 -> 10 kHz resampling (host-built)
    int64_t sample_off;      // into wav
    int64_t out_off;         // into the 10 kHz buffer
    double pos0;             // real input index of output sample 0
    double x1o;              // time of output sample 0
    int n_in, n_out;
    int table;               // index of this clip's weight table (one per distinct pos0)
    int pad;
};
static_assert(sizeof(ResampleInfo) == 48 && offsetof(ResampleInfo, sample_off) == 0 && offsetof(ResampleInfo, out_off) == 8 &&
              offsetof(ResampleInfo, pos0) == 16 && offsetof(ResampleInfo, x1o) == 24 && offsetof(ResampleInfo, n_in) == 32 &&
              offsetof(ResampleInfo, n_out) == 36 && offsetof(ResampleInfo, table) == 40 && offsetof(ResampleInfo, pad) == 44,
              "ResampleInfo layout");

constexpr int FB_ORDER = 10;          // Burg order = 2 x 5 formants
struct FormantFrame { double f[5]; double b[5]; };        // ascending frequencies, their bandwidths; NaN = no such formant
static_assert(sizeof(FormantFrame) == 80 && offsetof(FormantFrame, f) == 0 && offsetof(FormantFrame, b) == 40, "FormantFrame layout");

// ---- the resampler's tile -------------------------------------------------------------------------------------------------------
// A workgroup of RS_THREADS = 5 phases x 64 lanes makes 5 x RS_QT outputs; a lane owns RS_QL consecutive groups of five, whose
// tap windows are 8 input samples apart.  The tap loop runs in blocks of 8 taps and past `taps` (the weight rows are zero
// there); the tile holds every input sample it reads, stored with a 33/32 skew.
constexpr int RS_QL = 4;                  // consecutive q per lane
constexpr int RS_QT = 64 * RS_QL;         // q per workgroup
constexpr int RS_THREADS = 320;
constexpr int RS_MAX_SPREAD = 7;          // the five phase bases of a table differ by less than 8
VL_HD constexpr int rs_taps(int depth) { return 2 * depth + 1; }
// tap blocks of 8 that cover the taps of a lane's RS_QL outputs
VL_HD constexpr int rs_tap_blocks(int depth) { return (rs_taps(depth) + 8 * (RS_QL - 1) + 7) / 8; }
// input samples a workgroup reads when its phase bases spread over bmax - bmin = spread
VL_HD constexpr int rs_span(int depth, int spread) { return 8 * RS_QL * 63 + spread + 8 * rs_tap_blocks(depth); }
VL_HD constexpr int rs_span_max(int depth) { return rs_span(depth, RS_MAX_SPREAD); }
// tile index of input sample i of the span: lanes are 32 samples apart, the skew puts a half wave's reads on distinct banks
VL_HD constexpr int rs_skew(int i) { return i + (i >> 5); }
// doubles the launch has always requested beyond the last one the kernel can touch (kept: the request decides how many
// workgroups share a CU); at depth 500 the request is 25 496 bytes
constexpr int RS_LDS_PAD = 37;
VL_HD constexpr size_t rs_lds_bytes(int depth) { return (size_t)(rs_skew(rs_span_max(depth) - 1) + 1 + RS_LDS_PAD) * sizeof(double); }
// doubles per weight row: the tap blocks, and one more block of zeros
VL_HD constexpr int rs_table_stride(int depth) { return 8 * rs_tap_blocks(depth) + 8; }
// output samples at either end of a clip that lie within depth + 2 input samples of it (redone by resample_edge_kernel)
VL_HD int rs_n_edge(int depth) { return (int)((double)(depth + 2) * 0.625) + 3; }

// ---- the formant launch --------------------------------------------------------------------------------------------------------
// One wave takes FB_GROUP consecutive frames, a workgroup FB_WAVES waves; per wave the dynamic LDS holds Burg's two 1-based
// arrays b1, b2 of nsw + 2 doubles each.
constexpr int FB_GROUP = 6;
constexpr int FB_WAVES = 4;
constexpr int FB_FRAMES_PER_WG = FB_WAVES * FB_GROUP;
VL_HD constexpr int fb_grid(int max_frames) { return (max_frames + FB_FRAMES_PER_WG - 1) / FB_FRAMES_PER_WG; }
VL_HD constexpr size_t fb_wave_doubles(int nsw) { return (size_t)2 * (nsw + 2); }
VL_HD constexpr size_t fb_lds_bytes(int nsw) { return (size_t)FB_WAVES * fb_wave_doubles(nsw) * sizeof(double); }
VL_HD double* fb_b1(void* lds, int wave, int nsw) { return reinterpret_cast<double*>(lds) + (size_t)wave * fb_wave_doubles(nsw); }
VL_HD double* fb_b2(void* lds, int wave, int nsw) { return fb_b1(lds, wave, nsw) + (nsw + 2); }

// ---- the pulse walker's workspace ------------------------------------------------------------------------------------------------
struct Stretch { int il, irr, off, cap; };      // voiced frames [il, irr]; first slot and slot count of the stretch in the clip's scratch
static_assert(sizeof(Stretch) == 16 && offsetof(Stretch, cap) == 12, "Stretch layout");

// slots of a stretch of `frames` frames: at most frames * pdt * ceiling / 0.8 + 3 pulses on either side
VL_HD int stretch_cap(int frames, double pdt, double ceiling) { return (int)((double)frames * pdt * ceiling * 1.25) + 4; }

// Per clip: max_st stretches (voiced runs need an unvoiced frame between them) and cap_slots slots.  The caps of a clip's
// stretches round down one by one and add 4 each, so together they stay below the cap of all frames as one stretch plus 4
// per stretch; 12 more have always been requested.  Arrays (byte offsets): left[slot] = (time, veto margin 0.8 / f0) in
// walking order (entry 0 = the middle pulse), right[slot] = time, abs_peak[clip], st[clip][stretch],
// counts[clip][stretch] = (n_left, n_right), n_st[clip].
struct PulseWorkspace {
    int max_st, cap_slots;
    int64_t left, right, abs_peak, st, counts, n_st, bytes;
    static constexpr int64_t LEFT_BYTES = 2 * sizeof(double), COUNT_BYTES = 2 * sizeof(int);
    VL_HD PulseWorkspace(int n_clips, int max_frames, double pitch_dt, double ceiling) {
        max_st = max_frames / 2 + 2;
        cap_slots = stretch_cap(max_frames, pitch_dt, ceiling) + 4 * max_st + 12;
        const int64_t n = n_clips;
        left = 0;
        right = left + n * cap_slots * LEFT_BYTES;
        abs_peak = right + n * cap_slots * (int64_t)sizeof(double);
        st = abs_peak + n * (int64_t)sizeof(double);
        counts = st + n * max_st * (int64_t)sizeof(Stretch);
        n_st = counts + n * max_st * COUNT_BYTES;
        bytes = n_st + n * (int64_t)sizeof(int) + n * (int64_t)sizeof(int) + 256;    // one more int per clip and 256 bytes: always requested
    }
};

// ---- value at time t of a track sampled at t1 + i dt, i = 0 .. n - 1 (Sampled_getValueAtX, linear) ---------------------------
// Linear between the two frames around t; where the farther one is undefined or outside the track, the nearer frame's value;
// where the nearer one is, undefined (NaN).  read(i) gives frame i, defined(v) says whether a frame's value counts.
// (frame_real_index: the real frame index of t; its floor and the frame after it are the two frames value_at_time may read)
VL_HD double frame_real_index(double t1, double dt, double t) { return (t - t1) / dt; }
template <class Read, class Defined>
VL_HD double value_at_time(Read read, Defined defined, int n, double t1, double dt, double t) {
    if (n <= 0) return qnan();
    const double ireal = frame_real_index(t1, dt, t);
    const int64_t ileft = (int64_t)floor(ireal);
    double phase = ireal - (double)ileft;
    int64_t inear, ifar;
    if (phase < 0.5) { inear = ileft; ifar = ileft + 1; } else { inear = ileft + 1; ifar = ileft; phase = 1.0 - phase; }
    if (inear < 0 || inear >= n) return qnan();
    const double vn = read(inear);
    if (!defined(vn)) return qnan();
    if (ifar < 0 || ifar >= n) return vn;
    const double vf = read(ifar);
    if (!defined(vf)) return vn;
    return vn + phase * (vf - vn);
}

// Pitch "Get value at time": a frame is voiced when 0 < f < ceiling
VL_HD bool pitch_voiced(double f, double ceiling) { return f > 0.0 && f < ceiling; }
VL_HD double pitch_value_at(const double* f, int n, double t1, double dt, double ceiling, double t) {
    return value_at_time([f](int64_t i) { return f[i]; }, [ceiling](double v) { return pitch_voiced(v, ceiling); }, n, t1, dt, t);
}

// ---- Ltas: "Get mean" without interpolation, "Get slope" and the robust tilt (src/mshds_extractor.py:227-251) ---------------
constexpr int LTAS_NB = 50;            // maximum frequency 5000 Hz / bandwidth 100 Hz
constexpr double LTAS_BW = 100.0;

// Sampled_getMean of nx bars of width dx, the first centred at x1, over [xmin, xmax]
VL_HD double ltas_mean_rect(const double* z, int nx, double x1, double dx, double xmin, double xmax) {
    xmin = fmax(xmin, x1 - 0.5 * dx);
    xmax = fmin(xmax, x1 + (nx - 0.5) * dx);
    if (!(xmin < xmax)) return qnan();
    const double rimin = (xmin - x1) / dx + 1.0, rimax = (xmax - x1) / dx + 1.0;
    double total = 0.0, rng = 0.0;
    if (rimax >= 0.5 && rimin < nx + 0.5) {
        const int imin = rimin < 0.5 ? 0 : (int)floor(rimin + 0.5);
        const int imax = rimax >= nx + 0.5 ? nx + 1 : (int)floor(rimax + 0.5);
        for (int i = imin + 1; i < imax; ++i) { rng += 1.0; total += z[i - 1]; }
        if (imin == imax) {
            if (imin >= 1 && imin <= nx) { const double ph = rimax - rimin; rng += ph; total += ph * z[imin - 1]; }
        } else {
            if (imin >= 1) { const double ph = imin - rimin + 0.5; rng += ph; total += ph * z[imin - 1]; }
            if (imax <= nx) { const double ph = rimax - imax + 0.5; rng += ph; total += ph * z[imax - 1]; }
        }
    }
    return rng > 0.0 ? total / rng : qnan();
}

// From the dB values of the LTAS_NB bands (NaN = band without a bin): undefined bands take the nearest defined value at the
// ends and the line between their defined neighbours inside; slope = mean over 1000-4000 Hz minus mean over 50-1000 Hz;
// tilt = median slope (NUMquantile 0.5) of Theil's incomplete method over the bands centred in [100, 5000] Hz.  Both NaN
// when no band is defined.  z is the work array: the fill and then the sorted slopes are written into it (slope i goes to
// z[i], below every band that a later slope reads).
VL_HD void ltas_slope_tilt(double* z, double* slope_out, double* tilt_out) {
    double slope = qnan(), tilt = qnan();
    int bl = -1;                                                    // last band defined before the fill
    bool any = false;
    for (int b = 0; b < LTAS_NB; ++b) {
        if (z[b] == z[b]) { bl = b; any = true; continue; }
        int br = b + 1;                                             // bands to the right are not filled yet
        while (br < LTAS_NB && !(z[br] == z[br])) ++br;
        if (bl < 0) { if (br < LTAS_NB) z[b] = z[br]; }
        else if (br >= LTAS_NB) z[b] = z[bl];
        else z[b] = ((br - b) * z[bl] + (b - bl) * z[br]) / (double)(br - bl);
    }
    if (any) {
        const double x1 = 0.5 * LTAS_BW;
        const double low = ltas_mean_rect(z, LTAS_NB, x1, LTAS_BW, 50.0, 1000.0);
        const double high = ltas_mean_rect(z, LTAS_NB, x1, LTAS_BW, 1000.0, 4000.0);
        slope = high - low;
        int imin = 1 + (int)ceil((100.0 - x1) / LTAS_BW), imax = 1 + (int)floor((5000.0 - x1) / LTAS_BW);
        imin = imin < 1 ? 1 : imin;
        imax = imax > LTAS_NB ? LTAS_NB : imax;
        const int cntp = imax - imin + 1, nc = cntp / 2, n2 = (cntp & 1) ? nc + 1 : nc;
        double* s = z;
        for (int i = 0; i < nc; ++i) {
            const double xa = x1 + (imin - 1 + i) * LTAS_BW, xb = x1 + (imin - 1 + n2 + i) * LTAS_BW;
            s[i] = (z[imin - 1 + n2 + i] - z[imin - 1 + i]) / (xb - xa);
        }
        for (int i = 1; i < nc; ++i) {                              // insertion sort (<= 24 values)
            const double v = s[i];
            int j = i - 1;
            while (j >= 0 && s[j] > v) { s[j + 1] = s[j]; --j; }
            s[j + 1] = v;
        }
        if (nc >= 1) {                                              // NUMquantile(0.5)
            if (nc == 1) tilt = s[0];
            else {
                const double place = 0.5 * nc + 0.5;
                int lf = (int)floor(place);
                lf = lf < 1 ? 1 : (lf > nc - 1 ? nc - 1 : lf);
                tilt = s[lf] == s[lf - 1] ? s[lf - 1] : s[lf - 1] + (place - lf) * (s[lf] - s[lf - 1]);
            }
        } else {
            slope = qnan();                                         // the tilt report fails -> both NaN (:250-251)
        }
    }
    *slope_out = slope;
    *tilt_out = tilt;
}

}  // namespace mshds
}  // namespace rsaf
