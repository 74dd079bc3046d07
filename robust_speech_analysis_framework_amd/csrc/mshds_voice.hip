// The MSHDS analyses that work from the pitch track and the glottal pulses, float64 kernels for gfx950.
//
// Serves _extract_Slope_Tilt (:227-251) and _measureFormants (:303-338) of src/mshds_extractor.py, and the
// "To PointProcess (cc)" pulses that both, and the cepstral part (mshds_cpp.hip), start from: the 16 -> 10 kHz
// resampler at the head of To Formant (burg), Burg formants, the cc pulse walker, the pitch-corrected Ltas.
// Semantics = oracle/mshds_oracle.py.
//
// Mapping: a 320-thread workgroup per 5 x 256 resampler outputs (wave = phase of the 8 : 5 grid, a lane owns 4
// consecutive groups of five; the outputs whose depth the sound's ends clip are redone by a thread each),
// one wave per formant frame (4 waves x 6 frames per workgroup), one workgroup per clip for the voiced stretches,
// one wave per voiced stretch for the pulse walker and one wave per clip to merge them, 256 threads per clip for
// the Ltas, one wave per clip for the formant statistics.
#include <algorithm>

#include "mshds_common.h"

namespace rsaf {
namespace mshds {

// ---- 16 kHz -> 10 kHz resampling (Sound_resample (10000, 500) at the head of To Formant (burg)) -----------------
// Input: the clip after Praat's FFT low-pass (rsaf_praat_lowpass_batch).  out[m] = sum_k x[base + k] * W[phase][k + D]:
// the ratio 5/8 gives 5 distinct fractional offsets, whose NUM_interpolate_sinc weights at full depth D the host
// tabulates in float64.
struct ResampleInfo {        // per clip (host-built), 48 bytes
    int64_t sample_off;      // into wav
    int64_t out_off;         // into the 10 kHz buffer
    double pos0;             // real input index of output sample 0
    double x1o;              // time of output sample 0
    int n_in, n_out;
    int table;               // index of this clip's weight table (one per distinct pos0)
    int pad;
};

// 320-thread workgroup = 5 phases x 256 consecutive q: wave r owns phase r, so its weight row is wave-uniform and comes
// through the scalar cache into SGPRs (no LDS traffic for the weights); a lane owns 4 consecutive q, whose tap windows
// are 8 samples apart: every sample it reads from the LDS tile feeds 4 FMAs (taps k, k - 8, k - 16, k - 24 of its four
// outputs), which balances the LDS read rate against the fp64 FMA rate.  Lanes are 32 samples apart in the tile; a
// 33/32 skew puts the 8-byte reads of a half wave on distinct banks.  The tables hold NUM_interpolate_sinc's weights at
// full depth for the five fractional positions of the 8 : 5 grid, rows zero-padded to `wstride` doubles; outputs whose
// depth Praat clips (within `depth` input samples of either end) are recomputed by resample_edge_kernel.
constexpr int RS_QL = 4;                  // consecutive q per lane
constexpr int RS_QT = 64 * RS_QL;         // q per workgroup
__global__ __launch_bounds__(320) void resample_kernel(const double* __restrict__ lp, const ResampleInfo* __restrict__ ri,
                                                       const double* __restrict__ tables, int wstride,
                                                       const int* __restrict__ phase_base, int depth,
                                                       double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const ResampleInfo c = ri[blockIdx.y];
    const int q0 = blockIdx.x * RS_QT;
    if (5 * q0 >= c.n_out) return;
    const int taps = 2 * depth + 1;
    double* xs = reinterpret_cast<double*>(smem_raw);                 // input tile
    const int tid = threadIdx.x;
    const int* pb = phase_base + c.table * 5;
    int bmin = pb[0], bmax = pb[0];
    for (int r = 1; r < 5; ++r) { bmin = min(bmin, pb[r]); bmax = max(bmax, pb[r]); }
    const int lo = 8 * q0 + bmin - depth;                             // first input index of the tile
    const int nkb = (taps + 8 * (RS_QL - 1) + 7) / 8;                 // tap blocks of 8; the rows are zero beyond `taps`
    const int span = 8 * RS_QL * 63 + (bmax - bmin) + 8 * nkb;        // every index the tap loop reads
    const double* x = lp + c.sample_off;
    for (int i = tid; i < span; i += 320) {
        const int j = lo + i;
        xs[i + (i >> 5)] = (j >= 0 && j < c.n_in) ? x[j] : 0.0;
    }
    __syncthreads();
    const int r = __builtin_amdgcn_readfirstlane(tid >> 6), ql = tid & 63;
    const double* __restrict__ w = tables + ((int64_t)c.table * 5 + r) * wstride;   // wave-uniform
    const int i0 = 8 * RS_QL * ql + pb[r] - bmin;                     // tile index of tap 0 of the lane's first output
    double acc[RS_QL] = {0.0, 0.0, 0.0, 0.0};
    double wq[RS_QL][8];                                              // weights k = 8 (kb - j) + t of output j
#pragma unroll
    for (int j = 0; j < RS_QL; ++j)
#pragma unroll
        for (int t = 0; t < 8; ++t) wq[j][t] = 0.0;
    for (int kb = 0; kb < nkb; ++kb) {
#pragma unroll
        for (int j = RS_QL - 1; j > 0; --j)
#pragma unroll
            for (int t = 0; t < 8; ++t) wq[j][t] = wq[j - 1][t];
#pragma unroll
        for (int t = 0; t < 8; ++t) wq[0][t] = w[8 * kb + t];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int i = i0 + 8 * kb + t;
            const double xv = xs[i + (i >> 5)];
#pragma unroll
            for (int j = 0; j < RS_QL; ++j) acc[j] = fma(xv, wq[j][t], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < RS_QL; ++j) {
        const int m = 5 * (q0 + RS_QL * ql + j) + r;
        if (m < c.n_out) out[c.out_off + m] = acc[j];
    }
}

// the first and last `n_edge` output samples of every clip by the general routine when their depth is clipped (or the
// position falls outside the sound)
__global__ __launch_bounds__(256) void resample_edge_kernel(const double* __restrict__ lp, const ResampleInfo* __restrict__ ri,
                                                            int depth, int n_edge, double ratio_in_out, double* __restrict__ out) {
    const ResampleInfo c = ri[blockIdx.y];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * n_edge) return;
    const int m = e < n_edge ? e : c.n_out - 1 - (e - n_edge);
    if (m < 0 || m >= c.n_out) return;
    const double x = c.pos0 + (double)m * ratio_in_out + 1.0;         // Praat's 1-based real index
    const int64_t midleft = (int64_t)floor(x);
    const bool full = x >= 1.0 && x <= (double)c.n_in && midleft >= depth && (int64_t)c.n_in - midleft >= depth;
    if (full) return;
    out[c.out_off + m] = praat_interpolate_sinc(lp + c.sample_off, (int64_t)c.n_in, x, depth);
}

// ---- Formant (burg): one wave per frame -----------------------------------------------------------------------
// (wave sums / maxima on DPP + v_readlane, root broadcasts on v_readlane: the ds_bpermute forms - ~50 LDS-crossbar round
// trips per Aberth iteration, 24 per Burg order - were most of the 34 000 cycles a frame took)
// Gaussian-windowed 50 ms frame of the pre-emphasised 10 kHz signal -> Burg LPC (order 10) -> roots by
// Aberth-Ehrlich iteration (all ten simultaneously, lanes 0..9) + Newton polish -> reflect into the unit
// circle -> (frequency, bandwidth) of the roots in the upper half plane, ascending, at most 5.
constexpr int FB_ORDER = 10;
struct FormantFrame { double f[5]; double b[5]; };

// A wave takes FB_GROUP consecutive frames: the Burg recursion runs frame by frame with all 64 lanes on the frame's
// samples; the root finding - ten lanes per polynomial - then runs for the FB_GROUP polynomials at once (lane = 10 g + root),
// so that the most expensive phase (~650 instructions per Aberth iteration, 10-15 iterations) is paid once per 6 frames
// instead of once per frame with 54 idle lanes.
constexpr int FB_GROUP = 6;
__global__ __launch_bounds__(256) void formant_kernel(const double* __restrict__ y10, const ResampleInfo* __restrict__ ri,
                                                      const ClipInfo* __restrict__ ci, const double* __restrict__ win,
                                                      int nsw, double dt, double dxo, double preemph,
                                                      FormantFrame* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ double s_cf[4][FB_GROUP][FB_ORDER + 1];
    __shared__ double2 s_z[4][64];
    __shared__ double s_fq[4][64];
    __shared__ int s_okf[4][FB_GROUP];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const ClipInfo c = ci[blockIdx.y];
    const int fbase = (blockIdx.x * 4 + wv) * FB_GROUP;
    if (fbase >= c.n_frames) return;
    const ResampleInfo r = ri[blockIdx.y];
    double* b1 = reinterpret_cast<double*>(smem_raw) + (size_t)wv * 2 * (nsw + 2);
    double* b2 = b1 + (nsw + 2);
    const double* y = y10 + r.out_off;
    const int n = r.n_out;
    const double x1o = r.x1o;
    const double qn = __longlong_as_double(0x7ff8000000000000LL);
    auto wsync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    const int ng = min(FB_GROUP, c.n_frames - fbase);
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
        const int f = fbase + g;
        const double t = c.t1 + f * dt;
        const int left = (int)floor((t - x1o) / dxo);
        const int half = nsw / 2;
        int start = left + 1 - half, end = left + half;
        start = start < 0 ? 0 : start;
        end = end > n - 1 ? n - 1 : end;
        const int len = end - start + 1;
        // pre-emphasised, windowed frame into b1[1..len] (Burg's 1-based arrays); also the max intensity
        double mxi = 0.0, p = 0.0;
        for (int j0 = lane; j0 < len; j0 += 4 * 64) {                     // twelve loads in flight (see clip_peak_kernel)
            double ya[4], yb[4], wq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + 64 * u < len ? j0 + 64 * u : len - 1, i = start + j;
                ya[u] = y[i];
                yb[u] = y[i > 0 ? i - 1 : 0];
                wq[u] = win[j];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + 64 * u, i = start + j;
                if (j < len) {
                    const double v = (i > 0) ? ya[u] - preemph * yb[u] : ya[u];
                    mxi = fmax(mxi, v * v);
                    const double xv = v * wq[u];
                    b1[j + 1] = xv;
                    p += xv * xv;
                }
            }
        }
        mxi = wave_max_dpp(mxi);
        p = group_sum<64>(p);
        bool ok = !(len < FB_ORDER + 2 || mxi == 0.0 || p <= 0.0);
        wsync();
        double a[FB_ORDER + 1], aa[FB_ORDER + 1];
#pragma unroll
        for (int i = 0; i <= FB_ORDER; ++i) { a[i] = 0.0; aa[i] = 0.0; }
        if (ok) {
            // NUMburg.  x = b1 copy: b2[j] = x[j+1] for j = 1..len-1, b1[j] = x[j] for j = 1..len-1
            for (int j = 1 + lane; j <= len - 1; j += 64) b2[j] = b1[j + 1];
            wsync();
            for (int i = 1; i <= FB_ORDER; ++i) {
                double num = 0.0, den = 0.0;
                for (int j = 1 + lane; j <= len - i; j += 64) { const double u = b1[j], v = b2[j]; num += u * v; den += u * u + v * v; }
                num = group_sum<64>(num);
                den = group_sum<64>(den);
                if (den <= 0.0) { ok = false; break; }
                a[i] = 2.0 * num / den;
                for (int j = 1; j < i; ++j) a[j] = aa[j] - a[i] * aa[i - j];
                if (i < FB_ORDER) {
                    for (int j = 1; j <= i; ++j) aa[j] = a[j];
                    const double k = aa[i];
                    // b1[j] -= k*b2[j]; b2[j] = b2[j+1] - k*b1[j+1] (old b1) for j = 1..len-i-1
                    for (int j0 = 1; j0 <= len - i - 1; j0 += 64) {
                        const int j = j0 + lane;
                        double nb1 = 0.0, nb2 = 0.0;
                        const bool on = j <= len - i - 1;
                        if (on) { nb1 = b1[j] - k * b2[j]; nb2 = b2[j + 1] - k * b1[j + 1]; }
                        __builtin_amdgcn_wave_barrier();
                        if (on) { b1[j] = nb1; b2[j] = nb2; }
                        wsync();
                    }
                }
            }
        }
        // polynomial z^10 - a1 z^9 - ... - a10 ; cf[k] = coefficient of z^(10-k)
        if (lane == 0) {
            s_okf[wv][g] = ok ? 1 : 0;
            s_cf[wv][g][0] = 1.0;
#pragma unroll
            for (int k = 1; k <= FB_ORDER; ++k) s_cf[wv][g][k] = -a[k];
        }
        wsync();
    }
    // ---- roots of the ng polynomials at once: lane = 10 g + root ----
    const int g = lane / FB_ORDER, li = lane - g * FB_ORDER;
    const bool mine = g < ng;
    const int gg = mine ? g : 0;
    const bool okf = mine && s_okf[wv][gg] != 0;
    double cf[FB_ORDER + 1];
#pragma unroll
    for (int k = 0; k <= FB_ORDER; ++k) cf[k] = s_cf[wv][gg][k];
    // Aberth-Ehrlich: start on a circle of radius 0.9
    double zr = 0.0, zi = 0.0;
    { double sn, cs; sincos(2.0 * PI * (li + 0.35) / FB_ORDER, &sn, &cs); zr = 0.9 * cs; zi = 0.9 * sn; }
    for (int it = 0; it < 80; ++it) {
        // p(z), p'(z) by Horner
        double pr = cf[0], pi_ = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
        for (int k = 1; k <= FB_ORDER; ++k) {
            const double ndr = dr * zr - di * zi + pr, ndi = dr * zi + di * zr + pi_;
            dr = ndr; di = ndi;
            const double npr = pr * zr - pi_ * zi + cf[k], npi = pr * zi + pi_ * zr;
            pr = npr; pi_ = npi;
        }
        // w = p/p'
        const double dd = dr * dr + di * di;
        double wr_ = 0.0, wi_ = 0.0;
        if (dd > 0.0) { const double rd = fast_rcp(dd); wr_ = (pr * dr + pi_ * di) * rd; wi_ = (pi_ * dr - pr * di) * rd; }
        // s = sum_{j != i} 1/(z_i - z_j) over the roots of the same polynomial
        s_z[wv][lane] = make_double2(zr, zi);
        wsync();
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int j = 0; j < FB_ORDER; ++j) {
            const double2 oz = s_z[wv][gg * FB_ORDER + j];
            const double ex = zr - oz.x, ey = zi - oz.y;
            const double ee = ex * ex + ey * ey;
            if (j != li && ee > 0.0) { const double re = fast_rcp(ee); sr += ex * re; si -= ey * re; }
        }
        wsync();
        // delta = w / (1 - w*s)
        const double qr = 1.0 - (wr_ * sr - wi_ * si), qi = -(wr_ * si + wi_ * sr);
        const double qq = qr * qr + qi * qi;
        double er = wr_, ei = wi_;
        if (qq > 0.0) { const double rq = fast_rcp(qq); er = (wr_ * qr + wi_ * qi) * rq; ei = (wi_ * qr - wr_ * qi) * rq; }
        zr -= er; zi -= ei;
        const double step = okf ? fabs(er) + fabs(ei) : 0.0;
        if (wave_max_dpp(step) < 1e-11) break;               // the three Newton steps below square this down to rounding
    }
    for (int it = 0; it < 3; ++it) {                              // Newton polish on the original polynomial
        double pr = cf[0], pi_ = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
        for (int k = 1; k <= FB_ORDER; ++k) {
            const double ndr = dr * zr - di * zi + pr, ndi = dr * zi + di * zr + pi_;
            dr = ndr; di = ndi;
            const double npr = pr * zr - pi_ * zi + cf[k], npi = pr * zi + pi_ * zr;
            pr = npr; pi_ = npi;
        }
        const double dd = dr * dr + di * di;
        if (dd > 0.0) { zr -= (pr * dr + pi_ * di) / dd; zi -= (pi_ * dr - pr * di) / dd; }
    }
    // fix into the unit circle, keep the upper half plane, convert
    const double nyq = 0.5 / dxo;
    double mag2 = zr * zr + zi * zi;
    if (mag2 > 1.0) { zr /= mag2; zi /= mag2; mag2 = zr * zr + zi * zi; }   // z -> 1/conj(z)
    double fq = fabs(atan2(zi, zr)) * nyq / PI;
    const double bw = -log(mag2) * nyq / PI;
    const bool keep = okf && zi >= 0.0 && fq >= 50.0 && fq <= nyq - 50.0;
    if (!keep) fq = 1e300;
    // rank among the kept roots of the same frame (stable by root index), write the first five
    s_fq[wv][lane] = fq;
    wsync();
    int rank = 0;
#pragma unroll
    for (int j = 0; j < FB_ORDER; ++j) {
        const double of = s_fq[wv][gg * FB_ORDER + j];
        rank += (of < fq) || (of == fq && j < li);
    }
    // the five lowest of each frame through LDS, so that one lane writes each output slot
    s_z[wv][lane] = make_double2(qn, qn);
    wsync();
    if (keep && rank < 5) s_z[wv][gg * FB_ORDER + rank] = make_double2(fq, bw);
    wsync();
    if (mine && li < 5) {
        FormantFrame* o = out + c.frame_off + fbase + gg;
        const double2 v = s_z[wv][gg * FB_ORDER + li];
        o->f[li] = v.x;
        o->b[li] = v.y;
    }
}

// ---- glottal pulses: Sound & Pitch: To PointProcess (cc), one wave per clip ----------------------------------
__device__ double pitch_value_at(const double* __restrict__ f, int n, double t1, double dt, double ceiling, double t) {
    const double qn = __longlong_as_double(0x7ff8000000000000LL);
    if (n <= 0) return qn;
    const double ireal = (t - t1) / dt;
    const int64_t ileft = (int64_t)floor(ireal);
    double phase = ireal - (double)ileft;
    int64_t inear, ifar;
    if (phase < 0.5) { inear = ileft; ifar = ileft + 1; } else { inear = ileft + 1; ifar = ileft; phase = 1.0 - phase; }
    if (inear < 0 || inear >= n) return qn;
    const double fn = f[inear];
    if (!(fn > 0.0 && fn < ceiling)) return qn;
    if (ifar < 0 || ifar >= n) return fn;
    const double ff = f[ifar];
    if (!(ff > 0.0 && ff < ceiling)) return fn;
    return fn + phase * (ff - fn);
}

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
    double best = -1.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, r1b = 0.0, r3b = 0.0, ir = 0.0, pk = 0.0;
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
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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
    (void)r1;
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
struct Stretch { int il, irr, off, pad; };      // frame range, first slot of the stretch in the per-clip scratch

__device__ __forceinline__ bool voiced_at(const double* f, int nF, double ceiling, int i) {
    return i >= 0 && i < nF && f[i] > 0.0 && f[i] < ceiling;
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
    // scratch slots: a stretch of n frames holds at most n*pdt*ceiling/0.8 + 3 pulses on either side
    int run = 0;
    for (int base = 0; base < count; base += 64) {
        const int k = base + lane;
        int cap = 0;
        if (k < count) cap = (int)((double)(S[k].irr - S[k].il + 1) * pdt * ceiling * 1.25) + 4;
        int inc = cap;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t2 = __shfl_up(inc, o, 64); if (lane >= o) inc += t2; }
        if (k < count) { S[k].off = run + inc - cap; S[k].pad = cap; }
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
    const int cap = S.pad;
    double* fw = s_fw[wv];
    int fw0 = -(1 << 30);                                     // frame index of fw[0]; far away = empty
    // Pitch "Get value at time" (pitch_value_at) on the LDS window: the two frames around t, refilled when the walk leaves it
    auto f0_at = [&](double t, int dir) -> double {
        const double qn = __longlong_as_double(0x7ff8000000000000LL);
        if (nF <= 0) return qn;
        const double ireal = (t - c.t1) / pdt;
        const int64_t ileft = (int64_t)floor(ireal);
        double phase = ireal - (double)ileft;
        int64_t inear, ifar;
        if (phase < 0.5) { inear = ileft; ifar = ileft + 1; } else { inear = ileft + 1; ifar = ileft; phase = 1.0 - phase; }
        if (inear < 0 || inear >= nF) return qn;
        const int64_t lo = ileft, hi = ileft + 1;              // both frames (either may lie outside the track: read as 0)
        if (lo < fw0 || hi >= fw0 + PULSE_FW) {
            const int64_t w0 = dir < 0 ? hi - (PULSE_FW - 1) : lo;
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < PULSE_FW; i += 64) { const int64_t j = w0 + i; fw[i] = (j >= 0 && j < nF) ? f[j] : 0.0; }
            fw0 = (int)w0;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        const double fn = fw[inear - fw0];
        if (!(fn > 0.0 && fn < ceiling)) return qn;
        if (ifar < 0 || ifar >= nF) return fn;
        const double ff = fw[ifar - fw0];
        if (!(ff > 0.0 && ff < ceiling)) return fn;
        return fn + phase * (ff - fn);
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

// ---- Ltas (pitch-corrected) -> "Get slope" and robust tilt (src/mshds_extractor.py:227-251) ---------------
// One workgroup per clip; every wave takes every fourth pulse.  A pulse whose two neighbouring intervals are
// plausible periods contributes the energy spectrum of the one period around it: a DFT of exactly that many
// samples (lane = frequency bin, rotation recurrence over the samples), binned into 100 Hz bands.
// Per-wave band sums are combined in a fixed order, so the result does not depend on scheduling.
constexpr int LTAS_NB = 50;            // maximum frequency 5000 Hz / bandwidth 100 Hz
constexpr double LTAS_BW = 100.0;
constexpr int LTAS_MAXN = 1024;        // samples of one period that fit the LDS staging (longest period 20 ms = 320)

__device__ double ltas_mean_rect(const double* z, int nx, double x1, double dx, double xmin, double xmax) {
    const double qn = __longlong_as_double(0x7ff8000000000000LL);
    xmin = fmax(xmin, x1 - 0.5 * dx);
    xmax = fmin(xmax, x1 + (nx - 0.5) * dx);
    if (!(xmin < xmax)) return qn;
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
    return rng > 0.0 ? total / rng : qn;
}

__global__ __launch_bounds__(256) void ltas_kernel(const float* __restrict__ wav, const ClipInfo* __restrict__ ci,
                                                   const double* __restrict__ pulses, int max_pulses,
                                                   const int* __restrict__ n_pulses, double shortest, double longest,
                                                   double max_factor, double* __restrict__ out) {
    __shared__ double s_energy[4][LTAS_NB], s_count[4][LTAS_NB], s_z[LTAS_NB], s_slopes[LTAS_NB];
    __shared__ float s_x[4][LTAS_MAXN];
    __shared__ int s_periods[4], s_fail[4];
    const ClipInfo c = ci[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* x = wav + c.sample_off;
    const int n = c.n_samples;
    const double* pts = pulses + (int64_t)blockIdx.x * max_pulses;
    const int np_ = n_pulses[blockIdx.x];
    const double qn = __longlong_as_double(0x7ff8000000000000LL);
    for (int b = lane; b < LTAS_NB; b += 64) { s_energy[wv][b] = 0.0; s_count[wv][b] = 0.0; }
    int periods = 0, fail = 0;
    for (int ip = 1 + wv; ip < np_ - 1; ip += 4) {
        const double tl = pts[ip - 1], tm = pts[ip], tr = pts[ip + 1];
        const double left = tm - tl, right = tr - tm;
        const double factor = left > right ? left / right : right / left;
        if (!(left >= shortest && left <= longest && right >= shortest && right <= longest && factor <= max_factor)) continue;
        const double t1 = tm - 0.5 * left, t2 = tm + 0.5 * right;
        const int64_t ix1 = (int64_t)ceil((t1 - c.x1) / DXS), ix2 = (int64_t)floor((t2 - c.x1) / DXS);   // Sound_extractPart
        if (ix2 < ix1 || ix2 - ix1 + 1 > LTAS_MAXN) { fail = 1; continue; }   // Praat: "no samples" aborts the analysis
        const int m = (int)(ix2 - ix1 + 1);
        for (int j = lane; j < m; j += 64) { const int64_t i = ix1 + j; s_x[wv][j] = (i >= 0 && i < n) ? x[i] : 0.0f; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const double sdx = 1.0 / (DXS * m);
        const int nfreq = m / 2 + 1;
        // bins k = 1 .. nfreq-1 whose band ceil(k*sdx/100) is within 1..50 (k = 0 falls into band 0)
        for (int kb = 1; kb < nfreq; kb += 64) {
            const int k = kb + lane;
            const double freq = k * sdx;
            int band = (int)ceil(freq / LTAS_BW);
            const bool on = k < nfreq && band >= 1 && band <= LTAS_NB;
            double e = 0.0;
            if (__any(on)) {
                // sum_j x_j exp(-2 pi i k j / m): rotate (c, s) by the bin's angle, which lies in (0, pi]
                const double th = 2.0 * PI * (double)(k < nfreq ? k : 0) / (double)m;
                const double C = cos_0_pi(th), S = sin_0_pi(th);
                double cr = 1.0, sr = 0.0, re = 0.0, im = 0.0;
                for (int j = 0; j < m; ++j) {
                    const double v = s_x[wv][j];
                    re += v * cr; im -= v * sr;
                    const double c2 = cr * C - sr * S;
                    sr = sr * C + cr * S;
                    cr = c2;
                }
                re *= DXS; im *= DXS;
                e = (re * re + im * im) * 2.0 * sdx;
            }
            if (!on) { band = -1 - lane; e = 0.0; }
            // bands are non-decreasing in k: the first lane of a run adds the whole run (<= 4 bins per band)
            const int bprev = __shfl_up(band, 1, 64);
            const bool head = on && (lane == 0 || bprev != band);
            double sum = e, cnt = 1.0;
#pragma unroll
            for (int d = 1; d <= 7; ++d) {
                const int bn = __shfl_down(band, d, 64);
                const double en = __shfl_down(e, d, 64);
                if (lane + d < 64 && bn == band) { sum += en; cnt += 1.0; }
            }
            // a run can continue in the next 64-bin round: LDS accumulation below handles that (same wave, ordered)
            if (head) { s_energy[wv][band - 1] += sum; s_count[wv][band - 1] += cnt; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        ++periods;
    }
    if (lane == 0) { s_periods[wv] = periods; s_fail[wv] = fail; }
    __syncthreads();
    if (tid == 0) {
        const int total_periods = s_periods[0] + s_periods[1] + s_periods[2] + s_periods[3];
        const int failed = s_fail[0] | s_fail[1] | s_fail[2] | s_fail[3];
        double slope = qn, tilt = qn;
        if (np_ - 2 >= 1 && total_periods >= 1 && !failed) {
            double total = 0.0;
            for (int b = 0; b < LTAS_NB; ++b) {
                s_energy[0][b] = (s_energy[0][b] + s_energy[1][b]) + (s_energy[2][b] + s_energy[3][b]);
                s_count[0][b] = (s_count[0][b] + s_count[1][b]) + (s_count[2][b] + s_count[3][b]);
                total += s_count[0][b];
            }
            const double duration = c.xmax;                      // PointProcess_Sound_to_Ltas divides by sound->xmax - sound->xmin
            bool any = false;
            for (int b = 0; b < LTAS_NB; ++b) {
                if (s_count[0][b] > 0.0) {
                    const double mean_e = s_energy[0][b] / s_count[0][b];
                    s_z[b] = 10.0 * log10(mean_e * (total / LTAS_NB) / LTAS_BW / duration / 4.0e-10);
                    any = true;
                } else {
                    s_z[b] = qn;
                }
            }
            if (any) {
                for (int b = 0; b < LTAS_NB; ++b) s_slopes[b] = s_z[b];     // defined values before filling
                for (int b = 0; b < LTAS_NB; ++b) {
                    if (s_slopes[b] == s_slopes[b]) continue;
                    int bl = b - 1, br = b + 1;
                    while (bl >= 0 && !(s_slopes[bl] == s_slopes[bl])) --bl;
                    while (br < LTAS_NB && !(s_slopes[br] == s_slopes[br])) ++br;
                    if (bl < 0) s_z[b] = s_slopes[br];
                    else if (br >= LTAS_NB) s_z[b] = s_slopes[bl];
                    else s_z[b] = ((br - b) * s_slopes[bl] + (b - bl) * s_slopes[br]) / (double)(br - bl);
                }
                const double x1 = 0.5 * LTAS_BW;
                const double low = ltas_mean_rect(s_z, LTAS_NB, x1, LTAS_BW, 50.0, 1000.0);
                const double high = ltas_mean_rect(s_z, LTAS_NB, x1, LTAS_BW, 1000.0, 4000.0);
                slope = high - low;
                // Theil's incomplete method over the bands centred in [100, 5000] Hz
                int imin = 1 + (int)ceil((100.0 - x1) / LTAS_BW), imax = 1 + (int)floor((5000.0 - x1) / LTAS_BW);
                imin = imin < 1 ? 1 : imin;
                imax = imax > LTAS_NB ? LTAS_NB : imax;
                const int cntp = imax - imin + 1, nc = cntp / 2, n2 = (cntp & 1) ? nc + 1 : nc;
                for (int i = 0; i < nc; ++i) {
                    const double xa = x1 + (imin - 1 + i) * LTAS_BW, xb = x1 + (imin - 1 + n2 + i) * LTAS_BW;
                    s_slopes[i] = (s_z[imin - 1 + n2 + i] - s_z[imin - 1 + i]) / (xb - xa);
                }
                for (int i = 1; i < nc; ++i) {                              // insertion sort (<= 24 values)
                    const double v = s_slopes[i];
                    int j = i - 1;
                    while (j >= 0 && s_slopes[j] > v) { s_slopes[j + 1] = s_slopes[j]; --j; }
                    s_slopes[j + 1] = v;
                }
                if (nc >= 1) {                                              // NUMquantile(0.5)
                    if (nc == 1) tilt = s_slopes[0];
                    else {
                        const double place = 0.5 * nc + 0.5;
                        int lf = (int)floor(place);
                        lf = lf < 1 ? 1 : (lf > nc - 1 ? nc - 1 : lf);
                        tilt = s_slopes[lf] == s_slopes[lf - 1] ? s_slopes[lf - 1]
                                                                  : s_slopes[lf - 1] + (place - lf) * (s_slopes[lf] - s_slopes[lf - 1]);
                    }
                } else {
                    slope = qn;                                             // the tilt report fails -> both NaN (:250-251)
                }
            }
        }
        out[2 * blockIdx.x] = slope;
        out[2 * blockIdx.x + 1] = tilt;
    }
}

// ---- _measureFormants statistics: F1, B1, F2, B2 linearly interpolated at every pulse ------------------------
__global__ __launch_bounds__(64) void formant_stats_kernel(const FormantFrame* __restrict__ ff, const ClipInfo* __restrict__ fci,
                                                           double fdt, const double* __restrict__ pulses, int max_pulses,
                                                           const int* __restrict__ n_pulses, double* __restrict__ out) {
    const ClipInfo c = fci[blockIdx.x];
    const int lane = threadIdx.x, np_ = n_pulses[blockIdx.x], nF = c.n_frames;
    const FormantFrame* F = ff + c.frame_off;
    const double* pts = pulses + (int64_t)blockIdx.x * max_pulses;
    const double qn = __longlong_as_double(0x7ff8000000000000LL);
    double cnt[4] = {0, 0, 0, 0}, sum[4] = {0, 0, 0, 0};
    auto value = [&](int k, double t) -> double {      // k: 0 F1, 1 B1, 2 F2, 3 B2
        if (nF <= 0) return qn;
        const double ireal = (t - c.t1) / fdt;
        const int64_t ileft = (int64_t)floor(ireal);
        double phase = ireal - (double)ileft;
        int64_t inear, ifar;
        if (phase < 0.5) { inear = ileft; ifar = ileft + 1; } else { inear = ileft + 1; ifar = ileft; phase = 1.0 - phase; }
        if (inear < 0 || inear >= nF) return qn;
        const int fi = k >> 1;
        const double vn = (k & 1) ? F[inear].b[fi] : F[inear].f[fi];
        if (!(vn == vn)) return qn;
        if (ifar < 0 || ifar >= nF) return vn;
        const double vf = (k & 1) ? F[ifar].b[fi] : F[ifar].f[fi];
        if (!(vf == vf)) return vn;
        return vn + phase * (vf - vn);
    };
    for (int i = lane; i < np_; i += 64)
        for (int k = 0; k < 4; ++k) { const double v = value(k, pts[i]); if (v == v) { cnt[k] += 1; sum[k] += v; } }
    double mean[4];
    for (int k = 0; k < 4; ++k) { cnt[k] = wave_sum_f64(cnt[k]); sum[k] = wave_sum_f64(sum[k]); mean[k] = cnt[k] > 0 ? sum[k] / cnt[k] : qn; }
    double sq[4] = {0, 0, 0, 0};
    for (int i = lane; i < np_; i += 64)
        for (int k = 0; k < 4; ++k) { const double v = value(k, pts[i]); if (v == v) { const double d = v - mean[k]; sq[k] += d * d; } }
    for (int k = 0; k < 4; ++k) sq[k] = wave_sum_f64(sq[k]);
    if (lane == 0)
        for (int k = 0; k < 4; ++k) {
            out[blockIdx.x * 8 + 2 * k] = mean[k];
            out[blockIdx.x * 8 + 2 * k + 1] = cnt[k] > 1 ? sqrt(sq[k] / (cnt[k] - 1)) : qn;
        }
}

}  // namespace mshds
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::mshds;

extern "C" {

int rsaf_mshds_resample10k_table_stride(int depth) { return (2 * depth + 1 + 8 * (RS_QL - 1) + 7) / 8 * 8 + 8; }

int rsaf_mshds_resample10k(const double* lowpassed, const void* resample_info, int n_clips, int max_out, const double* tables,
                           int table_stride, const int* phase_base, int depth, double* out, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0 && n_clips <= 65535 && max_out >= 0 && depth >= 3, "bad argument");
    if (n_clips == 0 || max_out == 0) return RSAF_OK;
    RSAF_CHECK_ARG(lowpassed && resample_info && tables && phase_base && out, "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const int taps = 2 * depth + 1;
    RSAF_CHECK_ARG(table_stride >= rsaf_mshds_resample10k_table_stride(depth), "weight rows shorter than rsaf_mshds_resample10k_table_stride");
    const int span = 8 * (RS_QT - 1) + 8 + taps + 8 * RS_QL + 8;       // phase bases differ by < 8; the tap loop runs past `taps`
    const size_t lds = (size_t)(span + span / 32 + 2) * sizeof(double);
    RSAF_CHECK_ARG(lds <= 150 * 1024, "resampler depth too large for LDS");
    if (lds > 48 * 1024)
        RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ProfScope prof("mshds_resample10k", s, 0.0, 0.0);
    const int nq = (max_out + 4) / 5;
    hipLaunchKernelGGL(resample_kernel, dim3((nq + RS_QT - 1) / RS_QT, n_clips), dim3(320), lds, s, lowpassed,
                       (const ResampleInfo*)resample_info, tables, table_stride, phase_base, depth, out);
    RSAF_CHECK_HIP(hipGetLastError());
    const int n_edge = (int)((double)(depth + 2) * 0.625) + 3;         // output samples within depth + 2 input samples of an end
    hipLaunchKernelGGL(resample_edge_kernel, dim3((2 * n_edge + 255) / 256, n_clips), dim3(256), 0, s, lowpassed,
                       (const ResampleInfo*)resample_info, depth, n_edge, 1.6, out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_mshds_formants(const double* y10, const void* resample_info, const void* clip_info, int n_clips, int max_frames,
                        const double* window, int nsamp_window, double time_step, double dx_out, double preemph_factor,
                        void* frames_out, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0 && n_clips <= 65535 && max_frames >= 0 && nsamp_window >= 16, "bad argument");
    if (n_clips == 0 || max_frames == 0) return RSAF_OK;
    RSAF_CHECK_ARG(y10 && resample_info && clip_info && window && frames_out, "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)4 * 2 * (nsamp_window + 2) * sizeof(double);
    RSAF_CHECK_ARG(lds <= 150 * 1024, "formant window too long");
    if (lds > 48 * 1024)
        RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)formant_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ProfScope prof("mshds_formant_frames", s, 0.0, 0.0);
    hipLaunchKernelGGL(formant_kernel, dim3((max_frames + 4 * FB_GROUP - 1) / (4 * FB_GROUP), n_clips), dim3(256), lds, s, y10,
                       (const ResampleInfo*)resample_info, (const ClipInfo*)clip_info, window, nsamp_window, time_step,
                       dx_out, preemph_factor, (FormantFrame*)frames_out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// scratch of rsaf_mshds_pulses: stretch table + per-stretch counts + left (time, margin) + right (time) slots
static void pulses_layout(int n_clips, int max_frames, int max_samples, double pitch_dt, double ceiling, int* max_st,
                          int* cap_slots, int64_t* total) {
    *max_st = max_frames / 2 + 2;
    *cap_slots = (int)((double)max_frames * pitch_dt * ceiling * 1.25) + 4 * *max_st + 16;
    (void)max_samples;
    *total = (int64_t)n_clips * ((int64_t)*max_st * (sizeof(Stretch) + sizeof(int2)) + sizeof(int) * 2 + sizeof(double) +
                                 (int64_t)*cap_slots * (sizeof(double2) + sizeof(double))) + 256;
}

int64_t rsaf_mshds_pulses_workspace_bytes(int n_clips, int max_frames, double pitch_dt, double pitch_ceiling) {
    int ms, cs;
    int64_t total;
    pulses_layout(n_clips, max_frames, 0, pitch_dt, pitch_ceiling, &ms, &cs, &total);
    return total;
}

int rsaf_mshds_pulses(const float* wav, const void* pitch_clip_info, int n_clips, int max_frames, const double* sel_freq,
                      double pitch_dt, double pitch_ceiling, void* workspace, int64_t workspace_bytes, double* pulses,
                      int max_pulses, int* n_pulses, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0 && n_clips <= 65535 && max_pulses >= 1 && max_frames >= 0, "bad argument");
    if (n_clips == 0) return RSAF_OK;
    RSAF_CHECK_ARG(wav && pitch_clip_info && sel_freq && workspace && pulses && n_pulses, "NULL pointer");
    int max_st, cap_slots;
    int64_t need;
    pulses_layout(n_clips, max_frames, 0, pitch_dt, pitch_ceiling, &max_st, &cap_slots, &need);
    RSAF_CHECK_ARG(workspace_bytes >= need, "workspace too small (rsaf_mshds_pulses_workspace_bytes)");
    char* w = (char*)workspace;
    double2* left = (double2*)w;              w += (int64_t)n_clips * cap_slots * sizeof(double2);
    double* right = (double*)w;               w += (int64_t)n_clips * cap_slots * sizeof(double);
    double* abs_peak = (double*)w;            w += (int64_t)n_clips * sizeof(double);
    Stretch* st = (Stretch*)w;                w += (int64_t)n_clips * max_st * sizeof(Stretch);
    int2* counts = (int2*)w;                  w += (int64_t)n_clips * max_st * sizeof(int2);
    int* n_st = (int*)w;
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

int rsaf_mshds_ltas_slope_tilt(const float* wav, const void* clip_info, int n_clips, const double* pulses,
                               int max_pulses, const int* n_pulses, double shortest_period, double longest_period,
                               double max_period_factor, double* out, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0 && max_pulses >= 0, "bad clip/pulse count");
    if (n_clips == 0) return RSAF_OK;
    RSAF_CHECK_ARG(wav && clip_info && pulses && n_pulses && out, "NULL pointer");
    RSAF_CHECK_ARG(longest_period * 16000.0 + 2.0 <= LTAS_MAXN, "longest period does not fit the LDS staging");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("mshds_ltas", s, 0.0, 0.0);
    hipLaunchKernelGGL(ltas_kernel, dim3(n_clips), dim3(256), 0, s, wav, (const ClipInfo*)clip_info, pulses, max_pulses,
                       n_pulses, shortest_period, longest_period, max_period_factor, out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_mshds_formant_stats(const void* frames, const void* clip_info, int n_clips, double time_step, const double* pulses,
                             int max_pulses, const int* n_pulses, double* out, rsaf_stream_t stream) {
    if (n_clips <= 0) return RSAF_OK;
    RSAF_CHECK_ARG(frames && clip_info && pulses && n_pulses && out, "NULL pointer");
    hipLaunchKernelGGL(formant_stats_kernel, dim3(n_clips), dim3(64), 0, (hipStream_t)stream, (const FormantFrame*)frames,
                       (const ClipInfo*)clip_info, time_step, pulses, max_pulses, n_pulses, out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

}  // extern "C"
