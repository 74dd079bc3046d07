// MSHDS formants, float64 kernels for gfx950: the 16 -> 10 kHz resampler at the head of To Formant (burg), the Burg formant
// frames, and the statistics of F1, B1, F2, B2 at the glottal pulses.
//
// Serves _measureFormants (:303-338) of src/mshds_extractor.py.  Semantics = oracle/mshds_oracle.py.  Layouts, the
// resampler's tile and the launch geometry: mshds_voice_layout.h.
//
// Mapping: a 320-thread workgroup per 5 x 256 resampler outputs (wave = phase of the 8 : 5 grid, a lane owns 4
// consecutive groups of five; the outputs whose depth the sound's ends clip are redone by a thread each),
// one wave per formant frame (4 waves x 6 frames per workgroup), one wave per clip for the formant statistics.
#include "mshds_common.h"
#include "mshds_voice_layout.h"

namespace rsaf {
namespace mshds {

// ---- 16 kHz -> 10 kHz resampling (Sound_resample (10000, 500) at the head of To Formant (burg)) -----------------
// Input: the clip after Praat's FFT low-pass (rsaf_praat_lowpass_batch).  out[m] = sum_k x[base + k] * W[phase][k + D]:
// the ratio 5/8 gives 5 distinct fractional offsets, whose NUM_interpolate_sinc weights at full depth D the host
// tabulates in float64.
//
// 320-thread workgroup = 5 phases x 256 consecutive q: wave r owns phase r, so its weight row is wave-uniform and comes
// through the scalar cache into SGPRs (no LDS traffic for the weights); a lane owns 4 consecutive q, whose tap windows
// are 8 samples apart: every sample it reads from the LDS tile feeds 4 FMAs (taps k, k - 8, k - 16, k - 24 of its four
// outputs), which balances the LDS read rate against the fp64 FMA rate.  Lanes are 32 samples apart in the tile; a
// 33/32 skew puts the 8-byte reads of a half wave on distinct banks.  The tables hold NUM_interpolate_sinc's weights at
// full depth for the five fractional positions of the 8 : 5 grid, rows zero-padded to `wstride` doubles; outputs whose
// depth Praat clips (within `depth` input samples of either end) are recomputed by resample_edge_kernel.
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const double* __restrict__ lp, const ResampleInfo* __restrict__ ri,
                                                              const double* __restrict__ tables, int wstride,
                                                              const int* __restrict__ phase_base, int depth,
                                                              double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const ResampleInfo c = ri[blockIdx.y];
    const int q0 = blockIdx.x * RS_QT;
    if (5 * q0 >= c.n_out) return;
    double* xs = reinterpret_cast<double*>(smem_raw);                 // input tile
    const int tid = threadIdx.x;
    const int* pb = phase_base + c.table * 5;
    int bmin = pb[0], bmax = pb[0];
    for (int r = 1; r < 5; ++r) { bmin = min(bmin, pb[r]); bmax = max(bmax, pb[r]); }
    const int lo = 8 * q0 + bmin - depth;                             // first input index of the tile
    const int nkb = rs_tap_blocks(depth);                             // the rows are zero beyond the taps
    const int span = rs_span(depth, bmax - bmin);                     // every index the tap loop reads
    const double* x = lp + c.sample_off;
    for (int i = tid; i < span; i += RS_THREADS) {
        const int j = lo + i;
        xs[rs_skew(i)] = (j >= 0 && j < c.n_in) ? x[j] : 0.0;
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
            const double xv = xs[rs_skew(i)];
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
//
// A wave takes FB_GROUP consecutive frames: the Burg recursion runs frame by frame with all 64 lanes on the frame's
// samples; the root finding - ten lanes per polynomial - then runs for the FB_GROUP polynomials at once (lane = 10 g + root),
// so that the most expensive phase (~650 instructions per Aberth iteration, 10-15 iterations) is paid once per 6 frames
// instead of once per frame with 54 idle lanes.
struct FormantLds {                                    // static LDS of formant_kernel, a row per wave
    double cf[FB_WAVES][FB_GROUP][FB_ORDER + 1];       // polynomial of every frame of the group: cf[k] = coefficient of z^(10-k)
    double2 z[FB_WAVES][64];                           // root estimates (lane = 10 g + root); then the (frequency, bandwidth) slots
    double fq[FB_WAVES][64];                           // frequencies to rank
    int okf[FB_WAVES][FB_GROUP];                       // frame has a polynomial
};

// The frame around time t of the pre-emphasised, windowed signal into b1[1..len] (Burg's 1-based arrays); returns len, and
// the frame's maximum intensity and power.
__device__ __forceinline__ int formant_frame_to_lds(const double* __restrict__ y, int n, double x1o, double dxo, double t,
                                                    const double* __restrict__ win, int nsw, double preemph, int lane,
                                                    double* b1, double* max_intensity, double* power) {
    const int left = (int)floor((t - x1o) / dxo);
    const int half = nsw / 2;
    int start = left + 1 - half, end = left + half;
    start = start < 0 ? 0 : start;
    end = end > n - 1 ? n - 1 : end;
    const int len = end - start + 1;
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
    *max_intensity = wave_max_dpp(mxi);
    *power = group_sum<64>(p);
    return len;
}

// NUMburg of b1[1..len] (b2 = work array): a[1..FB_ORDER]; false when a denominator vanishes
__device__ __forceinline__ bool burg_recursion(double* b1, double* b2, int len, int lane, double (&a)[FB_ORDER + 1]) {
    double aa[FB_ORDER + 1];
#pragma unroll
    for (int i = 0; i <= FB_ORDER; ++i) aa[i] = 0.0;
    // x = b1 copy: b2[j] = x[j+1] for j = 1..len-1, b1[j] = x[j] for j = 1..len-1
    for (int j = 1 + lane; j <= len - 1; j += 64) b2[j] = b1[j + 1];
    wave_lds_sync();
    for (int i = 1; i <= FB_ORDER; ++i) {
        double num = 0.0, den = 0.0;
        for (int j = 1 + lane; j <= len - i; j += 64) { const double u = b1[j], v = b2[j]; num += u * v; den += u * u + v * v; }
        num = group_sum<64>(num);
        den = group_sum<64>(den);
        if (den <= 0.0) return false;
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
                wave_lds_sync();
            }
        }
    }
    return true;
}

// p(z) = (pr, pi) and p'(z) = (dr, di) of the monic polynomial cf at z = (zr, zi), by Horner
__device__ __forceinline__ void horner_p_dp(const double (&cf)[FB_ORDER + 1], double zr, double zi, double& pr, double& pi_,
                                            double& dr, double& di) {
    pr = cf[0]; pi_ = 0.0; dr = 0.0; di = 0.0;
#pragma unroll
    for (int k = 1; k <= FB_ORDER; ++k) {
        const double ndr = dr * zr - di * zi + pr, ndi = dr * zi + di * zr + pi_;
        dr = ndr; di = ndi;
        const double npr = pr * zr - pi_ * zi + cf[k], npi = pr * zi + pi_ * zr;
        pr = npr; pi_ = npi;
    }
}

// Aberth-Ehrlich on the polynomials of a wave at once (lane = 10 gg + li holds root li of polynomial gg; sz = the wave's root
// slots in LDS), from a circle of radius 0.9, until no root of a live polynomial (okf) moves by 1e-11
__device__ __forceinline__ void aberth_roots(const double (&cf)[FB_ORDER + 1], int gg, int li, int lane, bool okf, double2* sz,
                                             double& zr, double& zi) {
    { double sn, cs; sincos(2.0 * PI * (li + 0.35) / FB_ORDER, &sn, &cs); zr = 0.9 * cs; zi = 0.9 * sn; }
    for (int it = 0; it < 80; ++it) {
        double pr, pi_, dr, di;
        horner_p_dp(cf, zr, zi, pr, pi_, dr, di);
        // w = p/p'
        const double dd = dr * dr + di * di;
        double wr_ = 0.0, wi_ = 0.0;
        if (dd > 0.0) { const double rd = fast_rcp(dd); wr_ = (pr * dr + pi_ * di) * rd; wi_ = (pi_ * dr - pr * di) * rd; }
        // s = sum_{j != i} 1/(z_i - z_j) over the roots of the same polynomial
        sz[lane] = make_double2(zr, zi);
        wave_lds_sync();
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int j = 0; j < FB_ORDER; ++j) {
            const double2 oz = sz[gg * FB_ORDER + j];
            const double ex = zr - oz.x, ey = zi - oz.y;
            const double ee = ex * ex + ey * ey;
            if (j != li && ee > 0.0) { const double re = fast_rcp(ee); sr += ex * re; si -= ey * re; }
        }
        wave_lds_sync();
        // delta = w / (1 - w*s)
        const double qr = 1.0 - (wr_ * sr - wi_ * si), qi = -(wr_ * si + wi_ * sr);
        const double qq = qr * qr + qi * qi;
        double er = wr_, ei = wi_;
        if (qq > 0.0) { const double rq = fast_rcp(qq); er = (wr_ * qr + wi_ * qi) * rq; ei = (wi_ * qr - wr_ * qi) * rq; }
        zr -= er; zi -= ei;
        const double step = okf ? fabs(er) + fabs(ei) : 0.0;
        if (wave_max_dpp(step) < 1e-11) break;               // the three Newton steps of the polish square this down to rounding
    }
}

// The root (zr, zi) of a frame's polynomial -> reflected into the unit circle, kept if in the upper half plane and 50 Hz inside
// the band, converted to (frequency, bandwidth), ranked among the kept roots of its frame (stable by root index); the five
// lowest of each frame go through LDS, so that one lane writes each output slot (o = the frame's output; mine: lane has one).
__device__ __forceinline__ void roots_to_formants(double zr, double zi, double dxo, int gg, int li, int lane, bool okf, bool mine,
                                                  double2* sz, double* sfq, FormantFrame* o) {
    const double nyq = 0.5 / dxo;
    double mag2 = zr * zr + zi * zi;
    if (mag2 > 1.0) { zr /= mag2; zi /= mag2; mag2 = zr * zr + zi * zi; }   // z -> 1/conj(z)
    double fq = fabs(atan2(zi, zr)) * nyq / PI;
    const double bw = -log(mag2) * nyq / PI;
    const bool keep = okf && zi >= 0.0 && fq >= 50.0 && fq <= nyq - 50.0;
    if (!keep) fq = 1e300;
    sfq[lane] = fq;
    wave_lds_sync();
    int rank = 0;
#pragma unroll
    for (int j = 0; j < FB_ORDER; ++j) {
        const double of = sfq[gg * FB_ORDER + j];
        rank += (of < fq) || (of == fq && j < li);
    }
    sz[lane] = make_double2(qnan(), qnan());
    wave_lds_sync();
    if (keep && rank < 5) sz[gg * FB_ORDER + rank] = make_double2(fq, bw);
    wave_lds_sync();
    if (mine && li < 5) {
        const double2 v = sz[gg * FB_ORDER + li];
        o->f[li] = v.x;
        o->b[li] = v.y;
    }
}

__global__ __launch_bounds__(64 * FB_WAVES) void formant_kernel(const double* __restrict__ y10, const ResampleInfo* __restrict__ ri,
                                                                const ClipInfo* __restrict__ ci, const double* __restrict__ win,
                                                                int nsw, double dt, double dxo, double preemph,
                                                                FormantFrame* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ FormantLds s;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const ClipInfo c = ci[blockIdx.y];
    const int fbase = (blockIdx.x * FB_WAVES + wv) * FB_GROUP;
    if (fbase >= c.n_frames) return;
    const ResampleInfo r = ri[blockIdx.y];
    double* b1 = fb_b1(smem_raw, wv, nsw);
    double* b2 = fb_b2(smem_raw, wv, nsw);
    const int ng = min(FB_GROUP, c.n_frames - fbase);
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
        double mxi, p;
        const int len = formant_frame_to_lds(y10 + r.out_off, r.n_out, r.x1o, dxo, c.t1 + (fbase + g) * dt, win, nsw, preemph,
                                             lane, b1, &mxi, &p);
        bool ok = !(len < FB_ORDER + 2 || mxi == 0.0 || p <= 0.0);
        wave_lds_sync();
        double a[FB_ORDER + 1];
#pragma unroll
        for (int i = 0; i <= FB_ORDER; ++i) a[i] = 0.0;
        if (ok) ok = burg_recursion(b1, b2, len, lane, a);
        // polynomial z^10 - a1 z^9 - ... - a10
        if (lane == 0) {
            s.okf[wv][g] = ok ? 1 : 0;
            s.cf[wv][g][0] = 1.0;
#pragma unroll
            for (int k = 1; k <= FB_ORDER; ++k) s.cf[wv][g][k] = -a[k];
        }
        wave_lds_sync();
    }
    // ---- roots of the ng polynomials at once: lane = 10 g + root ----
    const int g = lane / FB_ORDER, li = lane - g * FB_ORDER;
    const bool mine = g < ng;
    const int gg = mine ? g : 0;
    const bool okf = mine && s.okf[wv][gg] != 0;
    double cf[FB_ORDER + 1];
#pragma unroll
    for (int k = 0; k <= FB_ORDER; ++k) cf[k] = s.cf[wv][gg][k];
    double zr, zi;
    aberth_roots(cf, gg, li, lane, okf, s.z[wv], zr, zi);
    for (int it = 0; it < 3; ++it) {                              // Newton polish on the original polynomial
        double pr, pi_, dr, di;
        horner_p_dp(cf, zr, zi, pr, pi_, dr, di);
        const double dd = dr * dr + di * di;
        if (dd > 0.0) { zr -= (pr * dr + pi_ * di) / dd; zi -= (pi_ * dr - pr * di) / dd; }
    }
    roots_to_formants(zr, zi, dxo, gg, li, lane, okf, mine, s.z[wv], s.fq[wv], out + c.frame_off + fbase + gg);
}

// ---- _measureFormants statistics: F1, B1, F2, B2 linearly interpolated at every pulse ------------------------
__global__ __launch_bounds__(64) void formant_stats_kernel(const FormantFrame* __restrict__ ff, const ClipInfo* __restrict__ fci,
                                                           double fdt, const double* __restrict__ pulses, int max_pulses,
                                                           const int* __restrict__ n_pulses, double* __restrict__ out) {
    const ClipInfo c = fci[blockIdx.x];
    const int lane = threadIdx.x, np_ = n_pulses[blockIdx.x], nF = c.n_frames;
    const FormantFrame* F = ff + c.frame_off;
    const double* pts = pulses + (int64_t)blockIdx.x * max_pulses;
    double cnt[4] = {0, 0, 0, 0}, sum[4] = {0, 0, 0, 0};
    auto value = [&](int k, double t) -> double {      // k: 0 F1, 1 B1, 2 F2, 3 B2
        const int fi = k >> 1;
        return value_at_time([&](int64_t i) { return (k & 1) ? F[i].b[fi] : F[i].f[fi]; }, [](double v) { return v == v; },
                             nF, c.t1, fdt, t);
    };
    for (int i = lane; i < np_; i += 64)
        for (int k = 0; k < 4; ++k) { const double v = value(k, pts[i]); if (v == v) { cnt[k] += 1; sum[k] += v; } }
    double mean[4];
    for (int k = 0; k < 4; ++k) { cnt[k] = wave_sum_f64(cnt[k]); sum[k] = wave_sum_f64(sum[k]); mean[k] = cnt[k] > 0 ? sum[k] / cnt[k] : qnan(); }
    double sq[4] = {0, 0, 0, 0};
    for (int i = lane; i < np_; i += 64)
        for (int k = 0; k < 4; ++k) { const double v = value(k, pts[i]); if (v == v) { const double d = v - mean[k]; sq[k] += d * d; } }
    for (int k = 0; k < 4; ++k) sq[k] = wave_sum_f64(sq[k]);
    if (lane == 0)
        for (int k = 0; k < 4; ++k) {
            out[blockIdx.x * 8 + 2 * k] = mean[k];
            out[blockIdx.x * 8 + 2 * k + 1] = cnt[k] > 1 ? sqrt(sq[k] / (cnt[k] - 1)) : qnan();
        }
}

}  // namespace mshds
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::mshds;

extern "C" {

int rsaf_mshds_resample10k_table_stride(int depth) { return rs_table_stride(depth); }

int rsaf_mshds_resample10k(const double* lowpassed, const void* resample_info, int n_clips, int max_out, const double* tables,
                           int table_stride, const int* phase_base, int depth, double* out, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0 && n_clips <= 65535 && max_out >= 0 && depth >= 3, "bad argument");
    if (n_clips == 0 || max_out == 0) return RSAF_OK;
    RSAF_CHECK_ARG(lowpassed && resample_info && tables && phase_base && out, "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    RSAF_CHECK_ARG(table_stride >= rs_table_stride(depth), "weight rows shorter than rsaf_mshds_resample10k_table_stride");
    const size_t lds = rs_lds_bytes(depth);
    RSAF_CHECK_ARG(lds <= 150 * 1024, "resampler depth too large for LDS");
    if (lds > 48 * 1024)
        RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ProfScope prof("mshds_resample10k", s, 0.0, 0.0);
    const int nq = (max_out + 4) / 5;
    hipLaunchKernelGGL(resample_kernel, dim3((nq + RS_QT - 1) / RS_QT, n_clips), dim3(RS_THREADS), lds, s, lowpassed,
                       (const ResampleInfo*)resample_info, tables, table_stride, phase_base, depth, out);
    RSAF_CHECK_HIP(hipGetLastError());
    const int n_edge = rs_n_edge(depth);
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
    const size_t lds = fb_lds_bytes(nsamp_window);
    RSAF_CHECK_ARG(lds <= 150 * 1024, "formant window too long");
    if (lds > 48 * 1024)
        RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)formant_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ProfScope prof("mshds_formant_frames", s, 0.0, 0.0);
    hipLaunchKernelGGL(formant_kernel, dim3(fb_grid(max_frames), n_clips), dim3(64 * FB_WAVES), lds, s, y10,
                       (const ResampleInfo*)resample_info, (const ClipInfo*)clip_info, window, nsamp_window, time_step,
                       dx_out, preemph_factor, (FormantFrame*)frames_out);
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
