// Praat-style contour analyses behind the MSHDS features, float64 kernels for gfx950.
//
// Replaces these parselmouth/Praat calls of src/mshds_extractor.py: _speechrate (:11-125), _extract_intensity (:185-205),
// the mean of _extract_harmonicity (:207-225) and _extract_Spectral_Moments (:340-376).  The pitch analysis they read
// lives in mshds_pitch.hip, formants, pulses and Ltas in mshds_formant.hip, mshds_pulses.hip and mshds_ltas.hip, the
// cepstral part in mshds_cpp.hip, what the files share in mshds_common.h.
// Algorithms: Praat's intensity (Kaiser-weighted mean square), Gaussian-window spectrogram + spectral moments gated by
// pitch definedness, the harmonics-to-noise mean over a cc pitch track, de Jong & Wempe syllable nuclei.  Semantics =
// oracle/mshds_oracle.py (parity unpinned: Praat itself is not available).  Praat computes in double, so do these
// kernels.
//
// Mapping: one workgroup per clip for the global peak, one wave per frame for intensity and the 1 024-point spectrogram
// slice (a workgroup per frame for other transform lengths), one wave per clip for the speech rate and the per-clip
// statistics.
#include <algorithm>

#include "mshds_common.h"      // FMA contraction is off from there on

namespace rsaf {
namespace mshds {

// ---- per-clip mean and global peak |x - mean| ------------------------------------------------------
__global__ __launch_bounds__(256) void clip_peak_kernel(const float* __restrict__ wav, const ClipInfo* __restrict__ ci,
                                                        double* __restrict__ gpeak) {
    __shared__ double red[4];
    __shared__ double bc;
    const ClipInfo c = ci[blockIdx.x];
    const float* x = wav + c.sample_off;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // (these loops keep eight loads in flight: an exec-masked loop with one load per turn is not unrolled by the compiler
    // and waits for the memory once per turn; the additions keep their order)
    double s = 0.0;
    const int last = c.n_samples - 1;
    for (int i0 = threadIdx.x; i0 < c.n_samples; i0 += 8 * 256) {
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = x[i0 + 256 * u <= last ? i0 + 256 * u : last];
#pragma unroll
        for (int u = 0; u < 8; ++u) if (i0 + 256 * u <= last) s += (double)q[u];
    }
    s = wave_sum_f64(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) bc = c.n_samples > 0 ? (red[0] + red[1] + red[2] + red[3]) / c.n_samples : 0.0;
    __syncthreads();
    const double mean = bc;
    double m = 0.0;
    for (int i0 = threadIdx.x; i0 < c.n_samples; i0 += 8 * 256) {
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = x[i0 + 256 * u <= last ? i0 + 256 * u : last];
#pragma unroll
        for (int u = 0; u < 8; ++u) if (i0 + 256 * u <= last) m = fmax(m, fabs((double)q[u] - mean));
    }
    m = wave_max_f64(m);
    __syncthreads();
    if (lane == 0) red[w] = m;
    __syncthreads();
    if (threadIdx.x == 0) gpeak[blockIdx.x] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// ---- intensity: one wave per frame -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void intensity_kernel(const float* __restrict__ wav, const ClipInfo* __restrict__ ci,
                                                        const double* __restrict__ win, int half, double dt,
                                                        int subtract_mean, double* __restrict__ out) {
    const ClipInfo c = ci[blockIdx.y];
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= c.n_frames) return;
    const int lane = threadIdx.x & 63;
    const float* x = wav + c.sample_off;
    const double t = c.t1 + f * dt;
    const int64_t mid = nearest_index(t, c.x1);
    const int64_t lo = mid - half < 0 ? 0 : mid - half;
    const int64_t hi = mid + half > c.n_samples - 1 ? c.n_samples - 1 : mid + half;
    double mean = 0.0;
    if (subtract_mean) {
        double s = 0.0;
        for (int64_t i0 = lo + lane; i0 <= hi; i0 += 8 * 64) {           // eight loads in flight (see clip_peak_kernel)
            float q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = x[i0 + 64 * u <= hi ? i0 + 64 * u : hi];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (i0 + 64 * u <= hi) s += (double)q[u];
        }
        mean = wave_sum_f64(s) / (double)(hi - lo + 1);
    }
    double sw = 0.0, sx = 0.0;
    for (int64_t i0 = lo + lane; i0 <= hi; i0 += 8 * 64) {
        float q[8];
        double wq[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t i = i0 + 64 * u <= hi ? i0 + 64 * u : hi;
            q[u] = x[i];
            wq[u] = win[i - mid + half];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (i0 + 64 * u <= hi) {
                const double d = (double)q[u] - mean;
                sw += wq[u];
                sx += d * d * wq[u];
            }
        }
    }
    sw = wave_sum_f64(sw);
    sx = wave_sum_f64(sx);
    if (lane == 0) {
        const double v = sx / sw / 4.0e-10;
        out[c.frame_off + f] = v < 1e-30 ? -300.0 : 10.0 * log10(v);
    }
}

// ---- intensity statistics: energy mean, parabolic max / min -----------------------------------------------
__global__ __launch_bounds__(64) void intensity_stats_kernel(const double* __restrict__ db, const ClipInfo* __restrict__ ci,
                                                             double* __restrict__ out) {
    const ClipInfo c = ci[blockIdx.x];
    const int lane = threadIdx.x, n = c.n_frames;
    const double* y = db + c.frame_off;
    const double qn = __longlong_as_double(0x7ff8000000000000LL);
    if (n <= 0) {
        if (lane == 0) { out[blockIdx.x * 2] = qn; out[blockIdx.x * 2 + 1] = qn; }
        return;
    }
    double se = 0.0, mx = -INFINITY, mn = -INFINITY;      // mn holds the maximum of -y
    for (int i = lane; i < n; i += 64) {
        const double v = y[i];
        se += pow(10.0, v / 10.0);
        if (i == 0 || i == n - 1) { mx = fmax(mx, v); mn = fmax(mn, -v); }
        if (i > 0 && i < n - 1) {
            const double a = y[i - 1], b = y[i + 1];
            if (v > a && v >= b) {
                const double dy = 0.5 * (b - a), d2 = 2.0 * v - a - b;
                mx = fmax(mx, d2 != 0.0 ? v + 0.5 * dy * dy / d2 : v);
            }
            if (-v > -a && -v >= -b) {
                const double dy = 0.5 * (a - b), d2 = -2.0 * v + a + b;
                mn = fmax(mn, d2 != 0.0 ? -v + 0.5 * dy * dy / d2 : -v);
            }
        }
    }
    se = wave_sum_f64(se); mx = wave_max_f64(mx); mn = wave_max_f64(mn);
    if (lane == 0) {
        const double mean_db = 10.0 * log10(se / n);
        const double minv = -mn;
        out[blockIdx.x * 2] = mean_db;
        out[blockIdx.x * 2 + 1] = minv != 0.0 ? mx / minv : qn;
    }
}

// ---- HNR mean: 10 log10(r / (1 - r)) over voiced frames of a cc pitch track -------------------------------
__global__ __launch_bounds__(64) void hnr_stats_kernel(const double* __restrict__ sel_freq, const double* __restrict__ sel_str,
                                                       const ClipInfo* __restrict__ ci, double* __restrict__ out) {
    const ClipInfo c = ci[blockIdx.x];
    const int lane = threadIdx.x;
    double n = 0, s = 0;
    for (int i = lane; i < c.n_frames; i += 64) {
        const double f = sel_freq[c.frame_off + i], r = sel_str[c.frame_off + i];
        if (f != 0.0) {
            n += 1;
            s += r <= 1e-15 ? -150.0 : (r > 1.0 - 1e-15 ? 150.0 : 10.0 * log10(r / (1.0 - r)));
        }
    }
    n = wave_sum_f64(n); s = wave_sum_f64(s);
    if (lane == 0) out[blockIdx.x] = n > 0 ? s / n : __longlong_as_double(0x7ff8000000000000LL);
}

// ---- Gaussian-window spectrogram slice + spectral moments, gated by pitch definedness ----------------------
// one workgroup per frame; fp64 radix-2 FFT (in LDS, half length: real input) of the zero-padded windowed frame, bins 0..nbins-1 (bin width 1/(dx*nfft))
__global__ __launch_bounds__(512) void spec_moments_kernel(const float* __restrict__ wav, const ClipInfo* __restrict__ ci,
                                                           const ClipInfo* __restrict__ pitch_ci, const double* __restrict__ sel_freq,
                                                           double pitch_dt, double ceiling, const double* __restrict__ win,
                                                           const double2* __restrict__ tw, int nsamp, int half, int nfft,
                                                           int nbins, double tstep, double fstep,
                                                           double* __restrict__ mom /* [frames][5]: ok, cog, sd, skew, kurt */) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double2* a = reinterpret_cast<double2*>(smem_raw);          // nfft complex values of the FFT
    double* pw = reinterpret_cast<double*>(a + nfft / 2);        // nbins (the FFT works on nfft / 2 complex values)
    __shared__ double s_red[8][4];
    const ClipInfo c = ci[blockIdx.y];
    const int f = blockIdx.x;
    if (f >= c.n_frames) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nwv = blockDim.x >> 6;
    double* o = mom + (c.frame_off + f) * 5;
    const double t = c.t1 + f * tstep;
    // gate: Pitch "Get value at time" defined iff the nearest pitch frame is voiced
    {
        const ClipInfo pc = pitch_ci[blockIdx.y];
        const double ireal = (t - pc.t1) / pitch_dt;
        const double il = floor(ireal);
        const int64_t near = (ireal - il < 0.5) ? (int64_t)il : (int64_t)il + 1;
        bool ok = near >= 0 && near < pc.n_frames;
        if (ok) {
            const double pf = sel_freq[pc.frame_off + near];
            ok = pf > 0.0 && pf < ceiling;
        }
        if (!ok) {
            if (tid == 0) o[0] = 0.0;
            return;
        }
    }
    const float* x = wav + c.sample_off;
    const int64_t start = low_index(t, c.x1) + 1 - half;
    // windowed frame, zero-padded to nfft.  Real input: one complex FFT of half the length over z[j] = x[2j] + i x[2j+1]
    // (stored bit-reversed for the in-place radix-2 passes), then X[k] = E + W^k O with E / O the even / odd parts.
    const int nthr = blockDim.x;
    int log2n = 0;
    while ((1 << log2n) < nfft) ++log2n;
    const int m = nfft >> 1, log2m = log2n - 1;
    for (int j = tid; j < m; j += nthr) {
        double v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int jj = 2 * j + e;
            v[e] = 0.0;
            if (jj < nsamp) {
                int64_t i = start + jj;
                i = i < 0 ? 0 : (i > c.n_samples - 1 ? c.n_samples - 1 : i);
                v[e] = (double)x[i] * win[jj];
            }
        }
        a[log2m ? (int)(__brev((unsigned)j) >> (32 - log2m)) : 0] = make_double2(v[0], v[1]);
    }
    __syncthreads();
    for (int st = 1; st <= log2m; ++st) {
        const int half_ = 1 << (st - 1), tstep_ = nfft >> st;
        for (int b = tid; b < (m >> 1); b += nthr) {
            const int grp = b >> (st - 1), p = b & (half_ - 1);
            const int i0 = (grp << st) + p, i1 = i0 + half_;
            const double2 w = tw[p * tstep_];
            const double2 u = a[i0], v = a[i1];
            const double tr = v.x * w.x - v.y * w.y, ti = v.x * w.y + v.y * w.x;
            a[i0] = make_double2(u.x + tr, u.y + ti);
            a[i1] = make_double2(u.x - tr, u.y - ti);
        }
        __syncthreads();
    }
    for (int k = tid; k < nbins; k += nthr) {              // nbins <= nfft / 2 + 1
        const double2 zk = a[k == m ? 0 : k], zc = a[k == 0 ? 0 : m - k];
        const double er = 0.5 * (zk.x + zc.x), ei = 0.5 * (zk.y - zc.y);
        const double orr = 0.5 * (zk.y + zc.y), oi = -0.5 * (zk.x - zc.x);
        const double2 w = k == m ? make_double2(-1.0, 0.0) : tw[k];
        const double re = er + w.x * orr - w.y * oi, im = ei + w.x * oi + w.y * orr;
        pw[k] = re * re + im * im;
    }
    __syncthreads();
    double s0 = 0, s1 = 0;
    for (int k = tid; k < nbins; k += nthr) { s0 += pw[k]; s1 += pw[k] * (k * fstep); }
    s0 = wave_sum_f64(s0); s1 = wave_sum_f64(s1);
    if (lane == 0) { s_red[wv][0] = s0; s_red[wv][1] = s1; }
    __syncthreads();
    double tot = 0.0, cog = 0.0;
    for (int q = 0; q < nwv; ++q) { tot += s_red[q][0]; cog += s_red[q][1]; }
    cog /= tot;
    __syncthreads();
    double m2 = 0, m3 = 0, m4 = 0;
    for (int k = tid; k < nbins; k += nthr) {
        const double d = k * fstep - cog, p = pw[k];
        const double d2 = d * d;
        m2 += p * d2; m3 += p * d2 * d; m4 += p * d2 * d2;
    }
    m2 = wave_sum_f64(m2); m3 = wave_sum_f64(m3); m4 = wave_sum_f64(m4);
    if (lane == 0) { s_red[wv][0] = m2; s_red[wv][1] = m3; s_red[wv][2] = m4; }
    __syncthreads();
    if (tid == 0) {
        double u2 = 0.0, u3 = 0.0, u4 = 0.0;
        for (int q = 0; q < nwv; ++q) { u2 += s_red[q][0]; u3 += s_red[q][1]; u4 += s_red[q][2]; }
        u2 /= tot; u3 /= tot; u4 /= tot;
        o[0] = 1.0;
        o[1] = cog;
        o[2] = sqrt(u2);
        o[3] = u3 / (u2 * sqrt(u2));
        o[4] = u4 / (u2 * u2) - 3.0;
    }
}

// mean of each moment over gated frames whose value is not NaN (reference :366-374)
// The same analysis, one wavefront per frame, for the usual transform length of 1 024 (25 ms Gaussian window at 16 kHz):
// the real transform is one 512-point complex transform in registers (wave_fft.h), the power of bins k and 512 - k comes
// from the conjugate pair the lane holding k < 256 evaluates, and the four moments are sums over the registers.
constexpr int SPM_FRAMES = 4;
__global__ __launch_bounds__(64, 4) void spec_moments_wave_kernel(const float* __restrict__ wav, const ClipInfo* __restrict__ ci,
                                                                  const ClipInfo* __restrict__ pitch_ci, const double* __restrict__ sel_freq,
                                                                  double pitch_dt, double ceiling, const double* __restrict__ win,
                                                                  const double2* __restrict__ tw, int nsamp, int half, int nbins,
                                                                  double tstep, double fstep, double* __restrict__ mom) {
    using namespace wfft;
    __shared__ double lds[Plan<8>::LDS_DOUBLES];
    constexpr int R = 8, S = 512, H = 4;
    const ClipInfo c = ci[blockIdx.y];
    const int f0 = blockIdx.x * SPM_FRAMES;
    if (f0 >= c.n_frames) return;
    const ClipInfo pc = pitch_ci[blockIdx.y];
    const int lane_ = threadIdx.x;
    const float* x = wav + c.sample_off;
    const int n = c.n_samples;
    LdsMem mem{lds};
    const int f1 = f0 + SPM_FRAMES < c.n_frames ? f0 + SPM_FRAMES : c.n_frames;
#pragma unroll 1
    for (int f = f0; f < f1; ++f) {
        int lane = lane_;
        asm volatile("" : "+v"(lane));
        double* o = mom + (c.frame_off + f) * 5;
        const double t = c.t1 + f * tstep;
        // gate: Pitch "Get value at time" defined iff the nearest pitch frame is voiced
        {
            const double ireal = (t - pc.t1) / pitch_dt;
            const double il = floor(ireal);
            const int64_t near = (ireal - il < 0.5) ? (int64_t)il : (int64_t)il + 1;
            bool ok = near >= 0 && near < pc.n_frames;
            if (ok) {
                const double pf = sel_freq[pc.frame_off + near];
                ok = pf > 0.0 && pf < ceiling;
            }
            if (!ok) {                                            // uniform
                if (lane == 0) o[0] = 0.0;
                continue;
            }
        }
        const int start = (int)(low_index(t, c.x1) + 1 - half);
        cplx v[R];
#pragma unroll
        for (int m = 0; m < R; ++m) {
            const int j = 2 * (lane + 64 * m);                    // samples 2 k, 2 k + 1 of the frame (loads on clamped indices)
            int i0 = start + j, i1 = i0 + 1;
            i0 = i0 < 0 ? 0 : (i0 > n - 1 ? n - 1 : i0);
            i1 = i1 < 0 ? 0 : (i1 > n - 1 ? n - 1 : i1);
            const int w0 = j < nsamp ? j : nsamp - 1, w1 = j + 1 < nsamp ? j + 1 : nsamp - 1;
            const double a0 = (double)x[i0] * win[w0], a1 = (double)x[i1] * win[w1];
            v[m] = cplx{j < nsamp ? a0 : 0.0, j + 1 < nsamp ? a1 : 0.0};
        }
        const double2_t wl2 = reinterpret_cast<const double2_t*>(tw)[lane];
        const cplx wl{wl2.x, wl2.y};
        {
            const double2_t a = reinterpret_cast<const double2_t*>(tw)[2 * lane], b = reinterpret_cast<const double2_t*>(tw)[(lane % 8) * 16];
            wave_fft<R>(v, lds, lane, cplx{a.x, a.y}, cplx{b.x, b.y});
        }
        ac_spec_store<R>(v, mem, lane);
        wave_sync();
        // power of bins k (pa) and 512 - k (pb) for the lane's k = lane + 64 m < 256; lane 0 also holds bin 256 (p256)
        double pa[H], pb[H];
#pragma unroll
        for (int m = 0; m < H; ++m) {
            const int k = lane + 64 * m;
            const int pp = k ? S / 2 - k : 0;
            cplx zc{mem.ld(pp), mem.ld(S / 2 + pp)};
            if (m == 0) zc = cplx{lane == 0 ? v[0].x : zc.x, lane == 0 ? v[0].y : zc.y};
            const cplx zk = v[m], w = mul_w64(wl, m * 4);                       // W_1024^(64 m) = W_64^(4 m)
            const double er = 0.5 * (zk.x + zc.x), ei = 0.5 * (zk.y - zc.y), orr = 0.5 * (zk.y + zc.y), oi = -0.5 * (zk.x - zc.x);
            const double tr = w.x * orr - w.y * oi, ti = w.x * oi + w.y * orr;
            const double ar = er + tr, ai = ei + ti, br = er - tr, bi = ti - ei;
            pa[m] = ar * ar + ai * ai;
            pb[m] = br * br + bi * bi;
        }
        const double p256 = v[H].x * v[H].x + v[H].y * v[H].y;
        wave_sync();
        // bins: k (pa[m]), 512 - k (pb[m]; k = 0: bin 512), 256 (lane 0)
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int m = 0; m < H; ++m) {
            const int k = lane + 64 * m, kb = S - k;
            if (k < nbins) { s0 += pa[m]; s1 += pa[m] * (k * fstep); }
            if (kb < nbins) { s0 += pb[m]; s1 += pb[m] * (kb * fstep); }
        }
        if (lane == 0 && S / 2 < nbins) { s0 += p256; s1 += p256 * ((S / 2) * fstep); }
        const double tot = group_sum<64>(s0);
        const double cog = group_sum<64>(s1) / tot;
        double m2 = 0.0, m3 = 0.0, m4 = 0.0;
        auto acc = [&](double p, int k) {
            const double d = k * fstep - cog, d2 = d * d;
            m2 += p * d2; m3 += p * d2 * d; m4 += p * d2 * d2;
        };
#pragma unroll
        for (int m = 0; m < H; ++m) {
            const int k = lane + 64 * m, kb = S - k;
            if (k < nbins) acc(pa[m], k);
            if (kb < nbins) acc(pb[m], kb);
        }
        if (lane == 0 && S / 2 < nbins) acc(p256, S / 2);
        const double u2 = group_sum<64>(m2) / tot, u3 = group_sum<64>(m3) / tot, u4 = group_sum<64>(m4) / tot;
        if (lane == 0) {
            o[0] = 1.0;
            o[1] = cog;
            o[2] = sqrt(u2);
            o[3] = u3 / (u2 * sqrt(u2));
            o[4] = u4 / (u2 * u2) - 3.0;
        }
    }
}

__global__ __launch_bounds__(64) void moments_stats_kernel(const double* __restrict__ mom, const ClipInfo* __restrict__ ci,
                                                           double* __restrict__ out) {
    const ClipInfo c = ci[blockIdx.x];
    const int lane = threadIdx.x;
    double n[4] = {0, 0, 0, 0}, s[4] = {0, 0, 0, 0};
    for (int i = lane; i < c.n_frames; i += 64) {
        const double* m = mom + (c.frame_off + i) * 5;
        if (m[0] != 0.0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double v = m[1 + q];
                if (v == v) { n[q] += 1; s[q] += v; }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { n[q] = wave_sum_f64(n[q]); s[q] = wave_sum_f64(s[q]); }
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            out[blockIdx.x * 4 + q] = n[q] > 0 ? s[q] / n[q] : __longlong_as_double(0x7ff8000000000000LL);
}

// ---- _speechrate (de Jong & Wempe syllable nuclei; src/mshds_extractor.py:11-125) -----------------------
// One wave per clip.  Parallel parts: parabolic extrema, rank sort (0.99 quantile), local maxima and
// their sinc-70 refined times (four 16-lane groups).  The interval / peak bookkeeping is integer-state
// sequential logic and runs on lane 0 with a per-clip global workspace.
__device__ double value_cubic(const double* __restrict__ y, int n, double ireal) {
    const double x1 = ireal + 1.0;
    if (x1 > n) return y[n - 1];
    if (x1 < 1) return y[0];
    const int midleft = (int)floor(x1);
    if (x1 == (double)midleft) return y[midleft - 1];
    const int midright = midleft + 1;
    int depth = 2;
    if (depth > midright - 1) depth = midright - 1;
    if (depth > n - midleft) depth = n - midleft;
    if (depth <= 0) return y[(int)floor(x1 + 0.5) - 1];
    const double yl = y[midleft - 1], yr = y[midright - 1];
    if (depth == 1) return yl + (x1 - midleft) * (yr - yl);
    const double dyl = 0.5 * (yr - y[midleft - 2]), dyr = 0.5 * (y[midright] - yl);
    const double fil = x1 - midleft, fir = midright - x1;
    return yl * fir + yr * fil - fil * fir * (0.5 * (dyr - dyl) + (fil - 0.5) * (dyl + dyr - 2.0 * (yr - yl)));
}

constexpr int SR_MAX_PEAKS = 4096;

__global__ __launch_bounds__(64) void speechrate_kernel(const double* __restrict__ db_all, const ClipInfo* __restrict__ ci,
                                                        double dt, const double* __restrict__ sel_freq,
                                                        const ClipInfo* __restrict__ pci, double pitch_dt, double ceiling,
                                                        double* __restrict__ work, int64_t work_stride, int max_frames,
                                                        int peak_cap, int in_global, double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const ClipInfo c = ci[blockIdx.x];
    const int n = c.n_frames, lane = threadIdx.x;
    double* o = out + (int64_t)blockIdx.x * 5;
    const double qn = __longlong_as_double(0x7ff8000000000000LL);
    if (n <= 0) {
        if (lane < 5) o[lane] = qn;
        return;
    }
    // contours that do not fit the LDS (clips beyond ~2 minutes) live in the per-clip global scratch instead
    double* gscr = work + (int64_t)blockIdx.x * work_stride + 3 * ((int64_t)max_frames + 2) + 2 * (int64_t)peak_cap;
    double* y = in_global ? gscr : reinterpret_cast<double*>(smem_raw);      // [n] intensity contour
    double* srt = y + ((n + 1) & ~1);                          // [n] sorted copy, later peak positions
    int* pk = reinterpret_cast<int*>(srt + ((n + 1) & ~1));    // [peak_cap] local-maximum indices
    const double* src = db_all + c.frame_off;
    for (int i = lane; i < n; i += 64) y[i] = src[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // parabolic extrema (Vector_getMaximum / Minimum)
    double mx = -INFINITY, mnn = -INFINITY;
    for (int i = lane; i < n; i += 64) {
        const double v = y[i];
        if (i == 0 || i == n - 1) { mx = fmax(mx, v); mnn = fmax(mnn, -v); }
        if (i > 0 && i < n - 1) {
            const double a = y[i - 1], b = y[i + 1];
            if (v > a && v >= b) { const double dy = 0.5 * (b - a), d2 = 2.0 * v - a - b; mx = fmax(mx, d2 != 0.0 ? v + 0.5 * dy * dy / d2 : v); }
            if (-v > -a && -v >= -b) { const double dy = 0.5 * (a - b), d2 = -2.0 * v + a + b; mnn = fmax(mnn, d2 != 0.0 ? -v + 0.5 * dy * dy / d2 : -v); }
        }
    }
    const double max_int = wave_max_f64(mx), min_int = -wave_max_f64(mnn);
    // rank sort -> 0.99 quantile (Praat NUMquantile)
    for (int i = lane; i < n; i += 64) {
        const double v = y[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) { const double u = y[j]; rank += (u < v) || (u == v && j < i); }
        srt[rank] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    double q99;
    if (n == 1) q99 = srt[0];
    else {
        const double place = 0.99 * n + 0.5;
        int left = (int)floor(place);
        left = left < 1 ? 1 : (left > n - 1 ? n - 1 : left);
        q99 = (srt[left] == srt[left - 1]) ? srt[left - 1] : srt[left - 1] + (place - left) * (srt[left] - srt[left - 1]);
    }
    const double silencedb = -25.0, mindip = 2.0, minpause = 0.3, minsound = 0.1;
    double silencedb_1 = q99 + silencedb;
    if (silencedb_1 < min_int) silencedb_1 = min_int;
    const double silencedb_2 = silencedb - (max_int - q99);
    // local maxima in ascending order
    int npk = 0;
    for (int base = 1; base < n - 1; base += 64) {
        const int i = base + lane;
        bool ok = false;
        if (i < n - 1) ok = y[i] > y[i - 1] && y[i] >= y[i + 1];
        const unsigned long long m = __ballot(ok);
        const int pos = npk + __popcll(m & ((1ull << lane) - 1ull));
        if (ok && pos < peak_cap) pk[pos] = i;
        npk += __popcll(m);
    }
    if (npk > peak_cap) npk = peak_cap;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // sinc-70 refined peak positions (reuse srt[] for them), four peaks at a time
    {
        const int l16 = lane & 15, grp = lane >> 4;
        for (int b = 0; b < npk; b += 4) {
            const int k = b + grp;
            const bool live = k < npk;
            double xm, ym;
            improve_max_group<16, false>(y, n, (double)pk[live ? k : 0], 70, 0, n - 1, l16, live, xm, ym);
            if (live && l16 == 0) srt[k] = xm;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (lane != 0) return;
    // ------------------------------ lane 0: sequential bookkeeping ------------------------------
    double* iva = work + (int64_t)blockIdx.x * work_stride;    // interval starts
    double* ivb = iva + (n + 2);                               // interval ends
    double* ivl = ivb + (n + 2);                               // 1 = sounding, 0 = silent
    double* tpk = ivl + (n + 2);                               // kept peak times
    double* vpk = tpk + peak_cap;                              // kept peak values
    const double duration = c.xmax;                            // the Intensity (and its TextGrid) keep the sound's domain [0, xmax]
    int niv = 0;
    {
        const double thr = max_int - fabs(silencedb_2);
        if (minpause > duration || thr < min_int) {
            iva[0] = 0.0; ivb[0] = duration; ivl[0] = 1.0; niv = 1;
        } else {
            double start = 0.0;
            bool state = y[0] < thr;                            // in silence
            for (int i = 1; i < n; ++i) {
                const bool sil = y[i] < thr;
                if (sil != state) {
                    const double tb = c.t1 + (i - 0.5) * dt;
                    iva[niv] = start; ivb[niv] = tb; ivl[niv] = state ? 0.0 : 1.0; ++niv;
                    start = tb; state = sil;
                }
            }
            iva[niv] = start; ivb[niv] = duration; ivl[niv] = state ? 0.0 : 1.0; ++niv;
            for (int pass = 0; pass < 2; ++pass) {
                const double lab = pass == 0 ? 1.0 : 0.0;       // cut short sounding first, then short silences
                const double mind = pass == 0 ? minsound : minpause;
                int i = 0;
                while (i < niv) {
                    if (ivl[i] == lab && (ivb[i] - iva[i]) < mind && niv > 1) {
                        const double a = iva[i], b = ivb[i];
                        for (int k = i; k < niv - 1; ++k) { iva[k] = iva[k + 1]; ivb[k] = ivb[k + 1]; ivl[k] = ivl[k + 1]; }
                        --niv;
                        if (i == 0) iva[0] = a;
                        else ivb[i - 1] = b;                     // previous interval extended (also for the last one)
                    } else ++i;
                }
                const double ml = pass == 0 ? 0.0 : 1.0;        // merge equal neighbours of the other label
                i = 0;
                while (i < niv - 1) {
                    if (ivl[i] == ml && ivl[i + 1] == ivl[i]) {
                        const double a = iva[i];
                        for (int k = i; k < niv - 1; ++k) { iva[k] = iva[k + 1]; ivb[k] = ivb[k + 1]; ivl[k] = ivl[k + 1]; }
                        --niv;
                        iva[i] = a;
                    } else ++i;
                }
            }
        }
    }
    int npauses = 0;
    double phonation = 0.0, begin_speak = 0.0, end_speak = 0.0;
    for (int i = 0; i < niv; ++i)
        if (ivl[i] != 0.0) {
            if (npauses == 0) begin_speak = iva[i];
            end_speak = ivb[i];
            phonation += ivb[i] - iva[i];
            ++npauses;
        }
    if (npauses == 0) {
        for (int k = 0; k < 5; ++k) o[k] = qn;
        return;
    }
    int nkeep = 0;
    for (int k = 0; k < npk; ++k) {
        const double v = value_cubic(y, n, srt[k]);
        if (v > silencedb_1) { tpk[nkeep] = c.t1 + srt[k] * dt; vpk[nkeep] = v; ++nkeep; }
    }
    const ClipInfo pc = pci[blockIdx.x];
    int nsyll = 0;
    if (nkeep > 1) {
        double currenttime = tpk[0], currentint = vpk[0];
        for (int p = 0; p < nkeep - 1; ++p) {
            const double nxt = tpk[p + 1];
            int imin = (int)ceil((currenttime - c.t1) / dt), imax = (int)floor((nxt - c.t1) / dt);
            imin = imin < 0 ? 0 : imin;
            imax = imax > n - 1 ? n - 1 : imax;
            double dip;
            if (imin <= imax) {
                dip = y[imin];
                for (int i = imin + 1; i <= imax; ++i) dip = fmin(dip, y[i]);
            } else {
                int ia = (int)floor((currenttime - c.t1) / dt + 0.5), ib = (int)floor((nxt - c.t1) / dt + 0.5);
                ia = ia < 0 ? 0 : (ia > n - 1 ? n - 1 : ia);
                ib = ib < 0 ? 0 : (ib > n - 1 ? n - 1 : ib);
                dip = fmin(y[ia], y[ib]);
            }
            if (fabs(currentint - dip) > mindip) {
                // valid syllable nucleus at tpk[p]: count it if it is in a sounding interval and voiced
                const double tm = tpk[p];
                bool snd = false;
                for (int k = 0; k < niv; ++k)
                    if ((iva[k] <= tm && tm < ivb[k]) || (k == niv - 1 && tm == ivb[k])) { snd = ivl[k] != 0.0; break; }
                bool voiced = false;
                if (pc.n_frames > 0) {
                    const double ireal = (tm - pc.t1) / pitch_dt;
                    const double il = floor(ireal);
                    const int64_t near = (ireal - il < 0.5) ? (int64_t)il : (int64_t)il + 1;
                    if (near >= 0 && near < pc.n_frames) {
                        const double pf = sel_freq[pc.frame_off + near];
                        voiced = pf > 0.0 && pf < ceiling;
                    }
                }
                if (snd && voiced) ++nsyll;
            }
            currenttime = nxt;
            currentint = value_cubic(y, n, (nxt - c.t1) / dt);
        }
    }
    const double original_dur = end_speak - begin_speak;
    const int n_pauses = npauses - 1;
    o[0] = original_dur > 0 ? nsyll / original_dur : 0.0;
    o[1] = phonation > 0 ? nsyll / phonation : 0.0;
    o[2] = original_dur > 0 ? phonation / original_dur : 0.0;
    o[3] = original_dur > 0 ? n_pauses / original_dur : 0.0;
    o[4] = n_pauses > 0 ? (original_dur - phonation) / n_pauses : 0.0;
}

}  // namespace mshds
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::mshds;

extern "C" {

int rsaf_mshds_clip_peak(const float* wav, const void* clip_info, int n_clips, double* gpeak, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0, "negative n_clips");
    if (n_clips == 0) return RSAF_OK;
    RSAF_CHECK_ARG(wav && clip_info && gpeak, "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("mshds_clip_peak", s, 0.0, 0.0);
    hipLaunchKernelGGL(clip_peak_kernel, dim3(n_clips), dim3(256), 0, s, wav, (const ClipInfo*)clip_info, gpeak);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_mshds_intensity(const float* wav, const void* clip_info, int n_clips, int max_frames, const double* window,
                         int half_window, double time_step, int subtract_mean, double* db_out, double* stats_out,
                         rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0 && n_clips <= 65535 && max_frames >= 0, "bad clip/frame count");
    if (n_clips == 0) return RSAF_OK;
    RSAF_CHECK_ARG(wav && clip_info && window && db_out && stats_out, "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    if (max_frames > 0) {
        ProfScope prof("mshds_intensity", s, 0.0, 0.0);
        hipLaunchKernelGGL(intensity_kernel, dim3((max_frames + 3) / 4, n_clips), dim3(256), 0, s, wav,
                           (const ClipInfo*)clip_info, window, half_window, time_step, subtract_mean, db_out);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(intensity_stats_kernel, dim3(n_clips), dim3(64), 0, s, db_out, (const ClipInfo*)clip_info, stats_out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

// peaks of an n-frame contour: at most n/2; the LDS form keeps SR_MAX_PEAKS of them (a smooth 16 ms contour of at most
// ~8 500 frames has far fewer), the global-memory form of long clips sizes the lists exactly
static int sr_peak_cap(int max_frames, bool in_global) { return in_global ? max_frames / 2 + 2 : SR_MAX_PEAKS; }
static bool sr_in_global(int max_frames) {
    return (size_t)2 * ((max_frames + 1) & ~1) * sizeof(double) + SR_MAX_PEAKS * sizeof(int) > 150 * 1024;
}

int64_t rsaf_mshds_speechrate_workspace_doubles(int max_frames) {
    const bool g = sr_in_global(max_frames);
    const int64_t cap = sr_peak_cap(max_frames, g);
    return 3 * ((int64_t)max_frames + 2) + 2 * cap + (g ? 2 * ((int64_t)max_frames + 2) + cap / 2 + 2 : 0);
}

int rsaf_mshds_speechrate(const double* intensity_db, const void* clip_info, int n_clips, int max_frames,
                          double intensity_dt, const double* sel_freq, const void* pitch_clip_info, double pitch_dt,
                          double pitch_ceiling, double* workspace, double* out, rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0 && max_frames >= 0, "bad clip/frame count");
    if (n_clips == 0) return RSAF_OK;
    RSAF_CHECK_ARG(intensity_db && clip_info && sel_freq && pitch_clip_info && workspace && out, "NULL pointer");
    const bool in_global = sr_in_global(max_frames);
    const int peak_cap = sr_peak_cap(max_frames, in_global);
    const size_t lds = in_global ? 0 : (size_t)2 * ((max_frames + 1) & ~1) * sizeof(double) + SR_MAX_PEAKS * sizeof(int);
    hipStream_t s = (hipStream_t)stream;
    if (lds > 48 * 1024)
        RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)speechrate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds));
    ProfScope prof("mshds_speechrate", s, 0.0, 0.0);
    hipLaunchKernelGGL(speechrate_kernel, dim3(n_clips), dim3(64), lds, s, intensity_db, (const ClipInfo*)clip_info,
                       intensity_dt, sel_freq, (const ClipInfo*)pitch_clip_info, pitch_dt, pitch_ceiling, workspace,
                       rsaf_mshds_speechrate_workspace_doubles(max_frames), max_frames, peak_cap, in_global ? 1 : 0, out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_mshds_hnr_mean(const double* sel_freq, const double* sel_strength, const void* clip_info, int n_clips,
                        double* out, rsaf_stream_t stream) {
    if (n_clips <= 0) return RSAF_OK;
    RSAF_CHECK_ARG(sel_freq && sel_strength && clip_info && out, "NULL pointer");
    hipLaunchKernelGGL(hnr_stats_kernel, dim3(n_clips), dim3(64), 0, (hipStream_t)stream, sel_freq, sel_strength,
                       (const ClipInfo*)clip_info, out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

int rsaf_mshds_spectral_moments(const float* wav, const void* clip_info, const void* pitch_clip_info, int n_clips,
                                int max_frames, const double* sel_freq, double pitch_dt, double ceiling,
                                const double* window, const double* twiddle, int nsamp_window, int nfft, int nbins,
                                double time_step, double freq_step, double* moments, double* stats_out,
                                rsaf_stream_t stream) {
    RSAF_CHECK_ARG(n_clips >= 0 && n_clips <= 65535 && max_frames >= 0, "bad clip/frame count");
    if (n_clips == 0) return RSAF_OK;
    RSAF_CHECK_ARG(wav && clip_info && pitch_clip_info && sel_freq && window && twiddle && moments && stats_out,
                   "NULL pointer");
    RSAF_CHECK_ARG(nfft > 0 && (nfft & (nfft - 1)) == 0 && nbins > 0 && nbins <= nfft / 2 + 1, "bad FFT geometry");
    hipStream_t s = (hipStream_t)stream;
    RSAF_CHECK_ARG(nfft >= 2 && (nfft & (nfft - 1)) == 0 && nfft >= nsamp_window && nbins <= nfft / 2 + 1, "nfft must be a power of two >= window");
    const size_t lds = (size_t)(nfft + nbins) * sizeof(double);
    RSAF_CHECK_ARG(lds <= 60 * 1024, "spectrogram window too long");
    if (max_frames > 0) {
        ProfScope prof("mshds_spec_moments", s, 0.0, 0.0);
        const int threads = nfft >= 2048 ? 512 : 256;      // nfft / 4 butterflies per pass of the half-length FFT
        const char* e = getenv("RSAF_SPM_WAVE");
        if (nfft == 1024 && nsamp_window >= 2 && !(e && e[0] == '0'))
            hipLaunchKernelGGL(spec_moments_wave_kernel, dim3((max_frames + SPM_FRAMES - 1) / SPM_FRAMES, n_clips), dim3(64), 0, s,
                               wav, (const ClipInfo*)clip_info, (const ClipInfo*)pitch_clip_info, sel_freq, pitch_dt, ceiling,
                               window, (const double2*)twiddle, nsamp_window, nsamp_window / 2, nbins, time_step, freq_step,
                               moments);
        else
        hipLaunchKernelGGL(spec_moments_kernel, dim3(max_frames, n_clips), dim3(threads), lds, s, wav,
                           (const ClipInfo*)clip_info, (const ClipInfo*)pitch_clip_info, sel_freq, pitch_dt, ceiling,
                           window, (const double2*)twiddle, nsamp_window, nsamp_window / 2, nfft, nbins, time_step,
                           freq_step, moments);
        RSAF_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(moments_stats_kernel, dim3(n_clips), dim3(64), 0, s, moments, (const ClipInfo*)clip_info, stats_out);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}

}  // extern "C"
