// MSHDS pitch-corrected Ltas -> "Get slope" and robust tilt, a float64 kernel for gfx950.
//
// Serves _extract_Slope_Tilt (:227-251) of src/mshds_extractor.py, from the cc pulses (mshds_pulses.hip).
// Semantics = oracle/mshds_oracle.py.  What follows the bands' dB values (fill, slope, tilt): mshds_voice_layout.h.
//
// One workgroup of 256 threads per clip; every wave takes every fourth pulse.  A pulse whose two neighbouring intervals are
// plausible periods contributes the energy spectrum of the one period around it: a DFT of exactly that many
// samples (lane = frequency bin, rotation recurrence over the samples), binned into 100 Hz bands.
// Per-wave band sums are combined in a fixed order, so the result does not depend on scheduling.
#include "mshds_common.h"
#include "mshds_voice_layout.h"

namespace rsaf {
namespace mshds {

constexpr int LTAS_MAXN = 1024;        // samples of one period that fit the LDS staging (longest period 20 ms = 320)

__global__ __launch_bounds__(256) void ltas_kernel(const float* __restrict__ wav, const ClipInfo* __restrict__ ci,
                                                   const double* __restrict__ pulses, int max_pulses,
                                                   const int* __restrict__ n_pulses, double shortest, double longest,
                                                   double max_factor, double* __restrict__ out) {
    __shared__ double s_energy[4][LTAS_NB], s_count[4][LTAS_NB], s_z[LTAS_NB];
    __shared__ float s_x[4][LTAS_MAXN];
    __shared__ int s_periods[4], s_fail[4];
    const ClipInfo c = ci[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* x = wav + c.sample_off;
    const int n = c.n_samples;
    const double* pts = pulses + (int64_t)blockIdx.x * max_pulses;
    const int np_ = n_pulses[blockIdx.x];
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
        wave_lds_sync();
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
            wave_lds_sync();
        }
        ++periods;
    }
    if (lane == 0) { s_periods[wv] = periods; s_fail[wv] = fail; }
    __syncthreads();
    if (tid == 0) {
        const int total_periods = s_periods[0] + s_periods[1] + s_periods[2] + s_periods[3];
        const int failed = s_fail[0] | s_fail[1] | s_fail[2] | s_fail[3];
        double slope = qnan(), tilt = qnan();
        if (np_ - 2 >= 1 && total_periods >= 1 && !failed) {
            double total = 0.0;
            for (int b = 0; b < LTAS_NB; ++b) {
                s_energy[0][b] = (s_energy[0][b] + s_energy[1][b]) + (s_energy[2][b] + s_energy[3][b]);
                s_count[0][b] = (s_count[0][b] + s_count[1][b]) + (s_count[2][b] + s_count[3][b]);
                total += s_count[0][b];
            }
            const double duration = c.xmax;                      // PointProcess_Sound_to_Ltas divides by sound->xmax - sound->xmin
            for (int b = 0; b < LTAS_NB; ++b) {
                double db = qnan();
                if (s_count[0][b] > 0.0) {
                    const double mean_e = s_energy[0][b] / s_count[0][b];
                    db = 10.0 * log10(mean_e * (total / LTAS_NB) / LTAS_BW / duration / 4.0e-10);
                }
                s_z[b] = db;
            }
            ltas_slope_tilt(s_z, &slope, &tilt);
        }
        out[2 * blockIdx.x] = slope;
        out[2 * blockIdx.x + 1] = tilt;
    }
}

}  // namespace mshds
}  // namespace rsaf

using namespace rsaf;
using namespace rsaf::mshds;

extern "C" {

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

}  // extern "C"
