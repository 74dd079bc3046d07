// The shared map of the openSMILE-style chain (smile_lld.hip, smile_pitch.hip, smile_functionals.hip), each part stated
// once: the 38 LLD rows and the three functional levels, the 23 per-frame sums the frame kernel stashes for its end-of-run
// pass, and the carve-up of one wave's LDS in the frame kernel with the lifetime of every region.
//
// Plain C++17, no HIP types: tests/host/smile_layout_replay.cpp compiles it with g++ and checks the sizes, the containment,
// the liveness table and the row names against smile.py and the oracle (tests/test_smile_layout_host.py).
#pragma once
#include <cstddef>

#include "rsaf.h"

#if defined(__HIPCC__)
#define SL_HD __host__ __device__ __forceinline__
#else
#define SL_HD inline
#endif

namespace rsaf {
namespace smile {

// ---- LLD rows: lld[row * total_frames + frame], contour-major (include/rsaf.h) -----------------------------------------
enum LldRow : int {
    LLD_RMS_ENERGY = 0,
    LLD_MFCC1 = 1, LLD_MFCC2, LLD_MFCC3, LLD_MFCC4, LLD_MFCC5, LLD_MFCC6, LLD_MFCC7, LLD_MFCC8, LLD_MFCC9, LLD_MFCC10,
    LLD_MFCC11, LLD_MFCC12 = 12,
    LLD_ZCR = 13,
    LLD_F0_FINAL = 14,
    LLD_VOICING = 15,
    LLD_INTENSITY = 16,
    LLD_LOUDNESS,
    LLD_JITTER_LOCAL,
    LLD_JITTER_DDP,
    LLD_SHIMMER_LOCAL,
    LLD_LOG_HNR = 21,
    LLD_BAND_250_650 = 22,
    LLD_BAND_1000_4000,
    LLD_ROLLOFF_25, LLD_ROLLOFF_50, LLD_ROLLOFF_75, LLD_ROLLOFF_90,
    LLD_FLUX,
    LLD_CENTROID,
    LLD_ENTROPY,
    LLD_VARIANCE,
    LLD_SKEWNESS,
    LLD_KURTOSIS,
    LLD_SLOPE,
    LLD_SHARPNESS,
    LLD_HARMONICITY,
    LLD_FLATNESS = 37,
    LLD_COUNT
};
static_assert(LLD_COUNT == RSAF_SMILE_NLLD, "the row enum and the ABI's row count must agree");

// the contour names of the cCsvSink header (smile.LLD_NAMES states the same list for Python)
constexpr const char* LLD_ROW_NAME[LLD_COUNT] = {
    "pcm_RMSenergy", "mfcc[1]", "mfcc[2]", "mfcc[3]", "mfcc[4]", "mfcc[5]", "mfcc[6]", "mfcc[7]", "mfcc[8]", "mfcc[9]",
    "mfcc[10]", "mfcc[11]", "mfcc[12]", "pcm_zcr", "F0final", "voicingFinalUnclipped",
    "pcm_intensity", "pcm_loudness", "jitterLocal", "jitterDDP", "shimmerLocal", "logHNR",
    "pcm_fftMag_fband250-650", "pcm_fftMag_fband1000-4000", "pcm_fftMag_spectralRollOff25.0",
    "pcm_fftMag_spectralRollOff50.0", "pcm_fftMag_spectralRollOff75.0", "pcm_fftMag_spectralRollOff90.0",
    "pcm_fftMag_spectralFlux", "pcm_fftMag_spectralCentroid", "pcm_fftMag_spectralEntropy", "pcm_fftMag_spectralVariance",
    "pcm_fftMag_spectralSkewness", "pcm_fftMag_spectralKurtosis", "pcm_fftMag_spectralSlope", "pcm_fftMag_psySharpness",
    "pcm_fftMag_spectralHarmonicity", "pcm_fftMag_spectralFlatness"};

// functional levels (lld, lld2, lld3 of Androids.conf:284-368): rows [begin, end) share one block of cCsvSink columns
constexpr int LLD_NLEVELS = 3;
constexpr int LLD_LEVEL_BEGIN[LLD_NLEVELS] = {LLD_RMS_ENERGY, LLD_INTENSITY, LLD_BAND_250_650};
constexpr int LLD_LEVEL_END[LLD_NLEVELS] = {LLD_INTENSITY, LLD_BAND_250_650, LLD_COUNT};
static_assert(LLD_LEVEL_END[0] == 16 && LLD_LEVEL_END[1] == 22 && LLD_LEVEL_END[2] == 38, "levels {0,16} {16,22} {22,38}");

// ---- the sums a frame leaves for the end-of-run pass ----------------------------------------------------------------------
// Three groups of eight go through reduce8 (total q of a group lands in slot group base + q); the roll-off points follow.
enum SumSlot : int {
    SUM_GROUP_A = 0,                 // first reduction
    SUM_W2 = 0,                      //   sum win^2                     (RMS energy)
    SUM_HAM_W2,                      //   sum ham win^2                 (intensity)
    SUM_ZC,                          //   zero crossings
    SUM_TOTAL,                       //   sum P, P = |X|^2
    SUM_P_F,                         //   sum P f                       (centroid, slope)
    SUM_MAG,                         //   sum |X|                       (harmonicity)
    SUM_BAND1,                       //   sum P over 250 - 650 Hz
    SUM_BAND2,                       //   sum P over 1 000 - 4 000 Hz
    SUM_GROUP_B = 8,                 // second reduction
    SUM_SHARP = 8,                   //   sum P bark g(bark)
    SUM_FLUX,                        //   sum (|X| - |X_prev|)^2
    SUM_LN_P,                        //   sum ln P                      (flatness)
    SUM_P_LN_P,                      //   sum P ln P                    (entropy)
    SUM_HARM,                        //   sum of the peaks above their neighbours' mean
    SUM_B_PAD5, SUM_B_PAD6, SUM_B_PAD7,   // written as zeros (the group is eight wide)
    SUM_GROUP_C = 16,                // third reduction: central moments about the centroid
    SUM_M2 = 16,
    SUM_M3,
    SUM_M4,
    SUM_ROLLOFF = 19,                // + q, q = 0 .. 3: roll-off frequency at 25 / 50 / 75 / 90 %
    SUM_ROLLOFF_LAST = SUM_ROLLOFF + 3,
    NSUM                             // doubles per frame in the stash
};
static_assert(NSUM == 23, "the stash layout is 23 doubles per frame");
static_assert(SUM_GROUP_A % 8 == 0 && SUM_GROUP_B == SUM_GROUP_A + 8 && SUM_GROUP_C == SUM_GROUP_B + 8 && SUM_M4 < SUM_ROLLOFF,
              "a reduction group is eight consecutive slots");

constexpr int RUNW = 16;                 // frames per wave
constexpr int RED_D = 8 * 65;            // doubles of the 8-sums-at-a-time reduction scratch

// ---- LDS of one wave of the frame kernel, in doubles ----------------------------------------------------------------------
//
//   region            doubles                 holds, in phase order (phases as in tools/smile_phase.py)
//   fft     [0, Z_D)                          1: the packed-real FFT, c64[NC].  Dead once the magnitudes are out; then
//     low half  [0, NB)                       5: enhanced spectrum -> 6-7: spline moments (once the smoothing has read it)
//     red   (when RED_IN_Z) [0, RED_D)        2: reduction scratch
//   octave  [OFF_S, OFF_S + S_D)              the second half of the dead FFT buffer + a zero pad behind it
//     bins  [OFF_S, OFF_S + NB)               4: 26 log mel energies; 7-8: octave spectrum; 9-10: peak list, NC / 2 scores
//                                             then NC / 2 frequencies
//     zeros [OFF_S + NB, OFF_S + S_D)         what the harmonic shifts of phase 8 read behind bin NC.  The prologue writes zeros
//                                             to [Z_D, OFF_S + S_D), i.e. from octave index Z_D - OFF_S on (NC in the padded
//                                             instances, NC - 2 in the trimmed one): everything of the octave region outside the
//                                             FFT buffer.  The entries of that range below OFF_S + NB are bins, rewritten by
//                                             phase 7 every frame; from OFF_S + NB on nobody writes after the prologue
//   P0, P1  ARR each                          the two magnitude arrays.  this_frame(tr): 1-10, and it IS the next frame's
//                                             prev_frame; prev_frame(tr): 2 (flux), then free: 5-7 smoothed spectrum,
//                                             8-9 summation spectrum
//   stash   RUNW * NSUM                       every frame's sums, read by the end-of-run pass
//   red     (when !RED_IN_Z) RED_D            2: reduction scratch behind the stash
//
// Round 4 brought this from 15.6 to 12.7 KB per wave at 16 kHz (12 instead of 10 waves per CU).  The 2 048-point instance
// (44.1 / 48 kHz) is trimmed to the last double: 40 928 bytes per wave = FOUR waves per CU instead of three (its arrays
// need NC + 1 entries and the FFT buffer exactly 2 NC; the shorter instances keep the padding the reduction scratch in the
// FFT buffer relies on).
template <int LOG2N>
struct Geo {
    static constexpr int NFFT = 1 << LOG2N;
    static constexpr int NC = NFFT / 2;              // complex points of the packed-real transform
    static constexpr int NB = NC + 1;                // magnitude bins
    static constexpr int PPL = NC / 64;              // bins per lane (2, 4, 8, 16)
    static constexpr int NBP = NC + 8;               // padded length of the per-bin tables
    static constexpr bool TRIM = LOG2N >= 11;
    static constexpr int Z_D = 2 * NC + (TRIM ? 0 : 8);   // FFT buffer
    static constexpr int ARR = NC + (TRIM ? 2 : 8);       // one per-bin array (NB = NC + 1 entries)
    static constexpr int PAD_D = ((NC * 5) / 8 + 8 + 7) & ~7;   // zeros behind the octave spectrum: longer than the largest harmonic shift (< 0.62 NC)
    static constexpr int S_D = (Z_D - ARR) + PAD_D;  // the octave spectrum's room: NB bins + the pad
    static constexpr int MELCAP = NC / 4;            // cap of the longest side of a triangular mel band, in bins
    static constexpr int NPEAK = NC / 2;             // most peaks a summation spectrum can have
    static constexpr bool RED_IN_Z = Z_D >= RED_D;   // the reduction scratch lives in the FFT buffer when it fits
    static constexpr int OFF_Z = 0, OFF_S = ARR, OFF_P0 = Z_D + PAD_D, OFF_P1 = OFF_P0 + ARR, OFF_STASH = OFF_P1 + ARR;
    static constexpr int STASH_D = RUNW * NSUM;
    static constexpr int OFF_RED = RED_IN_Z ? 0 : OFF_STASH + STASH_D;
    static constexpr int WAVE_D = OFF_STASH + STASH_D + (RED_IN_Z ? 0 : RED_D);
    static constexpr size_t bytes() { return (size_t)WAVE_D * sizeof(double); }

    static_assert(2 * NC <= Z_D && NB <= ARR, "the transform and a magnitude array must fit their regions");
    static_assert(S_D >= NB + (NC * 5) / 8 + 1, "octave spectrum + pad must fit");
    static_assert(OFF_S + S_D == OFF_P0, "the octave region ends where the magnitude arrays begin");
    static_assert(NB <= OFF_S, "the spline moments (low half) are read while the octave spectrum is written");
    static_assert(2 * NC <= OFF_S + NB, "the transform must leave the zeros behind the octave spectrum alone");
    static_assert(2 * NPEAK <= NB, "the peak list (scores + frequencies) must leave the zeros alone");
    static_assert(RED_IN_Z ? (OFF_RED + RED_D <= Z_D && OFF_RED + RED_D <= OFF_S + NB)
                           : (OFF_RED >= OFF_STASH + STASH_D && OFF_RED + RED_D <= WAVE_D),
                  "the reduction scratch runs while both magnitude arrays, the stash and the zeros are live");
    static_assert(OFF_Z % 2 == 0 && OFF_S % 2 == 0 && OFF_P0 % 2 == 0 && OFF_P1 % 2 == 0 && OFF_STASH % 2 == 0 && OFF_RED % 2 == 0,
                  "16-byte alignment: the FFT buffer is read as c64, the arrays in pairs");
};

// One wave's views of its LDS (base 16-byte aligned).  Each accessor is one lifetime of the table above.
template <int LOG2N>
struct WaveLds {
    using G = Geo<LOG2N>;
    template <class C> static SL_HD C* fft(double* base) { return reinterpret_cast<C*>(base + G::OFF_Z); }   // c64[NC]
    static SL_HD double* enhanced(double* base) { return base + G::OFF_Z; }                  // [NB]
    static SL_HD double* moments(double* base) { return base + G::OFF_Z; }                   // [NB], after the smoothing has consumed enhanced()
    static SL_HD double* octave(double* base) { return base + G::OFF_S; }                    // [S_D]: NB bins + zeros
    static SL_HD double* log_mel(double* base) { return base + G::OFF_S; }                   // [NMEL], before the octave spectrum exists
    static SL_HD double* peak_score(double* base) { return base + G::OFF_S; }                // [NPEAK], once the octave spectrum is summed
    static SL_HD double* peak_freq(double* base) { return base + G::OFF_S + G::NPEAK; }      // [NPEAK]
    static SL_HD double* this_frame(double* base, int tr) { return base + ((tr & 1) ? G::OFF_P1 : G::OFF_P0); }   // [NB] magnitudes of frame tr of the run
    static SL_HD double* prev_frame(double* base, int tr) { return base + ((tr & 1) ? G::OFF_P0 : G::OFF_P1); }   // [NB] the frame before; free after the flux
    static SL_HD double* stash(double* base, int tr) { return base + G::OFF_STASH + tr * NSUM; }                  // [NSUM]
    static SL_HD double* red(double* base) { return base + G::OFF_RED; }                     // [RED_D]
};

}  // namespace smile
}  // namespace rsaf
