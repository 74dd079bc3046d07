// csrc/smile_layout.h on the host: the LDS carve-up of the openSMILE-style frame kernel at its four FFT lengths, the stash
// slots and the LLD rows.  Per LOG2N = 8 .. 11: (1) bytes() is what the launch has always requested, (2) every region the
// accessors of WaveLds hand out lies inside the request, (3) no two regions that are live in the same phase overlap (the
// liveness table below; phases as in tools/smile_phase.py, 0 = the prologue of a run, 11 = the end-of-run pass), (4) the
// regions start 16-byte aligned.  Then NSUM, and the rows and levels for the Python side to compare with smile.py and
// the oracle.  Prints "ok ..." / "FAIL ..." lines; exit status 1 if any check failed.
#include <cstdio>
#include <string>
#include <vector>

#include "smile_layout.h"

using namespace rsaf::smile;

static int g_failed = 0;
static void report(bool ok, int log2n, const std::string& what) {
    std::printf("%s %d %s\n", ok ? "ok" : "FAIL", log2n, what.c_str());
    if (!ok) g_failed = 1;
}

constexpr unsigned ph(int a, int b) { return ((1u << (b + 1)) - 1u) & ~((1u << a) - 1u); }   // phases a .. b
constexpr unsigned ALWAYS = ph(0, 11);

struct Region {
    const char* name;
    long begin, len;      // doubles from the wave's base
    unsigned live;        // bit k: live in phase k
};

struct Cplx { double re, im; };

template <int LOG2N>
static void check() {
    using G = Geo<LOG2N>;
    using L = WaveLds<LOG2N>;
    static const long WANT[4] = {12096, 12672, 22144, 40928};
    report((long)G::bytes() == WANT[LOG2N - 8], LOG2N, "bytes " + std::to_string(G::bytes()));

    std::vector<double> store(G::WAVE_D + 2);
    double* base = store.data();
    auto off = [&](const double* p) { return (long)(p - base); };
    const int NMEL = 26;
    // frame tr = 0 of a run; tr = 1 swaps the two magnitude arrays
    const std::vector<Region> R = {
        {"fft", off(reinterpret_cast<double*>(L::template fft<Cplx>(base))), 2L * G::NC, ph(0, 1)},
        {"red", off(L::red(base)), RED_D, ph(2, 2)},
        {"log_mel", off(L::log_mel(base)), NMEL, ph(4, 4)},
        {"enhanced", off(L::enhanced(base)), G::NB, ph(5, 5)},
        {"moments", off(L::moments(base)), G::NB, ph(6, 7)},
        {"octave bins", off(L::octave(base)), G::NB, ph(7, 8)},
        {"octave zeros", off(L::octave(base)) + G::NB, G::S_D - G::NB, ALWAYS},
        {"peak_score", off(L::peak_score(base)), G::NPEAK, ph(9, 10)},
        {"peak_freq", off(L::peak_freq(base)), G::NPEAK, ph(9, 10)},
        {"this_frame", off(L::this_frame(base, 0)), G::NB, ph(1, 10)},
        {"prev_frame", off(L::prev_frame(base, 0)), G::NB, ph(0, 2) | ph(5, 9)},
        {"stash", off(L::stash(base, 0)), (long)RUNW * NSUM, ALWAYS},
    };
    bool inside = true, aligned = true, disjoint = true;
    std::string why;
    for (const Region& a : R) {
        if (a.begin < 0 || a.len <= 0 || (a.begin + a.len) * (long)sizeof(double) > (long)G::bytes()) { inside = false; why += std::string(" ") + a.name; }
        // (the zeros begin behind bin NC, wherever that falls: nothing reads them in pairs)
        if (a.begin % 2 && std::string(a.name) != "octave zeros") { aligned = false; why += std::string(" ") + a.name; }
    }
    for (size_t i = 0; i < R.size(); ++i)
        for (size_t j = i + 1; j < R.size(); ++j)
            if ((R[i].live & R[j].live) && R[i].begin < R[j].begin + R[j].len && R[j].begin < R[i].begin + R[i].len) {
                disjoint = false;
                why += std::string(" ") + R[i].name + "/" + R[j].name;
            }
    report(inside, LOG2N, "every region inside the request" + (inside ? "" : ":" + why));
    report(disjoint, LOG2N, "no two regions live in one phase overlap" + (disjoint ? "" : ":" + why));
    report(aligned, LOG2N, "16-byte alignment" + (aligned ? "" : ":" + why));
    report(L::this_frame(base, 1) == L::prev_frame(base, 0) && L::prev_frame(base, 1) == L::this_frame(base, 0) &&
               L::stash(base, RUNW - 1) + NSUM <= base + G::WAVE_D && L::stash(base, 1) == L::stash(base, 0) + NSUM,
           LOG2N, "the magnitude arrays swap per frame; one stash row per frame of the run");
}

int main() {
    check<8>();
    check<9>();
    check<10>();
    check<11>();
    report(NSUM == 23 && SUM_ROLLOFF_LAST == NSUM - 1 && SUM_GROUP_B == 8 && SUM_GROUP_C == 16, 0, "NSUM == 23");
    for (int i = 0; i < LLD_COUNT; ++i) std::printf("row %d %s\n", i, LLD_ROW_NAME[i]);
    for (int l = 0; l < LLD_NLEVELS; ++l) std::printf("level %d %d\n", LLD_LEVEL_BEGIN[l], LLD_LEVEL_END[l]);
    return g_failed;
}
