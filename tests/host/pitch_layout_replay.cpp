// csrc/mshds_pitch_layout.h on the host: the LDS requests, the workspace size and the frame record of the MSHDS pitch
// analysis at the geometries mshds._PitchGeom produces for the analyses of the feature scripts.  Per row: (1) the sizes
// are the ones the hand-written formulas of the kernels' first form gave (computed from those formulas, the first
// autocorrelation and cross-correlation rows also by hand), (2) every array of every layout lies inside bytes(), no two
// arrays overlap, every double array starts 8-byte aligned and the correlation array 16-byte aligned, (3) the FrameHdr
// fields sit where the kernels' packed loads expect them.  Prints "ok <row>" per row; exit status 1 on the first failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mshds_pitch_layout.h"
#include "wave_fft.h"

using namespace rsaf::mshds;

struct Row {
    const char* name;
    int is_cc, nw, min_lag, max_lag, ixmax, Lr, depth;   // depth: as passed to pitch_r_range (a grouped plan passes 30)
    int ncc, wave_r;                                     // CC: complex points of the workgroup kernel's request; wave kernel R (0: none)
    long lds_cand, lds_corr, lds_cell, cc_wave_sy, ws_bytes_per_frame;   // -1: not applicable
};

static const Row ROWS[] = {
    {"AC 75/500, 3, 70", 0, 638, 32, 214, 319, 319, 70, 0, 0, 10320, -1, 44032, -1, 10888},
    {"AC 50/600, 3, 70", 0, 958, 26, 321, 479, 479, 70, 0, 0, 11232, -1, 64512, -1, 12168},
    {"AC 24/300, 3, 70", 0, 1998, 53, 668, 999, 999, 70, 0, 0, 13792, -1, 131072, -1, 16328},
    {"AC 400/1600, 3, 70", 0, 118, 10, 41, 59, 59, 70, 0, 0, 8656, -1, 10752, -1, 8808},
    {"AC 30/450, 3, 70", 0, 1598, 35, 534, 799, 799, 70, 0, 0, 12864, -1, 105472, -1, 14728},
    {"CC 100/8000, 4.5, 700, per-cell", 1, 718, 2, 161, 718, 161, 30, 1024, 16, 9504, 34320, 24064, 164, 9624},
    {"CC 100/8000, 4.5, 700, in-kernel", 1, 718, 2, 161, 718, 161, 700, 1024, 16, 12896, 34320, 24064, 164, 9624},
    {"CC 60/8000, 4.5, 700, per-cell", 1, 1198, 2, 268, 1198, 268, 30, 2048, 32, 10352, 67952, 37888, 270, 10480},
    {"CC 40/8000, 4.5, 700, per-cell (N = 4096)", 1, 1798, 2, 401, 1798, 401, 30, 4096, 0, 11424, 134544, 54784, 404, 11544},
    {"CC 100/500, 1.0, 70", 1, 158, 32, 158, 158, 158, 70, 512, 16, 9296, 17920, 23552, 160, 9600},
};

static const char* g_row = "";
static void fail(const std::string& what) {
    std::printf("FAIL %s: %s\n", g_row, what.c_str());
    std::exit(1);
}
static void expect(long got, long want, const char* what) {
    if (got != want) fail(std::string(what) + ": " + std::to_string(got) + ", expected " + std::to_string(want));
}

struct Span { const char* name; long begin, bytes, align; };

// every array inside [0, total), aligned, and no two overlapping
static void check_spans(const char* layout, std::vector<Span> s, long total) {
    for (const Span& a : s) {
        if (a.begin < 0 || a.bytes <= 0 || a.begin + a.bytes > total)
            fail(std::string(layout) + "." + a.name + " [" + std::to_string(a.begin) + ", " + std::to_string(a.begin + a.bytes) +
                 ") leaves the " + std::to_string(total) + " bytes requested");
        if (a.begin % a.align) fail(std::string(layout) + "." + a.name + " is not " + std::to_string(a.align) + "-byte aligned");
    }
    std::sort(s.begin(), s.end(), [](const Span& a, const Span& b) { return a.begin < b.begin; });
    for (size_t i = 1; i < s.size(); ++i)
        if (s[i - 1].begin + s[i - 1].bytes > s[i].begin) fail(std::string(layout) + "." + s[i - 1].name + " overlaps " + s[i].name);
}

template <class T>
static Span span(const char* name, const char* base, const T* p, long elems, long align = (long)sizeof(T)) {
    return Span{name, (long)(reinterpret_cast<const char*>(p) - base), elems * (long)sizeof(T), align};
}

struct Cplx { double re, im; };

static void check_row(const Row& R) {
    g_row = R.name;
    std::vector<double> store(40000);                              // 320 KB, 16-byte aligned start below
    char* lds = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(store.data()) + 15) & ~(uintptr_t)15);

    // candidate kernel
    int r_lo, r_hi;
    pitch_r_range(R.ixmax, R.Lr, R.min_lag, R.max_lag, R.depth, &r_lo, &r_hi);
    const CandLds cand(r_lo, r_hi);
    expect((long)cand.bytes(), R.lds_cand, "lds_cand");
    {
        double* l = cand.lists(lds);
        int* li = reinterpret_cast<int*>(l);
        check_spans("CandLds",
                    {span("r_store", lds, cand.r_store(lds), r_hi - r_lo + 1, 16),
                     span("mfreq", lds, l + CandLds::MFREQ, MAX_MAXIMA), span("mstr", lds, l + CandLds::MSTR, MAX_MAXIMA),
                     span("mloc", lds, l + CandLds::MLOC, MAX_MAXIMA), span("cf", lds, l + CandLds::CF, MAXC),
                     span("cs", lds, l + CandLds::CS, MAXC), span("cloc", lds, l + CandLds::CLOC, MAXC),
                     span("maxlag", lds, li + CandLds::MAXLAG, MAX_MAXIMA), span("place", lds, li + CandLds::PLACE, MAXC),
                     span("place2", lds, li + CandLds::PLACE2, MAXC), span("cnt", lds, li + CandLds::CNT, CandLds::CNT_INTS),
                     span("cf2", lds, l + CandLds::CF2, MAXC), span("cs2", lds, l + CandLds::CS2, MAXC),
                     span("cloc2", lds, l + CandLds::CLOC2, MAXC), span("part", lds, l + CandLds::PART, PC_DOUBLES)},
                    (long)cand.bytes());
    }
    // per-cell coefficient kernel: the lags 0 .. Lr padded to a multiple of four
    const int ntap_pad = (R.Lr + 1 + 3) & ~3;
    const CellLds cell(ntap_pad);
    expect((long)cell.bytes(), R.lds_cell, "lds_cell");
    check_spans("CellLds", {span("tab", lds, cell.tab(lds), (long)ntap_pad * NCH), span("queues", lds, cell.queues(lds), 4 * CELL_Q)},
                (long)cell.bytes());
    if (R.is_cc) {
        // workgroup cross-correlation kernel
        const CcLds cc(R.ncc, R.Lr);
        expect((long)cc.bytes(), R.lds_corr, "lds_corr");
        double* sc = cc.scratch(lds);
        check_spans("CcLds",
                    {span("za", lds, cc.za<Cplx>(lds), R.ncc, 16), span("zb", lds, cc.zb<Cplx>(lds), R.ncc, 16),
                     span("sy", lds, cc.sy(lds), R.Lr + 1), span("red", lds, sc + CcLds::RED, 8), span("val", lds, sc + CcLds::VAL, 4),
                     span("scan", lds, sc + CcLds::SCAN, 16), span("unused", lds, sc + CcLds::UNUSED, 4)},
                    (long)cc.bytes());
        // one-wave cross-correlation kernel
        const int plan = R.wave_r == 32 ? rsaf::wfft::Plan<32>::LDS_DOUBLES : rsaf::wfft::Plan<16>::LDS_DOUBLES;
        const CcWaveLds ccw(plan, R.Lr);
        expect(ccw.sy_doubles, R.cc_wave_sy, "cc wave s_sy");
        expect((long)ccw.bytes(), (long)(plan + R.cc_wave_sy) * 8, "cc wave bytes");
        check_spans("CcWaveLds", {span("fft", lds, ccw.fft(lds), plan), span("sy", lds, ccw.sy(lds), R.Lr + 1)}, (long)ccw.bytes());
    }
    // workspace of a group of frames
    const int rstride = R.Lr + 2;
    expect((long)PitchWs::bytes_per_frame(rstride), R.ws_bytes_per_frame, "ws bytes/frame");
    const long frames = 7;
    const PitchWs ws(reinterpret_cast<double*>(lds), frames, rstride);
    check_spans("PitchWs",
                {span("rows", lds, ws.rows, frames * rstride), span("pc_a", lds, ws.pc_a, frames * PC_DOUBLES),
                 span("pc_b", lds, ws.pc_b, frames * PC_DOUBLES), span("hdr", lds, ws.hdr, frames, 4)},
                frames * (long)PitchWs::bytes_per_frame(rstride));
    // the frame record
    const FrameHdr* h = ws.hdr + 3;
    const char* hb = reinterpret_cast<const char*>(h);
    expect((long)sizeof(FrameHdr), 128, "sizeof(FrameHdr)");
    expect((long)(reinterpret_cast<const char*>(&h->flags) - hb), 0, "FrameHdr.flags");
    expect((long)(reinterpret_cast<const char*>(&h->n_a) - hb), 4, "FrameHdr.n_a");
    expect((long)(reinterpret_cast<const char*>(&h->n_b) - hb), 8, "FrameHdr.n_b");
    expect((long)(reinterpret_cast<const char*>(h->lag_a) - hb), 16, "FrameHdr.lag_a");
    expect((long)(reinterpret_cast<const char*>(h->lag_b) - hb), 48, "FrameHdr.lag_b");
    expect((long)(reinterpret_cast<const char*>(h->a_slot_of_b) - hb), 80, "FrameHdr.a_slot_of_b");
    expect((long)(reinterpret_cast<const char*>(FrameHdr::at(reinterpret_cast<const int*>(ws.hdr), 3)) - hb), 0, "FrameHdr::at");
    std::printf("ok %s\n", R.name);
}

int main() {
    for (const Row& R : ROWS) check_row(R);
    return 0;
}
