// csrc/mshds_cpp_layout.h on the host: the layouts and the integer-deciding arithmetic of the cepstral-peak-prominence
// chain.  Modes (argv[1]):
//   self    sizes and field offsets of Seg and ClipHdr, find_seg on each of its three fields against a linear scan,
//           the frame list carved from the work buffer, moving_average_range against a brute-force restatement.
//           Prints "ok <check>" per check; exit status 1 on the first failure.
//   round6  reads one double per line (any strtod form), prints round6 of it with %a.
//   geom    reads "tmin tmax clip_x1 pitch_floor" per line, prints
//           "verdict ix1 m_in m_out nf nx nfft lg x1_seg x1o t1 window" (verdict 0 ok, 1 skip, 2 fail; doubles with %a).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mshds_cpp_layout.h"

using namespace rsaf::mshds_cpp;

static void fail(const std::string& what) {
    std::printf("FAIL %s\n", what.c_str());
    std::exit(1);
}
static void expect(long long got, long long want, const std::string& what) {
    if (got != want) fail(what + ": " + std::to_string(got) + ", expected " + std::to_string(want));
}

static void check_sizes() {
    expect(sizeof(Seg), 120, "sizeof(Seg)");
    expect(SEG_DOUBLES, 15, "SEG_DOUBLES");
    const size_t offs[] = {offsetof(Seg, ix1), offsetof(Seg, m_in), offsetof(Seg, m_out), offsetof(Seg, res_off),
                           offsetof(Seg, frame_off), offsetof(Seg, nf), offsetof(Seg, x1_seg), offsetof(Seg, x1o),
                           offsetof(Seg, window), offsetof(Seg, t1), offsetof(Seg, nx), offsetof(Seg, nfft),
                           offsetof(Seg, work_off), offsetof(Seg, item_off), offsetof(Seg, lg)};
    for (int i = 0; i < 15; ++i) expect((long long)offs[i], 8 * i, "offset of Seg field " + std::to_string(i));
    expect(sizeof(ClipHdr), 16, "sizeof(ClipHdr)");
    int hdr[12];
    for (int i = 0; i < 12; ++i) hdr[i] = 100 + i;
    const ClipHdr* h = ClipHdr::at(hdr, 2);
    expect(h->n_seg, 108, "ClipHdr.n_seg");
    expect(h->fail, 109, "ClipHdr.fail");
    expect(h->total_frames, 110, "ClipHdr.total_frames");
    expect(h->total_resampled, 111, "ClipHdr.total_resampled");
    std::printf("ok sizes\n");
}

// the owner of element g by a linear scan: the last segment whose offset is <= g (the first one when none is)
template <double Seg::*F>
static int linear_owner(const std::vector<Seg>& s, int g) {
    int k = 0;
    for (int i = 1; i < (int)s.size(); ++i)
        if ((int)(s[i].*F) <= g) k = i;
    return k;
}

template <double Seg::*F>
static void check_find_seg_field(const char* field) {
    unsigned rng = 12345u;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return (rng >> 8) & 0xffff; };
    for (int n : {1, 2, 7, 64}) {
        for (int trial = 0; trial < 8; ++trial) {
            std::vector<Seg> s(n);
            std::memset(s.data(), 0, sizeof(Seg) * n);
            int off = 0;
            for (int i = 0; i < n; ++i) {
                s[i].*F = (double)off;
                // every third trial keeps equal neighbouring offsets (zero-length ranges), also at the end of the table
                const int len = (trial % 3 == 0 && (i % 2 == 1 || i == n - 2)) ? 0 : 1 + (int)(next() % 37);
                off += len;
            }
            for (int g = 0; g <= off + 2; ++g) {
                const int got = find_seg<F>(s.data(), n, g), want = linear_owner<F>(s, g);
                if (got != want)
                    fail(std::string("find_seg<") + field + ">: n " + std::to_string(n) + " trial " + std::to_string(trial) + " g " +
                         std::to_string(g) + ": " + std::to_string(got) + ", linear scan " + std::to_string(want));
            }
            // the last element of the last segment
            expect(find_seg<F>(s.data(), n, off > 0 ? off - 1 : 0), linear_owner<F>(s, off > 0 ? off - 1 : 0), "last element");
        }
    }
    std::printf("ok find_seg %s\n", field);
}

static void check_frame_list() {
    struct Case { int n_clips; long long cap_work; };
    const Case cases[] = {{1, 1024}, {48, 482000}, {65535, 70000000}};      // the last: 2 * n * cap_work - 1 overflows int
    for (const Case& c : cases) {
        const long long lp_doubles = (long long)c.n_clips * c.cap_work * 2;
        char* base = reinterpret_cast<char*>(0x1000);                         // never dereferenced
        const FrameList l(base, c.n_clips, c.cap_work);
        const std::string at = " at (" + std::to_string(c.n_clips) + ", " + std::to_string(c.cap_work) + ")";
        const long long want_cap = lp_doubles - 1 < 0x7fffffffLL ? lp_doubles - 1 : 0x7fffffffLL;     // the parent's expression
        expect(l.cap, want_cap, "FrameList.cap" + at);
        expect(reinterpret_cast<char*>(l.entries) - base, 0, "FrameList.entries" + at);
        const long long count_at = reinterpret_cast<char*>(l.count) - base;
        expect(count_at, 8 * (lp_doubles - 1), "FrameList.count" + at);
        if (count_at % 4) fail("FrameList.count is not 4-byte aligned" + at);
        if (count_at < 8LL * l.cap) fail("FrameList.count lies inside the entries" + at);
        if (count_at + 4 > 8 * lp_doubles) fail("FrameList.count leaves the buffer" + at);
        // the planner's check: n_clips * cap_frames frames must fit
        if (!l.holds(l.cap) || l.holds((long long)l.cap + 1)) fail("FrameList.holds" + at);
    }
    {
        const FrameList l(reinterpret_cast<char*>(0x1000), 4, 1024);            // 8191 entries
        if (!l.holds(4LL * 2047) || l.holds(4LL * 2048)) fail("FrameList.holds(n_clips * cap_frames)");
    }
    std::printf("ok frame list\n");
}

static void check_moving_average_range() {
    for (int w = 1; w <= 12; ++w)
        for (int n = 1; n <= 20; ++n)
            for (int i = 0; i < n; ++i) {
                // brute force: the elements j of [0, n) with i - w/2 <= j <= i + w/2, without the last one for an even w
                int lo = -1, hi = -1;
                for (int j = 0; j < n; ++j) {
                    const bool in = j >= i - w / 2 && j <= i + w / 2 && !(w % 2 == 0 && j == i + w / 2);
                    if (in && lo < 0) lo = j;
                    if (in) hi = j;
                }
                int a, b;
                moving_average_range(i, w, n, &a, &b);
                if (a != lo || b != hi)
                    fail("moving_average_range(" + std::to_string(i) + ", " + std::to_string(w) + ", " + std::to_string(n) + "): [" +
                         std::to_string(a) + ", " + std::to_string(b) + "], brute force [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
            }
    std::printf("ok moving_average_range\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "self";
    char line[512];
    if (mode == "self") {
        check_sizes();
        check_find_seg_field<&Seg::res_off>("res_off");
        check_find_seg_field<&Seg::frame_off>("frame_off");
        check_find_seg_field<&Seg::item_off>("item_off");
        check_frame_list();
        check_moving_average_range();
    } else if (mode == "round6") {
        while (std::fgets(line, sizeof line, stdin)) std::printf("%a\n", round6(std::strtod(line, nullptr)));
    } else if (mode == "geom") {
        while (std::fgets(line, sizeof line, stdin)) {
            char* p = line;
            const double tmin = std::strtod(p, &p), tmax = std::strtod(p, &p), x1 = std::strtod(p, &p), floor_hz = std::strtod(p, &p);
            SegGeom g{};
            int v = 1;                                                          // tmin >= tmax: the kernel skips the interval
            if (tmin < tmax) v = seg_geometry(tmin, tmax, x1, floor_hz, &g) && !g.exceeds(26) ? 0 : 2;
            if (v != 0) g = SegGeom{};
            std::printf("%d %lld %lld %lld %lld %lld %d %d %a %a %a %a\n", v, (long long)g.ix1, (long long)g.m_in, (long long)g.m_out,
                        (long long)g.nf, (long long)g.nx, g.nfft, g.lg, g.x1_seg, v == 0 ? g.x1o() : 0.0, g.t1, g.window);
        }
    } else {
        return 2;
    }
    return 0;
}
