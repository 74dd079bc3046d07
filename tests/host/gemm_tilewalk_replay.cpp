// csrc/gemm_f16x3.h on the host: the walk of the persistent workgroups over the tiles (h3_grid_fill, h3_tile_at) and the
// walk of a DMA source over the k-tiles (h3_kstep, h3_kstep_next) against the formulas the kernel used before them
// (gemm_tilewalk_parent.inc: 64-bit divisions per tile, KT * kstride per DMA instruction).
// Per grid: (1) the launcher's fill succeeds; (2) h3_tile_at equals the parent's lambda, for every tile index of a small
// grid, for the first and last 100 000 indices and a strided sample of a large one; (3) per batch the mapping is a
// bijection onto the tiles_m x tiles_n tiles (every index of the first, a middle and the last batch).
// Per k-walk: the running offset equals the parent's koff for every k-tile, in elements and in bytes.
// Prints "ok <row>" per row; exit status 1 on the first failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gemm_f16x3.h"
#include "gemm_tilewalk_parent.inc"

using namespace rsaf;

static std::string g_row;
static void fail(const std::string& what) {
    std::printf("FAIL %s: %s\n", g_row.c_str(), what.c_str());
    std::exit(1);
}

struct Grid { const char* name; int tiles_m, tiles_n, nz, nz2, group_m, bm, bn; };

static void check_tile(const GemmH3Params& p, const Grid& g, int64_t t) {
    const H3Tile T = h3_tile_at(p, (int)t);
    const ParentTile P = parent_tile_at(p, g.bm, g.bn, t);
    if ((int64_t)T.tm * g.bm != P.m0 || (int64_t)T.tn * g.bn != P.n0 || T.z != P.z || T.z1 != P.z1 || T.z2 != P.z2)
        fail("tile " + std::to_string(t) + ": (z, z1, z2, m0, n0) = (" + std::to_string(T.z) + ", " + std::to_string(T.z1) + ", " +
             std::to_string(T.z2) + ", " + std::to_string((int64_t)T.tm * g.bm) + ", " + std::to_string((int64_t)T.tn * g.bn) + "), the parent has (" +
             std::to_string(P.z) + ", " + std::to_string(P.z1) + ", " + std::to_string(P.z2) + ", " + std::to_string(P.m0) + ", " +
             std::to_string(P.n0) + ")");
}

static void check_grid(const Grid& g) {
    g_row = g.name;
    GemmH3Params p{};
    p.M = g.tiles_m * g.bm - (g.bm > 1 ? 1 : 0);             // the last row-tile and column-tile are partial
    p.N = g.tiles_n * g.bn - 16;
    if (p.N <= 0) p.N = 16;
    p.nz = g.nz; p.nz2 = g.nz2; p.group_m = g.group_m;
    if (!h3_grid_fill(p, g.bm, g.bn)) fail("h3_grid_fill refused the grid");
    if (p.tiles_m != g.tiles_m || p.tiles_n != g.tiles_n || p.nwg != g.tiles_m * g.tiles_n) fail("h3_grid_fill: wrong tile counts");
    const int64_t total = (int64_t)p.nwg * p.nz;
    if (total <= 400000) {
        for (int64_t t = 0; t < total; ++t) check_tile(p, g, t);
    } else {
        for (int64_t t = 0; t < 100000; ++t) check_tile(p, g, t);
        for (int64_t t = total - 100000; t < total; ++t) check_tile(p, g, t);
        for (int64_t t = 100000; t < total - 100000; t += 9973) check_tile(p, g, t);
    }
    const int batches[3] = {0, p.nz / 2, p.nz - 1};
    std::vector<char> seen((size_t)p.nwg);
    for (int b : batches) {
        std::fill(seen.begin(), seen.end(), 0);
        for (int o = 0; o < p.nwg; ++o) {
            const H3Tile T = h3_tile_at(p, (int)((int64_t)b * p.nwg + o));
            if (T.z != b) fail("batch " + std::to_string(b) + ": index " + std::to_string(o) + " lands in batch " + std::to_string(T.z));
            if (T.tm < 0 || T.tm >= p.tiles_m || T.tn < 0 || T.tn >= p.tiles_n) fail("batch " + std::to_string(b) + ": tile outside the grid");
            char& s = seen[(size_t)T.tm * p.tiles_n + T.tn];
            if (s) fail("batch " + std::to_string(b) + ": tile (" + std::to_string(T.tm) + ", " + std::to_string(T.tn) + ") is reached twice");
            s = 1;
        }
    }
    std::printf("ok %s\n", g.name);
}

// The k-walk of one operand: nkt k-tiles `kstride` elements apart, P tap panels (0: none)
static void check_kwalk(const char* name, int P, int nkt, int64_t kstride) {
    g_row = std::string(name) + " P=" + std::to_string(P) + " nkt=" + std::to_string(nkt) + " kstride=" + std::to_string(kstride);
    GemmH3Params p{};
    p.a_tap_panels = P;
    if (P > 0) p.a_tap_inv = 65536 / P + 1;                  // as the parent's launcher set it
    for (int unit = 1; unit <= 2; ++unit) {
        const H3KStep a = h3_kstep(kstride, P, unit), b = h3_kstep(kstride, 0, unit);
        int64_t offa = 0, offb = 0;
        int pca = 0, pcb = 0;
        for (int kt = 0; kt < nkt; ++kt) {
            if (offa != unit * parent_koff(p, true, kstride, kt)) fail("A, k-tile " + std::to_string(kt) + ": " + std::to_string(offa));
            if (offb != unit * parent_koff(p, false, kstride, kt)) fail("B, k-tile " + std::to_string(kt) + ": " + std::to_string(offb));
            if (P > 0 && pca != kt % P) fail("panel counter at k-tile " + std::to_string(kt));
            offa += h3_kstep_next(a, pca);
            offb += h3_kstep_next(b, pcb);
        }
    }
}

int main() {
    const Grid grids[] = {
        {"1x1x1 group_m 2", 1, 1, 1, 1, 2, 256, 256},
        {"nwg 6 (< 8)", 3, 2, 1, 1, 2, 256, 256},
        {"nwg 3, group_m 4 > tiles_m", 3, 1, 5, 1, 4, 512, 128},
        {"tiles_m 7 not a multiple of group_m 2", 7, 3, 2, 1, 2, 256, 256},
        {"tiles_m 11, group_m 3", 11, 5, 3, 1, 3, 256, 64},
        {"nz 32, nz2 16", 5, 1, 32, 16, 2, 256, 64},
        {"nz 48, nz2 16, 2 x 3 tiles", 2, 3, 48, 16, 2, 256, 256},
        {"nz 65535, 1 x 1 tiles", 1, 1, 65535, 1, 2, 256, 256},
        {"ffn1, 2 000 windows (1946 x 12)", 1946, 12, 1, 1, 2, 256, 256},
        {"ffn1 grid x 40 batches", 1946, 12, 40, 1, 2, 256, 256},
        {"conv1, 500-window group (15624 x 2)", 15624, 2, 1, 1, 2, 256, 256},
        {"conv1 grid x 24 batches, nz2 4", 15624, 2, 24, 4, 2, 256, 256},
        {"65535 batches of 32767 x 1 tiles (just below 2^31)", 32767, 1, 65535, 1, 2, 256, 64},
    };
    for (const Grid& g : grids) check_grid(g);
    // nwg % 8 = 0 .. 7 at every group size, tiles_m on both sides of group_m
    static char name[128];
    for (int tm = 1; tm <= 12; ++tm)
        for (int tn = 1; tn <= 5; ++tn)
            for (int gm : {1, 2, 3, 4, 8})
                for (int nz : {1, 3}) {
                    std::snprintf(name, sizeof name, "%d x %d tiles (nwg %% 8 = %d), group_m %d, nz %d", tm, tn, tm * tn % 8, gm, nz);
                    check_grid(Grid{name, tm, tn, nz, 1, gm, 256, 256});
                }
    // more than 2^31 - 1 tiles: refused
    {
        g_row = "2^31 tiles";
        GemmH3Params p{};
        p.M = 32768 * 256; p.N = 64; p.nz = 65536; p.group_m = 2;
        if (h3_grid_fill(p, 256, 64)) fail("h3_grid_fill accepted 2^31 tiles");
        std::printf("ok %s refused\n", g_row.c_str());
    }
    // the k-walks: no taps, P = 1, P = 48 with 3 taps (the CNN), and a few more; K / 16 up to 384; row-major (16) and panel strides
    const int64_t strides[] = {16, 16 * 1000, 16 * 499, (int64_t)16 * 3000000};
    for (int64_t ks : strides) {
        for (int nkt = 1; nkt <= 384; ++nkt) {
            check_kwalk("no taps", 0, nkt, ks);
            check_kwalk("taps", 1, nkt, ks);
            for (int P : {2, 3, 5, 24, 48, 128})
                if (nkt % P == 0) check_kwalk("taps", P, nkt, ks);
        }
        check_kwalk("the CNN's 3 taps x 48 panels", 48, 144, ks);
    }
    std::printf("ok k-walks\n");
    return 0;
}
