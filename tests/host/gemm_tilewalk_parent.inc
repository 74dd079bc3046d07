// The tile walk and the k-tile offset of gemm_f16x3_kernel as they stood before the walk moved into csrc/gemm_f16x3.h
// (h3_tile_at, h3_kstep_next): the two lambdas of the kernel, verbatim, inside functions that give them the names they
// captured.  Kept as the parent that tests/host/gemm_tilewalk_replay.cpp compares the header against.
struct ParentTile { int m0, n0; int64_t z, z1, z2; };

static ParentTile parent_tile_at(const rsaf::GemmH3Params& p, int BM, int BN, int64_t t_in) {
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    const int nwg = tiles_n * tiles_m;
    struct Tile { int m0, n0, Mz; int64_t z, z1, z2, coff; };
    auto tile_at = [&](int64_t t) {
        Tile T;
        T.z = t / nwg;
        const int orig = (int)(t - T.z * nwg);
        T.z1 = p.nz2 > 1 ? T.z / p.nz2 : T.z;
        T.z2 = p.nz2 > 1 ? T.z % p.nz2 : 0;                              // (window, group) of a grouped convolution
        T.Mz = p.ztab ? (int)p.ztab[2 * T.z1] : p.M;                     // rows of this batch (ragged windows)
        T.coff = p.ztab ? p.ztab[2 * T.z1 + 1] : -1;
        const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
        const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
        const int GROUP_M = p.group_m;
        const int per_group = GROUP_M * tiles_n;
        const int grp = wg / per_group;
        const int first_m = grp * GROUP_M;
        const int gsz = (tiles_m - first_m) < GROUP_M ? (tiles_m - first_m) : GROUP_M;
        const int in_grp = wg - grp * per_group;
        T.m0 = (first_m + in_grp % gsz) * BM;
        T.n0 = (in_grp / gsz) * BN;
        return T;
    };
    const Tile T = tile_at(t_in);
    return ParentTile{T.m0, T.n0, T.z, T.z1, T.z2};
}

// element offset of k-tile KT of an A instruction (is_a) or a B instruction whose k-tiles lie kstride apart; a_tap_inv as
// the parent's launcher made it (65536 / P + 1, checked by it for every k-tile of the launch)
static int64_t parent_koff(const rsaf::GemmH3Params& p, bool is_a, int64_t kstride_i, int KT) {
    const int64_t kstride[1] = {kstride_i};
    const int i = 0;
    auto koff = [&](int i, int KT) -> int64_t {
        if (p.a_tap_panels > 0 && is_a) {
            const int tap = (int)(((unsigned)KT * (unsigned)p.a_tap_inv) >> 16);
            return (int64_t)(KT - tap * p.a_tap_panels) * kstride[i] + (int64_t)tap * 16;
        }
        return (int64_t)KT * kstride[i];
    };
    return koff(i, KT);
}
