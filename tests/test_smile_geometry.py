"""``rsaf_smile_geometry`` / ``rsaf_smile_n_frames`` against ``smile_oracle.Params`` at EVERY integer sample rate the ABI
could be handed around its accepted range (host-only calls, no GPU): the same (frame, hop, nfft) or a refusal, and a refusal
exactly where the contract says (include/rsaf.h: [4000, 65536] Hz and a 25 ms frame that fits a 256 ... 2 048-point transform)."""
import ctypes as C

from oracle import smile_oracle as so

FS_LO, FS_HI = 3990, 65546


def test_geometry_of_every_rate_matches_the_oracle_or_is_refused(rsaf_lib):
    fr, hp, nf = C.c_int(0), C.c_int(0), C.c_int(0)
    accepted, nffts = 0, set()
    for fs in range(FS_LO, FS_HI + 1):
        P = so.Params(fs)
        ok = 4000 <= fs <= 65536 and 256 <= P.nfft <= 2048
        rc = rsaf_lib.rsaf_smile_geometry(fs, C.byref(fr), C.byref(hp), C.byref(nf))
        assert (rc == 0) == ok, (fs, rc)
        sizes = (0, P.frame - 1, P.frame, P.frame + P.hop - 1, P.frame + P.hop, P.frame + 16 * P.hop)
        if ok:
            assert (fr.value, hp.value, nf.value) == (P.frame, P.hop, P.nfft), fs
            for n in sizes:
                assert rsaf_lib.rsaf_smile_n_frames(n, fs) == P.n_frames(n), (fs, n)
            accepted += 1
            nffts.add(P.nfft)
        else:
            for n in sizes:
                assert rsaf_lib.rsaf_smile_n_frames(n, fs) == -1, (fs, n)
    # the refused rates inside [4000, 65536] are those whose frame is shorter than 129 samples (a 128-point transform):
    # 0.025 fs + 0.5 < 129 <=> fs < 5140
    assert accepted == 65536 - 5140 + 1 and nffts == {256, 512, 1024, 2048}
    assert rsaf_lib.rsaf_smile_geometry(5140, C.byref(fr), C.byref(hp), C.byref(nf)) == 0 and (fr.value, nf.value) == (129, 256)
    assert rsaf_lib.rsaf_smile_geometry(5139, C.byref(fr), C.byref(hp), C.byref(nf)) != 0
    assert b"unsupported frame length" in rsaf_lib.rsaf_last_error()
    assert rsaf_lib.rsaf_smile_geometry(65537, C.byref(fr), C.byref(hp), C.byref(nf)) != 0
    assert b"[4000, 65536]" in rsaf_lib.rsaf_last_error()
