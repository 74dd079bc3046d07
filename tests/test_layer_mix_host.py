"""csrc/layer_mix_layout.h replayed on the host (tests/host/layer_mix_replay.cpp): the partition of the layer mix's backward
puts every position into exactly one part (ragged last part, fewer positions than one part, the part count at its cap),
h is addressed one to one, and the sums in the stated order stay within 2^-24 |dp64| + 2 n 2^-53 sum|h dx| of a long double
sum.  The second test asks the built library's host-only size entries (``rsaf_layer_mix_partials``,
``rsaf_cnnlstm_train_dx_scratch_floats``) for the rows the replay printed from the headers, so that header and ABI cannot
part, and checks the codes they and the launching entries give for bad arguments (all refused before any launch)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from cnnlstm_geometry import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RSAF_ERR_ARG, RSAF_ERR_WORKSPACE = 1, 3


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("layer_mix") / "layer_mix_replay")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "robust_speech_analysis_framework_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "layer_mix_replay.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [l.split() for l in r.stdout.splitlines() if l.strip()]


def test_layer_mix_replay(replay):
    mix = [l for l in replay if l[0] == "ok"]
    dx = [l for l in replay if l[0] == "dx"]
    assert len(mix) == 9 and len(dx) == 13 and len(replay) == 22, replay
    parts = {tuple(map(int, l[1:5])): int(l[5]) for l in mix}
    assert parts[(2, 13, 5, 20)] == 1 and parts[(1, 3, 4099, 4)] == 2 and parts[(2, 25, 37, 768)] == 4
    assert parts[(4, 13, 20000, 768)] == 2048 and parts[(4, 13, 4378, 768)] == 821
    assert {(int(l[1]), int(l[2])) for l in dx} >= {(c[0], c[1]) for c in CASES}


def test_library_size_entries_match_the_headers(replay, rsaf_lib):
    for l in replay:
        if l[0] == "ok":
            B, L, T, D, parts, per, n = map(int, l[1:])
            assert n == parts * L and parts * per >= B * T * D // 4 > (parts - 1) * per
            assert rsaf_lib.rsaf_layer_mix_partials(B, L, T, D) == n, l
        else:
            D, Cc, n = map(int, l[1:])
            assert n == (D * 3 * Cc + 3) // 4 * 4
            assert rsaf_lib.rsaf_cnnlstm_train_dx_scratch_floats(D, Cc) == n, l


def test_bad_arguments_give_the_documented_codes(rsaf_lib):
    lib = rsaf_lib
    for bad in ((1, 0, 4, 8), (1, 33, 4, 8), (0, 2, 4, 8), (1, 2, 0, 8), (1, 2, 4, 6), (1, 2, 4, 0), (1 << 14, 2, 1 << 16, 1 << 10)):
        assert lib.rsaf_layer_mix_partials(*bad) == -1, bad
    assert lib.rsaf_layer_mix_partials(1, 32, 1, 4) == 32
    for bad in ((6, 8), (8, 6), (0, 8), (8, 0), (8, 1028), (-4, 8)):
        assert lib.rsaf_cnnlstm_train_dx_scratch_floats(*bad) == -1, bad
    assert lib.rsaf_cnnlstm_train_dx_scratch_floats(768, 1024) == 768 * 3 * 1024
    # the launching entries refuse these before they touch the device: host memory stands in for the operands
    buf = (C.c_float * 72)()
    dbl = (C.c_double * 72)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)          # 16-byte aligned, as the entries ask of h, x and dx
    q = C.c_void_p((C.addressof(dbl) + 15) & ~15)
    assert lib.rsaf_layer_mix_forward(p, 1, 33, 2, 4, p, p, None) == RSAF_ERR_ARG
    assert b"RSAF_LAYER_MIX_MAX" in lib.rsaf_last_error()
    assert lib.rsaf_layer_mix_forward(p, 1, 2, 2, 6, p, p, None) == RSAF_ERR_ARG
    assert lib.rsaf_layer_mix_forward(None, 1, 2, 2, 4, p, p, None) == RSAF_ERR_ARG
    assert lib.rsaf_layer_mix_backward(p, p, 1, 2, 2, 4, None, 64, p, None) == RSAF_ERR_ARG
    assert lib.rsaf_layer_mix_backward(p, p, 1, 2, 2, 4, q, 1, p, None) == RSAF_ERR_WORKSPACE
    assert b"rsaf_layer_mix_partials" in lib.rsaf_last_error()
