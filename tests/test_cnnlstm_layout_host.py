"""csrc/cnnlstm_layout.h checked on the host (tests/host/cnnlstm_layout_replay.cpp): the inference weight blob and workspace,
the training parameter blob, saved activations and scratch (with the sub-offsets of its `small` area) and the LDS of the
recurrence kernels, at the geometries of tests/cnnlstm_geometry.py, the shipped geometry, the training cap on C and a B T at
which the weight-gradient split doubles its chunk.  The replay compares totals and offsets with the numbers recorded from the
library before the layouts moved into the header (tests/host/cnnlstm_layout_parent.inc) and asserts bounds, overlap and
alignment of every segment; the second test asks the built library's size entries for the same rows, so that header and
ABI cannot part."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from cnnlstm_geometry import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "tests", "host", "cnnlstm_layout_parent.inc")
N_ROWS = 3 * len(CASES) + 2 + 1 + 1


def recorded_rows():
    """(name, D, C, H, NC, L, B, T, weight floats, weight offsets, workspace bytes, param floats, param offsets, saved, scratch)"""
    num = r"(-?\d+)"
    pat = re.compile(r'^\{"([^"]+)", ' + ", ".join([num] * 8) + r", \d+, \{([^}]*)\}, " + num + ", " + num + r", \d+, \{([^}]*)\}, "
                     + num + ", " + num + r"\},$")
    rows = []
    with open(INC) as f:
        for line in f:
            m = pat.match(line.strip())
            if m:
                g = m.groups()
                ints = lambda s: [int(v) for v in s.split(",")]                         # noqa: E731
                rows.append((g[0], *map(int, g[1:9]), ints(g[9]), int(g[10]), int(g[11]), ints(g[12]), int(g[13]), int(g[14])))
    return rows


def test_rows_cover_the_geometries():
    rows = recorded_rows()
    assert len(rows) == N_ROWS
    shapes = {r[1:8] for r in rows}
    for (D, Cc, H, _, NC, L, B, T) in CASES:
        for (b, t) in ((B, T), (1, 2), (17, 6)):
            assert (D, Cc, H, NC, L, b, t) in shapes
    assert (768, 128, 128, 2, 2, 4, 4378) in shapes and (768, 128, 128, 2, 2, 256, 1500) in shapes
    assert any(r[2] == 1024 for r in rows) and any(r[6] * r[7] > 4096 * 1024 for r in rows)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cnnlstm_layout_replay(tmp_path):
    exe = str(tmp_path / "cnnlstm_layout_replay")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "robust_speech_analysis_framework_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "cnnlstm_layout_replay.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(lines) == N_ROWS and all(l.startswith("ok ") for l in lines), r.stdout


def test_library_size_entries_match_the_recorded_rows():
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()

    def offsets(fn, *dims):
        buf, n = (C.c_int64 * 64)(), C.c_int(0)
        assert fn(*dims, buf, 64, C.byref(n)) == 0
        return list(buf[:n.value])

    for (name, D, Cc, H, NC, L, B, T, wf, wo, wsb, pf, po, sf, scf) in recorded_rows():
        assert lib.rsaf_cnnlstm_weight_floats(D, Cc, H, NC, L) == wf, name
        assert offsets(lib.rsaf_cnnlstm_weight_offsets, D, Cc, H, NC, L) == wo, name
        assert lib.rsaf_cnnlstm_workspace_bytes(B, T, D, Cc, H, L) == wsb, name
        assert lib.rsaf_cnnlstm_train_param_floats(D, Cc, H, NC, L) == pf, name
        assert offsets(lib.rsaf_cnnlstm_train_param_offsets, D, Cc, H, NC, L) == po, name
        assert lib.rsaf_cnnlstm_train_saved_floats(B, T, D, Cc, H, L) == sf, name
        assert lib.rsaf_cnnlstm_train_scratch_floats(B, T, D, Cc, H, L) == scf, name
