"""csrc/gemm_f16x3.h checked on the host (tests/host/gemm_tilewalk_replay.cpp): the tile walk of the persistent workgroups
(h3_grid_fill, h3_tile_at: 32-bit reciprocals) equals the 64-bit-division formula the kernel used before it
(tests/host/gemm_tilewalk_parent.inc, a verbatim copy) and is a bijection onto the tiles of every batch, on small grids
(every index) and on the ffn1 and conv1 grids of long runs (both ends and a strided sample); the running k-tile offset of
the DMA pointers (h3_kstep_next) equals the parent's koff(i, KT) for every k-tile, with and without tap panels."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gemm_tilewalk_replay(tmp_path):
    exe = str(tmp_path / "gemm_tilewalk_replay")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "robust_speech_analysis_framework_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "gemm_tilewalk_replay.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert r.returncode == 0, r.stdout + r.stderr
    # 13 named grids, 12 x 5 x 5 x 2 swept grids, the refused grid, the k-walks
    assert len(lines) == 13 + 600 + 1 + 1 and all(l.startswith("ok ") for l in lines), r.stdout
