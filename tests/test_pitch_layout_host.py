"""csrc/mshds_pitch_layout.h checked on the host (tests/host/pitch_layout_replay.cpp): the LDS carve-ups of the MSHDS
pitch kernels, the frame record and the workspace layout, at the geometries of the feature scripts' analyses.  The replay
asserts the sizes the launches request, that every array lies inside its request, that no two arrays overlap, the
alignments, and the byte positions of the frame record's fields."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pitch_layout_replay(tmp_path):
    exe = str(tmp_path / "pitch_layout_replay")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "robust_speech_analysis_framework_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "pitch_layout_replay.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(lines) == 10 and all(l.startswith("ok ") for l in lines), r.stdout
