"""csrc/smile_layout.h checked on the host (tests/host/smile_layout_replay.cpp): the LDS carve-up of the openSMILE-style
frame kernel at its four FFT lengths (sizes, containment, no overlap between regions live in the same phase, alignment), the
number of stash slots, and the LLD rows and functional levels of the header against their Python statements in smile.py
and oracle/smile_oracle.py (ctypes cannot read a header, so this test is what ties the two together)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("smile_layout") / "smile_layout_replay")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "robust_speech_analysis_framework_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "smile_layout_replay.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [l for l in r.stdout.splitlines() if l.strip()]


def test_lds_layout(replay):
    checks = [l for l in replay if not l.startswith(("row ", "level "))]
    assert len(checks) == 4 * 5 + 1 and all(l.startswith("ok ") for l in checks), "\n".join(checks)
    # the four requests, by value
    assert [l for l in checks if " bytes " in l] == ["ok 8 bytes 12096", "ok 9 bytes 12672", "ok 10 bytes 22144", "ok 11 bytes 40928"]


def test_rows_and_levels_match_python(replay):
    from oracle import smile_oracle
    from robust_speech_analysis_framework_amd import smile
    rows = [l.split(" ", 2) for l in replay if l.startswith("row ")]
    assert [int(r[1]) for r in rows] == list(range(smile.NLLD))
    names = [r[2] for r in rows]
    assert names == list(smile.LLD_NAMES)
    assert names == list(smile_oracle.LLD_NAMES)
    levels = [tuple(int(v) for v in l.split()[1:]) for l in replay if l.startswith("level ")]
    assert levels == [tuple(lv) for lv in smile._LEVELS]
    assert levels == [tuple(lv) for lv in smile_oracle.LEVELS]
