"""csrc/gn_stats.h replayed on the host (tests/host/gn_stats_replay.cpp), no GPU: GroupNorm's statistics as conv0_kernel's
statistics pass and gn_finalize_kernel form them (the per-slab float sums, their combination, the test whether they suffice,
the sums in double where they do not, the coefficients), driven over seeded channel sequences of conv0's output: input
DC + white noise at (DC, sd, conv bias) = (0, 1, 0), (0.05, 0.02, 0), (0.1, 0.01, 0), (0.3, 0.01, 0), (0.5, 0.002, 0),
(0, 1, 3), a constant sequence and an all-zero one, each at T0 = 143, 2127 and 8271 frames (one partial slab, five slabs,
seventeen; one empty slab appended, as a shorter window of a ragged call sees it), 32 channels each.

The figure of a sequence is max_t |a y_t + b - n_t| against the long double two-pass normalisation n_t.  Condition: per row
and T0 the worst channel's figure is within 4 x that of float32 two-pass statistics on the same sequences (worst channel
against worst channel: the replay's header says why not channel against channel), and the largest |y| is exact.  The replay
also prints the form before (float sum y and sum y^2 per slab, var = q / T0 - mean^2) as
the `parent` column, printed and not asserted: on every row with a DC offset at sd <= 0.01 it is 6 to 180 x the float32
two-pass's figure (with the conv bias at T0 = 143: 18 x), which the condition refuses."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_gn_stats_replay(tmp_path):
    exe = str(tmp_path / "gn_stats_replay")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "robust_speech_analysis_framework_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "gn_stats_replay.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    rows = [l for l in lines if l.startswith("row ")]
    assert lines[-1] == "ok gn_stats" and len(rows) == 8 * 3 and not any(l.startswith("FAIL") for l in lines)

    def col(line, name):
        w = line.split()
        return float(w[w.index(name) + 1])
    for l in rows:
        assert col(l, "new") <= 4.0 * col(l, "f32"), l
    outside = [l for l in rows if col(l, "parent") > 4.0 * col(l, "f32")]
    print(f"the form before is outside the bar on {len(outside)} of {len(rows)} rows (printed, not asserted)")
