"""csrc/w2v2_layout.h checked on the host (tests/host/w2v2_layout_replay.cpp): the weight layout, the workspace, the window
geometry, the path predicates and the dynamic-LDS layouts of the Wav2Vec2 forward, at seven geometries (the published
families and two small test geometries) crossed with four window sets.  The replay compares totals, offsets and workspace
sizes with the numbers recorded from the library before csrc/w2v2.hip was split, and asserts bounds, overlap and alignment
of every segment, the fit of the packed row tables, Rag against a recomputation, the LDS requests and the predicates.

A second run (`regimes`) sweeps non-increasing window lists with frame counts either side of 256, 512 and 513 at head widths
64 and 16, with and without POS_CONV_STACK: the regime runs that a ragged call is split into (window_regime, regime_runs)
partition the list in order, each is uniform under the path predicates, and none needs more workspace than the call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "w2v2_layout_replay")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "robust_speech_analysis_framework_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "w2v2_layout_replay.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_w2v2_layout_replay(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(lines) == 7 * 4 + 1 and all(l.startswith("ok ") for l in lines), r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_regime_runs_partition_a_call_and_fit_its_workspace(tmp_path):
    r = subprocess.run([_build(tmp_path), "regimes"], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(lines) == 8 and all(l.startswith("ok regimes ") for l in lines), r.stdout
