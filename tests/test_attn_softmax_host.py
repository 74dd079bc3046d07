"""csrc/attn_softmax.h replayed on the host (tests/host/attn_softmax_replay.cpp), no GPU.

arithmetic: the softmax of attn_f16x3_kernel as it runs now (row maximum on the raw accumulators, e = 2^((s - m) c) with
c = scale log2(e) as one float constant, e 2^14 split into two fp16, 1 / sum applied to the output) against the form before
it (expf(s scale - m scale), p 2^14 split), both against the float64 softmax.  v_exp_f32 is modelled as float64 exp2 rounded
to float (the instruction is within 1 ulp of that); the library expf likewise.  Sweep: score gaps from 0 to 133 (exp
underflows at 87.3, with denormals at 103.3), scale from 2^-20 to 2^4, row sums from 1 to 256, row maxima from -3.3 to 60.
Condition: the worst |p - p64| of the new form over the sweep (the relative error weighted by the probability itself) is at
most 1.25 x the worst of the form before.  Both forms are deterministic, so the margin only admits a reshuffled rounding; a
lost low plane or a truncated constant shows as 2^11 x or more.  (Folding the 2^14 into the exponent's argument as + 14
fails this at 3.45 x: the argument is then rounded to 2^-21 absolutely.)

layout: the store map of a wave's 32 x 64 output after the exchange of the wave's halves (every (query, column, plane)
written exactly once, 16-byte aligned stores that cover 1 KB of a panel without a gap per instruction), every address of
the transposed V reads inside the staged block, equal to the per-step form of the kernel before and conflict-free, and the
walk of the workgroups (every (window x head, query half) visited once, the two halves 8 ids apart).  The kernel stages
nothing through LDS for its stores, so there is no LDS patch whose addresses could leave a block."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attn") / "attn_softmax_replay")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "robust_speech_analysis_framework_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "attn_softmax_replay.cpp"), "-o", exe], check=True)
    return exe


def test_new_softmax_form_is_as_close_to_float64_as_the_form_before(replay):
    r = subprocess.run([replay, "arithmetic"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok arithmetic" and sum(l.startswith("sscale 2^") for l in lines) == 25
    worst = [l for l in lines if l.startswith("worst over the sweep")][0].split()
    parent, new = float(worst[worst.index("parent") + 1]), float(worst[worst.index("new") + 1])
    assert 0 < parent < 1e-6 and new <= 1.25 * parent


def test_store_map_reads_and_workgroup_walk(replay):
    r = subprocess.run([replay, "layout"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 3 and all(l.startswith("ok ") for l in lines), r.stdout
