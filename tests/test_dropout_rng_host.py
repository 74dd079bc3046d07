"""csrc/dropout_rng.h compiled with g++ (tests/host/dropout_rng_replay.cpp), no GPU: the published Philox4x32-10 known
answers, the header's words and masks against the NumPy restatement of the mapping in include/rsaf.h
(tests/dropout_restatement.py) word for word, and the statistics of the restatement.  The generator is deterministic, so
the statistics are conditions on fixed numbers, not measurements: 72 of them, the worst at 2.2 sigma under a 5 sigma bar."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import dropout_restatement as dr  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

KNOWN_ANSWERS = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]
NS = (1, 3, 4, 5, 1023, 1025)
STEPS = (0, 1, 2 ** 32 + 7)
P = 0.37


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dropout_rng") / "dropout_rng_replay")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "robust_speech_analysis_framework_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "dropout_rng_replay.cpp"), "-o", exe], check=True)

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.splitlines()

    return run


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_published_known_answers(replay, counter, key, want):
    assert replay("kat", *counter.split(), *key.split()) == [want]
    got = dr.philox4x32_10([int(v, 16) for v in counter.split()], [int(v, 16) for v in key.split()])
    assert " ".join(f"{int(v):08x}" for v in got) == want


def _parse(line, tag):
    head, *vals = line.split()
    assert head == tag
    return np.array([int(v, 16) for v in vals], dtype=np.uint32)


def test_header_equals_restatement_word_for_word(replay):
    cases = [(seed, step, slot, n) for seed in dr.SEEDS for step in STEPS for slot in range(6) for n in NS]
    lines = replay(*[a for c in cases for a in (*c, repr(P))])
    assert len(lines) == 2 * len(cases)
    for i, (seed, step, slot, n) in enumerate(cases):
        what = f"seed {seed} step {step} slot {slot} n {n}"
        words, mask = _parse(lines[2 * i], "words"), _parse(lines[2 * i + 1], "mask")
        assert np.array_equal(words, dr.words(seed, step, slot, n)), what
        assert np.array_equal(mask, dr.mask(seed, step, slot, n, P).view(np.uint32)), what
        assert set(mask.tolist()) <= {0, int(dr.keep_value(P).view(np.uint32))}, what


def test_all_dropped_at_p_one_and_threshold_edges(replay):
    lines = replay(3, 1, 2, 9, 1.0, 3, 1, 2, 9, 1.5)
    assert not _parse(lines[1], "mask").any() and not _parse(lines[3], "mask").any()
    assert not dr.mask(3, 1, 2, 9, 1.0).any()
    assert dr.threshold(0.5) == 2 ** 31 and dr.threshold(0.2) == 858993459 and dr.threshold(1.0 - 2.0 ** -33) == 2 ** 32 - 1


@pytest.mark.parametrize("p", [0.2, 0.35, 0.5])
@pytest.mark.parametrize("seed", dr.SEEDS)
def test_statistics_of_the_restatement(seed, p):
    n = 65536
    thr = dr.threshold(p)
    q = 1.0 - thr / 2.0 ** 32                                 # exact keep probability of a uniform word
    agree = q * q + (1.0 - q) * (1.0 - q)                     # two independent masks agree on an element
    keep = lambda sd, step, slot: dr.words(sd, step, slot, n) >= np.uint32(thr)     # noqa: E731
    base = keep(seed, 1, 0)
    z = abs(base.mean() - q) / math.sqrt(q * (1.0 - q) / n)
    print(f"seed {seed} p {p}: keep fraction {base.mean():.5f} against {q:.5f}, {z:.2f} sigma")
    assert z <= 5.0
    others = {"neighbouring elements": (base[:-1], base[1:]), "slot 0 / slot 1": (base, keep(seed, 1, 1)),
              "slot 0 / slot 5": (base, keep(seed, 1, 5)), "step 1 / step 2": (base, keep(seed, 2, 0)),
              "seed / seed + 1": (base, keep(seed + 1, 1, 0))}
    for name, (a, b) in others.items():
        frac = (a == b).mean()
        z = abs(frac - agree) / math.sqrt(agree * (1.0 - agree) / len(a))
        print(f"seed {seed} p {p}: {name} agree on {frac:.5f} against {agree:.5f}, {z:.2f} sigma")
        assert z <= 5.0, name
