"""The constructed cases of tests/smile_stage_cases.py reach what they claim - checked on the oracle alone, so that
tests/test_smile_rates_gpu.py and tests/test_smile_pitch_tail_gpu.py cannot pass vacuously."""
import math

import numpy as np
import pytest

from oracle import smile_oracle as so
import smile_stage_cases as sc

LOG_HNR_LO = math.log(1e-3 / (1.0 - 1e-3))
LOG_HNR_HI = math.log((1.0 - 1e-6) / 1e-6)               # 13.8155


def test_rate_list_geometries():
    assert sorted(sc.RATES) == [5160, 10240, 10280, 11025, 12000, 20480, 20520, 24000, 32000, 40960, 41000, 65536]
    for fs, (frame, hop, nfft) in sc.RATES.items():
        P = so.Params(fs)
        assert (P.frame, P.hop, P.nfft) == (frame, hop, nfft), fs
    full = [fs for fs, (fr, _, nf) in sc.RATES.items() if fr == nf]
    half = [fs for fs, (fr, _, nf) in sc.RATES.items() if fr == nf // 2 + 1]
    assert full == [10240, 20480, 40960] and half == [5160, 10280, 20520, 41000]
    assert {nf for _, _, nf in sc.RATES.values()} == {256, 512, 1024, 2048}          # all four template instances


@pytest.mark.parametrize("fs", sorted(sc.RATES))
def test_frame_cases_are_voiced_and_finite(fs):
    P = so.Params(fs)
    clips = sc.frame_clips(fs)
    frames = [P.n_frames(len(c)) for c in clips]
    assert tuple(frames[3:]) == sc.FRAME_CLIP_FRAMES_TAIL
    voiced = 0
    for c, nf in zip(clips[:3], frames[:3]):              # the four cuts are prefixes of a voiced clip: same code, fewer frames
        r = so.lld(c, P)
        assert r.shape == (so.NLLD, nf) and np.isfinite(r).all()
        voiced += int((r[so.I_F0] > 0).sum())
    assert voiced >= 0.05 * sum(frames)
    first = so.lld(clips[0], P)[so.I_F0]
    assert (first > 0).mean() >= 0.4                      # measured 46 - 100 % over the twelve rates


def test_viterbi_cases_reach_both_decisions():
    calls = sc.viterbi_cases()
    assert sorted(calls) == ["random", "structured"]
    for kind, cases in calls.items():
        assert [c.T for c in cases] == list(sc.VIT_LENGTHS) and cases[len(cases) // 2].T == 0
        for c in cases:
            F, V = c.expected()
            assert c.cand.shape == (c.T, 6, 2) and F.shape == (c.T,)
            if c.mixed:
                assert (F > 0).any() and (F == 0).any(), c.name
            if c.T >= 29:                                     # all three gate values on frames that would otherwise be non-zero
                F0, V0 = so.viterbi_smooth(c.cand3())
                for g in sc.GATE_RMS:
                    assert ((c.rms == g) & (V0 > 0)).any(), (c.name, g)
                assert (V[c.rms == sc.GATE_RMS[0]] == 0).all() and (V[c.rms == sc.GATE_RMS[1]] == V0[c.rms == sc.GATE_RMS[1]]).all()
    rnd = np.concatenate([c.cand.reshape(-1, 2) for c in calls["random"]])
    frames_without = np.concatenate([(c.cand[:, :, 0] > 0).sum(axis=1) == 0 for c in calls["random"] if c.T])
    assert 0.55 < (rnd[:, 0] > 0).mean() / (1.0 - frames_without.mean()) < 0.65 and 0.05 < frames_without.mean() < 0.2
    f = rnd[rnd[:, 0] > 0, 0]
    assert f.min() >= 52.0 and f.max() <= 620.0 and f.min() < 60.0 and f.max() > 550.0


def test_structured_contour_decides_what_its_comments_say():
    """The exact ties, the voicing edges and the lag-tuned stretches of the structured contour, read off the oracle."""
    # log2 differences of the octave alternatives are exact integers: both competitors of a tie cost the same to the bit
    for f in (64.0, 128.0, 55.0, 110.0):
        assert np.log2(2.0 * f) - np.log2(f) == 1.0
    c = [v for v in sc.viterbi_cases()["structured"] if v.T == 193][0]
    F, V = so.viterbi_smooth(c.cand3())
    # block 1 (frames 0-3): predecessor tie -> slot 1 (256 Hz), the lowest index, not slot 4 (64 Hz)
    assert list(F[:4]) == [256.0, 128.0, 128.0, 0.0]
    # block 2 (4-13): voicing exactly 0.7 over 8 frames stays voiced (no threshold penalty at the cut-off itself)
    assert (F[4:12] == 210.0).all() and (V[4:12] == 0.7).all() and (F[12:14] == 0).all()
    # block 3 (14-19): the duplicated candidate; block 4 (20-23): below the clamp -> unvoiced, v_best reported
    assert (F[14:19] == 300.0).all() and (F[20:24] == 0).all() and list(V[20:24]) == [5e-4, 5e-4, 5e-4, 0.0]
    # block 5 (24-55): a stretch of exactly 30: the fixed lag of 30 frames voices its FIRST frame only (one frame earlier the
    # best path ending 28 frames on is still unvoiced; one frame later the forced exit is in view)
    assert F[24] == 100.0 and V[24] == sc.LAG_V and (F[25:56] == 0).all()
    # block 6 (56-60): 55 / 220 Hz in front of 110 Hz tie exactly -> slot 0 (220 Hz)
    assert list(F[56:61]) == [220.0, 110.0, 110.0, 110.0, 0.0]
    # block 7 (61-93): a stretch of 31: its first two frames
    assert (F[61:63] == 100.0).all() and (F[63:94] == 0).all()
    # the clip's end: the best end state ties between slot 2 (256 Hz) and slot 5 (64 Hz) -> the lowest state
    assert list(F[-3:]) == [0.0, 128.0, 256.0]
    # the tuning of LAG_V: 29 frames of advantage do not pay the entry, 30 do
    a = -2.0 * math.log(sc.LAG_V) + 4.0
    b = -2.0 * math.log(1.0 - 0.7) + 4.0
    assert sc.LAG_V < 0.7 and 29 * (b - a) < 10.0 < 30 * (b - a)


def test_jitter_cases_reach_their_lag_ranges():
    cases = sc.jitter_cases()
    assert sorted(cases) == [5160, 8000, 16000, 48000, 65536]
    geo = {}
    for fs, lst in cases.items():
        P = so.Params(fs)
        for c in lst:
            v = c.f0 > 0
            assert v.any() and c.f0[v].min() >= 52.0 and c.f0[v].max() <= 620.0          # CCMAX and WCAP never bind
            nl_max, nl_min, span = c.lag_geometry()
            assert nl_max <= 1024 and span <= 4096
            geo[c.name] = (nl_max, nl_min, span)
            # single-candidate contours at voicing 0.9: the Viterbi pass and the gate return the contour itself
            F, V = so.energy_gate(*so.viterbi_smooth(c.cand3()), c.rms())
            assert np.array_equal(F, c.f0) and np.array_equal(V, np.where(v, sc.JIT_VOICING, 0.0)), c.name
            assert all(e - s >= 3 for s, e in c.runs())
    assert geo["low F0 52-56 Hz at 65536"][0] >= 630 and geo["low F0 52-56 Hz at 65536"][2] >= 2830
    assert geo["low F0 52-56 Hz at 48000"][0] > 448 and geo["low F0 52-56 Hz at 16000"][0] > 128
    assert geo["110 Hz at 16000"][0] == 72                       # 64 < NL <= 128: two lag passes
    assert geo["600-620 Hz at 5160"][1] == 4 and geo["600-620 Hz at 8000"][0] <= 8
    by = {c.name: c for c in cases[16000]}
    for tag, starts in (("A", (63, 128)), ("B", (64, 126))):
        c = by[f"12 runs {tag}"]
        runs = c.runs()
        assert len(runs) == 12 and len({e - s for s, e in runs}) == 12 and runs[-1][1] == len(c.f0) == 218
        assert set(starts) <= {s for s, _ in runs}
        assert any(s < 64 < e for s, e in runs) or any(s == 64 for s, _ in runs)
    off = by["110 Hz contour over a 91 Hz tone"]               # the first period's best lag: index >= 64 of the 72 lags 110 .. 181
    x = off.wav.astype(np.float64)
    cc = [np.dot(x[:145], x[t:t + 145]) / math.sqrt(np.dot(x[:145], x[:145]) * np.dot(x[t:t + 145], x[t:t + 145])) for t in range(110, 182)]
    assert geo[off.name][0] == 72 and 64 <= int(np.argmax(cc)) < 71
    st = by["steps 200 / 400 Hz"]
    assert len(st.runs()) == 1 and set(st.f0) == {200.0, 400.0} and (np.diff(st.f0) != 0).sum() >= 15


def test_jitter_cases_oracle_values_are_informative():
    for fs, lst in sc.jitter_cases().items():
        P = so.Params(fs)
        for c in lst:
            J = so.jitter_shimmer(c.wav, c.f0, P)
            v = c.f0 > 0
            assert np.isfinite(J).all() and (J[:, ~v] == 0).all()
            if c.mid:
                assert (J[0, v] > 0).mean() >= 0.5, c.name                               # jitterLocal carries
                assert ((J[3, v] > LOG_HNR_LO) & (J[3, v] < LOG_HNR_HI)).mean() >= 0.5, c.name
            if c.name.startswith("low F0"):
                assert (J[2, v] > 0).mean() >= 0.5 and ((J[3, v] > LOG_HNR_LO) & (J[3, v] < LOG_HNR_HI)).mean() >= 0.5, c.name
                # the period chain dies before the clip ends: the last frames repeat the values of the one before
                assert np.array_equal(J[:, -1], J[:, -2])
            if c.name == "DC waveform":
                assert (J[:3, v] == 0).all() and np.allclose(J[3, v], LOG_HNR_HI, rtol=0, atol=1e-8)
            if c.name == "all-zero waveform":
                assert (J[:3, v] == 0).all() and np.allclose(J[3, v], LOG_HNR_LO, rtol=0, atol=1e-12)
