"""HIP openSMILE-style chain vs the CPU oracle (called through the C ABI).  Parity unpinned: the oracle is this
repository's restatement of the openSMILE components (no SMILExtract binary or recorded output exists here)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import smile_oracle as so

# parity metric of SURVEY.md §8d: per LLD row / feature column, max|gpu-cpu| / max|cpu|.  north_star's bar is 1e-4 for values
# and exact for indices; the chain is float64 on both sides since round 3, so the values agree far inside it and every
# decision (peak enhancement, candidate ranking, Viterbi path, jitter lags, roll-off bins, maxPos / minPos) must coincide.
TOL = 1e-4
TIGHT = 1e-9                   # what float64-vs-float64 actually delivers (different FFT / summation orders)


def _row(name):
    return so.LLD_NAMES.index(name)


ROLLOFF_ROWS = tuple(_row(f"pcm_fftMag_spectralRollOff{p}.0") for p in (25, 50, 75, 90))
F0, VOICING, JITTER_LOCAL, LOG_HNR = _row("F0final"), _row("voicingFinalUnclipped"), _row("jitterLocal"), _row("logHNR")
JITTER_ROWS = (JITTER_LOCAL, _row("jitterDDP"), _row("shimmerLocal"), LOG_HNR)
PITCH_ROWS = (F0, VOICING) + JITTER_ROWS


def _clips(seconds_list, first=0):
    from robust_speech_analysis_framework_amd import synth
    return [synth.synth_clip(first + i, s) for i, s in enumerate(seconds_list)]


def voiced_clip(seed, seconds, fs=16000, f0=None):
    """Speech-like test signal whose pitch the 25 ms SHS front end resolves (f0 200-320 Hz, 12 harmonics with a
    formant-like tilt, vibrato + 0.5 % period jitter, syllable envelope with pauses, noise at -40 dB); 16-bit quantised."""
    rng = np.random.default_rng(seed)
    n = int(seconds * fs)
    t = np.arange(n) / fs
    base = rng.uniform(200.0, 320.0) if f0 is None else f0
    inst = base * (1.0 + 0.06 * np.sin(2 * np.pi * rng.uniform(3.0, 6.0) * t + rng.uniform(0, 6.28)))
    inst = inst * (1.0 + 0.005 * rng.standard_normal(n).cumsum() / np.sqrt(np.arange(1, n + 1)))
    ph = 2 * np.pi * np.cumsum(inst) / fs
    y = np.zeros(n)
    for h in range(1, 13):
        if base * h * 1.1 < fs / 2:
            y += (1.0 / h) * (1.0 + 0.8 * np.exp(-((base * h - 900.0) / 400.0) ** 2)) * np.sin(h * ph + rng.uniform(0, 6.28))
    env = np.zeros(n)
    pos = rng.uniform(0.0, 0.2)
    while pos < seconds:
        dur = rng.uniform(0.18, 0.45)
        i0, i1 = int(pos * fs), min(n, int((pos + dur) * fs))
        if i1 > i0:
            m = i1 - i0
            env[i0:i1] = rng.uniform(0.5, 1.0) * np.sin(np.pi * np.arange(m) / m) ** 0.5
        pos += dur + (rng.uniform(0.15, 0.4) if rng.random() < 0.3 else 0.02)
    y = y * env
    y = y / (np.abs(y).max() + 1e-12) + 10 ** (-40 / 20) * rng.standard_normal(n)
    y = 0.5 * y / np.abs(y).max()
    return (np.round(y * 32767.0).astype(np.int16).astype(np.float32) / np.float32(32768.0))


def _run_gpu(clips, fs=16000):
    import torch
    from robust_speech_analysis_framework_amd import smile
    p = smile.pack_clips(clips, fs=fs)
    lld, octv, cand = smile.smile_lld(p, octave_spectrum=True, return_candidates=True)
    torch.cuda.synchronize()
    assert lld.dtype == torch.float64 and cand.dtype == torch.float64
    return p, lld.cpu().numpy(), octv.cpu().numpy(), cand.cpu().numpy()


def _check_rows(gpu, ref, P):
    """All 38 rows, end to end against the float64 oracle: values at TIGHT (<< north_star's 1e-4), roll-off bins and the
    voiced / unvoiced pattern exact."""
    assert not np.isnan(gpu).any()
    assert np.array_equal(gpu[F0] > 0, ref[F0] > 0)                    # the Viterbi path's voicing decisions
    for i in range(so.NLLD):
        scale = np.max(np.abs(ref[i])) + 1e-30
        err = np.abs(gpu[i] - ref[i])
        if i in ROLLOFF_ROWS:
            assert np.array_equal(gpu[i], ref[i]), so.LLD_NAMES[i]     # bin index * df: exact
        else:
            assert err.max() / scale <= TIGHT, (so.LLD_NAMES[i], err.max() / scale, int(np.argmax(err)))


def _check_pitch_chain(clips, p, g, octv, cand, P, min_voiced=0.05):
    """Diagnostic view of the pitch chain, stage by stage (each oracle stage fed with the GPU's output of the stage
    before), kept from the float32 era: it says WHERE a disagreement of _check_rows starts."""
    off = 0
    voiced_total = 0
    for c, nf in zip(clips, p.frames):
        if nf == 0:
            continue
        sl = slice(off, off + nf)
        _, _, mag = so.magnitudes(c, P)
        S_ref = np.stack([so.spec_scale(mag[t], P) for t in range(nf)])                # (a) cSpecScale
        scale = np.abs(S_ref).max(axis=1) + 1e-30
        err = np.abs(octv[sl] - S_ref).max(axis=1) / scale
        assert err.max() <= TIGHT, (err.max(), int(np.argmax(err)))
        ref_c = np.stack([so.shs_candidates(octv[off + t], P)[:, :2] for t in range(nf)])   # (b) cPitchShs
        got_c = cand[sl]
        assert np.array_equal(got_c[:, :, 0] > 0, ref_c[:, :, 0] > 0)
        assert np.abs(got_c - ref_c).max() <= TIGHT * 1000.0                             # f0 up to 620 Hz
        c3 = np.concatenate([got_c, (got_c[:, :, :1] > 0).astype(np.float64)], axis=2)
        F, V = so.viterbi_smooth(c3)                                                     # (c) Viterbi + energy gate
        F, V = so.energy_gate(F, V, g[0, sl])
        assert np.array_equal(g[F0, sl], F) and np.array_equal(g[VOICING, sl], V)             # same path, same candidates: bit-equal
        J = so.jitter_shimmer(c, g[F0, sl], P)                                           # (d) cPitchJitter
        for r, row in enumerate(JITTER_ROWS):
            sc = np.abs(J[r]).max() + 1e-30
            assert np.abs(g[row, sl] - J[r]).max() / sc <= TIGHT, so.LLD_NAMES[row]
        voiced_total += int((g[F0, sl] > 0).sum())
        off += nf
    assert voiced_total >= min_voiced * sum(p.frames)               # the chain was actually exercised


def test_lld_parity_ragged_batch(rsaf_lib):
    P = so.Params(16000)
    clips = _clips([5.0, 1.003, 0.025, 2.51, 0.0349]) + [voiced_clip(1, 2.2), voiced_clip(2, 0.61)]
    p, g, octv, cand = _run_gpu(clips)
    assert p.frames == [so.n_frames(len(c)) for c in clips]       # integer-exact frame counts
    ref = np.concatenate([so.lld(c) for c in clips], axis=1)
    assert g.shape == ref.shape
    _check_pitch_chain(clips, p, g, octv, cand, P)
    _check_rows(g, ref, P)


def test_lld_parity_30s_clip(rsaf_lib):
    P = so.Params(16000)
    clips = _clips([30.0], first=7) + [voiced_clip(3, 30.0)]
    p, g, octv, cand = _run_gpu(clips)
    assert p.frames == [2998, 2998]
    ref = np.concatenate([so.lld(c) for c in clips], axis=1)
    _check_pitch_chain(clips, p, g, octv, cand, P)
    _check_rows(g, ref, P)                                             # all 38 rows end to end, 30 s voiced clip included
    assert (ref[F0, 2998:] > 0).mean() > 0.3


@pytest.mark.parametrize("fs", [8000, 22050, 44100, 48000])
def test_native_sample_rates(rsaf_lib, fs):
    """SMILExtract analyses a file at its own rate (frame sizes are seconds, Androids.conf:73-78): FFT 256 / 1024 / 2048."""
    P = so.Params(fs)
    clips = [voiced_clip(10 + fs % 7, 1.3, fs=fs), voiced_clip(11, 0.4, fs=fs, f0=180.0),
             (0.1 * np.random.default_rng(fs).standard_normal(int(0.2 * fs))).astype(np.float32)]
    p, g, octv, cand = _run_gpu(clips, fs=fs)
    assert p.frames == [P.n_frames(len(c)) for c in clips]
    ref = np.concatenate([so.lld(c, P) for c in clips], axis=1)
    assert g.shape == ref.shape and octv.shape[1] == P.nbins
    _check_pitch_chain(clips, p, g, octv, cand, P)
    _check_rows(g, ref, P)


def _run_boundary_cases():
    """(fs, samples): clips whose LAST run of 16 frames is full (16 frames), or holds ONE frame whose flux needs the frame
    in front of the run (17 frames; 33: the same at the third run); at 8 and 48 kHz the 256- and 2 048-point instances
    take the one-frame path."""
    cases = [(16000, 2800), (16000, 2960), (16000, 5520)]
    for fs in (8000, 48000):
        P = so.Params(fs)
        cases.append((fs, P.frame + 16 * P.hop))
    return cases


@pytest.mark.parametrize("fs,n", _run_boundary_cases())
def test_run_boundaries(rsaf_lib, fs, n):
    P = so.Params(fs)
    clip = voiced_clip(30 + fs % 11, 1.0, fs=fs)[:n]
    assert len(clip) == n
    p, g, _, _ = _run_gpu([clip], fs=fs)
    assert p.frames == [P.n_frames(n)] and p.frames[0] in (16, 17, 33)
    ref = so.lld(clip, P)
    assert g.shape == ref.shape
    _check_rows(g, ref, P)


def test_known_answers_through_the_kernels(rsaf_lib):
    """Harmonic tone -> F0final at the tone (within the shift quantisation of the summation), voiced, jitter ~ 0;
    silence and white noise -> unvoiced, zeros."""
    fs = 16000
    t = np.arange(fs) / fs
    tone = sum((1.0 / h) * np.sin(2 * np.pi * 250.0 * h * t) for h in range(1, 11))
    tone = (0.3 * tone / np.abs(tone).max()).astype(np.float32)
    noise = (0.05 * np.random.default_rng(0).standard_normal(fs)).astype(np.float32)
    p, g, _, _ = _run_gpu([tone, np.zeros(fs // 2, np.float32), noise])
    a, b, c = p.frames
    F = g[F0, :a]
    assert (F > 0).mean() > 0.95 and 0.0 <= (np.median(F[F > 0]) - 250.0) / 250.0 < 0.025
    assert np.median(g[VOICING, :a]) > 0.7 and np.median(g[JITTER_LOCAL, :a]) < 1e-3 and np.median(g[LOG_HNR, :a]) > 5.0
    assert np.all(g[list(PITCH_ROWS), a:a + b] == 0.0)               # silence: gated by the energy selector
    assert (g[F0, a + b:] > 0).mean() < 0.05                          # noise: (almost) never voiced


def test_empty_and_too_short_inputs(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import smile
    p = smile.pack_clips([np.zeros(0, np.float32), np.zeros(399, np.float32)])
    assert p.frames == [0, 0]
    f = smile.smile_features(p)
    torch.cuda.synchronize()
    assert f.shape == (2, 912) and torch.isnan(f).all()
    p0 = smile.pack_clips([])
    assert smile.smile_features(p0).shape == (0, 912)


@pytest.mark.parametrize("window", [0, 3])
def test_functionals_exact_on_identical_input(rsaf_lib, window):
    """Functionals kernel vs oracle on the SAME (GPU-produced) LLD: positions bit-exact.  window = 3 is the literal
    reading of Androids.conf:355-356 (statistics of the first 25 ms window), 0 the adopted whole-file reading."""
    import torch
    from robust_speech_analysis_framework_amd import smile
    clips = _clips([5.0, 3.2, 0.05], first=20) + [voiced_clip(4, 4.0)]
    p = smile.pack_clips(clips)
    lld = smile.smile_lld(p)
    f = smile.smile_functionals(lld, p, window_frames=window)
    torch.cuda.synchronize()
    g = f.cpu().numpy()
    assert f.dtype == torch.float64 and np.isfinite(g).all()          # 912 / 912 columns, all 38 LLDs built
    names = so.feature_names()
    pos = np.array([n.endswith("Pos") for n in names])
    x_all = lld.cpu().numpy()
    off, refs = 0, []
    for nf in p.frames:
        refs.append(so.functionals(x_all[:, off:off + nf], window))
        off += nf
    ref = np.stack(refs)
    scale = np.max(np.abs(ref), axis=0) + 1e-30
    err = np.abs(g - ref).max(axis=0) / scale
    assert err[~pos].max() <= 1e-8, (names[int(np.argmax(np.where(~pos, err, 0)))], err[~pos].max())
    assert np.array_equal(g[:, pos], ref[:, pos])                      # maxPos / minPos: integer-exact
    if window:
        assert g[:, pos].max() <= window - 1


def _column_contours():
    """(LLD row, is_delta) of each of the 912 columns, in cCsvSink order (smile_oracle.functionals)."""
    rows, deltas = [], []
    for lo, hi in so.LEVELS:
        for de in (False, True):
            for i in range(lo, hi):
                rows += [i] * so.NFUNC
                deltas += [de] * so.NFUNC
    return rows, deltas


def _assert_all_912(g, ref, lld_ref=None):
    """``lld_ref`` (the oracle's [38, frames] LLD per row of ``ref``): a maxPos / minPos that differs is accepted when the
    ORACLE's own contour ties at the two positions to 1e-9 of its largest value.  That is structural for clips of three
    frames - the smoothed contour of x0, x1, x2 with edge replication is linear, so its delta regression is (d, 1.2 d, d)
    and the first and the last frame tie in exact arithmetic: the position is decided by the last bit on either side."""
    names = so.feature_names()
    assert g.shape == ref.shape and np.isfinite(g).all() and np.isfinite(ref).all()
    pos = np.array([n.endswith("Pos") for n in names])
    rows, deltas = _column_contours()
    bad = []
    for r, c in np.argwhere(g != ref):
        if not pos[c]:
            continue
        tie = False
        if lld_ref is not None:
            contour = so.sma3(lld_ref[r][rows[c]])
            contour = so.delta2(contour) if deltas[c] else contour
            tie = abs(contour[int(g[r, c])] - contour[int(ref[r, c])]) <= 1e-9 * np.max(np.abs(contour))
        if not tie:
            bad.append((int(r), names[c], g[r, c], ref[r, c]))
        else:
            g = g.copy()
            g[r, c] = ref[r, c]                       # accepted tie: out of the value comparison below
    assert not bad, bad[:8]
    # values: north_star's bar is 1e-4 of the column; float64 on both sides delivers ~1e-10.  Columns whose reference
    # value is a cancellation residue (a regression slope or skewness that is zero up to rounding) are measured against
    # the scale of their contour instead of against themselves
    scale = np.maximum(np.abs(ref), 1e-6 * np.max(np.abs(ref), axis=1, keepdims=True))
    err = np.abs(g - ref) / scale
    worst = np.unravel_index(int(np.argmax(err)), err.shape)
    assert err.max() <= TOL, (names[worst[1]], int(worst[0]), g[worst], ref[worst])
    col_scale = np.max(np.abs(ref), axis=0) + 1e-30
    assert (np.abs(g - ref).max(axis=0) / col_scale).max() <= 1e-7


def test_end_to_end_features_parity(rsaf_lib):
    """ALL 912 columns of every clip against the float64 oracle, end to end (no stage-wise feeding): a 30 s voiced clip,
    a 30 s synthetic-speech clip and a ragged batch; maxPos / minPos columns exact, everything else within 1e-4."""
    import torch
    from robust_speech_analysis_framework_amd import smile
    clips = [voiced_clip(5, 30.0)] + _clips([30.0], first=44) + _clips([5.0, 1.003, 2.51, 0.0349, 0.025], first=40) \
        + [voiced_clip(8, 2.2), voiced_clip(9, 0.61)]
    p = smile.pack_clips(clips)
    f = smile.smile_features(p)
    torch.cuda.synchronize()
    g = f.cpu().numpy()
    ref = np.stack(_oracle_pool(clips))
    _assert_all_912(g, ref)
    # the literal [functL1] reading (first 25 ms window) end to end as well
    f3 = smile.smile_features(p, window_frames=3)
    torch.cuda.synchronize()
    _assert_all_912(f3.cpu().numpy(), np.stack(_oracle_pool(clips, 3)))


def _oracle_extract(args):
    from oracle import smile_oracle
    c, window = args
    return smile_oracle.extract(c, window_frames=window)


def _oracle_pool(clips, window=0):
    """The Python-loop parts of the oracle (spline, Viterbi, jitter) take ~1 s per audio-second: one process per clip
    (spawned: the test process has initialised the GPU and must not fork)."""
    import concurrent.futures as cf
    import multiprocessing as mp
    with cf.ProcessPoolExecutor(max_workers=min(8, len(clips)), mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_oracle_extract, [(c, window) for c in clips]))


def test_dropin_dataframe_contract(rsaf_lib, tmp_path):
    import pandas as pd
    from robust_speech_analysis_framework_amd import smile, synth
    from src.utils import aggregate_clip_features
    paths = synth.write_synth_corpus(str(tmp_path), 3, 1.5)
    hi = str(tmp_path / "native_44k.wav")
    synth.write_wav(hi, np.round(voiced_clip(6, 0.8, fs=44100) * 32768.0).astype(np.int16), fs=44100)
    bad = tmp_path / "broken.wav"
    bad.write_bytes(b"not a wav")
    conf = tmp_path / "Androids.conf"
    conf.write_text(_MINI_CONF)
    df = pd.DataFrame({"filepath": [paths[0], str(bad), hi, paths[1], paths[2]]})
    out = smile.extract_opensmile_features(df, "/nonexistent/SMILExtract", str(conf), verbose=False)
    assert list(out.columns) == so.feature_names() + ["filename"]
    assert list(out["filename"]) == ["synth_00000.wav", "native_44k.wav", "synth_00001.wav", "synth_00002.wav"]
    vals = out[so.feature_names()].to_numpy(dtype=np.float64)
    assert np.isfinite(vals).all()                                      # no NaN column reaches the caller
    # the 44.1 kHz file went through the 2048-point chain at its own rate
    ref = so.extract(voiced_clip(6, 0.8, fs=44100), fs=44100)
    names = so.feature_names()
    _assert_all_912(vals[1:2], ref[None, :])                           # the whole row of the 44.1 kHz file, positions exact
    first = smile.extract_opensmile_features(df, "x", str(conf), verbose=False, functionals="first-window")
    assert first[[n for n in names if n.endswith("maxPos")]].to_numpy().max() <= 2.0
    # downstream of the drop-in in notebook 01: session aggregation must see finite numbers (SVM pipelines reject NaN)
    meta = pd.DataFrame({"filename": list(out["filename"]), "unique_participant_id": ["a", "a", "b", "b"]})
    agg = aggregate_clip_features(out, meta)
    num = agg.select_dtypes(include=[np.number]).to_numpy()
    mean_cols = [c for c in agg.columns if str(c).endswith("_mean")]
    assert np.isfinite(agg[mean_cols].to_numpy(dtype=np.float64)).all() and num.shape[0] == 2
    empty = smile.extract_opensmile_features(df, "x", str(tmp_path / "missing.conf"), verbose=False)
    assert empty.empty


_MINI_CONF = """
[fr1:cFramer]
frameSize=0.0250
frameStep = 0.010
[pe2:cVectorPreemphasis]
k=0.97
[w1:cWindower]
winFunc = ham
[mspec:cMelspec]
htkcompatible = 1
usePower = 0
lofreq = 20
hifreq = 8000
[mfcc:cMfcc]
firstMfcc = 1
lastMfcc =  12
[delta1:cDeltaRegression]
deltawin=2
[delta2:cDeltaRegression]
deltawin=2
[delta3:cDeltaRegression]
deltawin=2
[functL1:cFunctionals]
frameSize=0.025
frameStep=0
functionalsEnabled=Extremes;Regression;Moments
"""
