"""Constructed cases for the openSMILE-style chain: the frame geometries of tests/test_smile_rates_gpu.py and the candidate /
waveform cases that tests/test_smile_pitch_tail_gpu.py feeds to ``rsaf_smile_pitch_track`` directly.

Seeded numpy only (no torch, no GPU): tests/test_smile_stage_cases.py checks on the oracle alone that every case reaches what
its ``reach`` line says, so that the GPU tests cannot pass vacuously.  Every record is a small class with a ``name`` and a
``reach`` (what the case is there for, in the kernels' own terms).
"""
import functools
import math

import numpy as np

from oracle import smile_oracle as so
from test_smile_gpu import voiced_clip

# ---- (a) frame geometries ------------------------------------------------------------------------------------------------
# fs -> (frame, hop, nfft).  Full transforms (frame == nfft: every lane's last hm[] / Z[] pair live), frames one sample over
# half the transform (more than half of Z is the pad), the corpus rates besides 8 / 16 / 22.05 / 44.1 / 48 kHz, and the upper
# bound of the ABI.  hop = floor(0.010 fs + 0.5): 51.6 -> 52, 102.4 -> 102, 102.8 -> 103, 204.8 -> 205, 409.6 -> 410, 655.36 -> 655.
RATES = {
    5160: (129, 52, 256),
    10240: (256, 102, 256),
    10280: (257, 103, 512),
    11025: (276, 110, 512),
    12000: (300, 120, 512),
    20480: (512, 205, 512),
    20520: (513, 205, 1024),
    24000: (600, 240, 1024),
    32000: (800, 320, 1024),
    40960: (1024, 410, 1024),
    41000: (1025, 410, 2048),
    65536: (1638, 655, 2048),
}


def frame_clips(fs):
    """The ragged call of one rate: a 0.5 s voiced clip, a 0.3 s one at 180 Hz, 0.2 s of white noise at 0.1, and cuts of a
    voiced clip of exactly frame - 1, frame, frame + 15 hop and frame + 16 hop samples (0 frames, 1 frame, a full last run of
    16, a last run of one frame whose flux needs the frame in front of the run)."""
    P = so.Params(fs)
    long_ = voiced_clip(30 + fs % 11, 1.0, fs=fs)
    clips = [voiced_clip(50 + fs % 13, 0.5, fs=fs), voiced_clip(11, 0.3, fs=fs, f0=180.0),
             (0.1 * np.random.default_rng(fs).standard_normal(int(0.2 * fs))).astype(np.float32)]
    for n in (P.frame - 1, P.frame, P.frame + 15 * P.hop, P.frame + 16 * P.hop):
        assert len(long_) >= n
        clips.append(long_[:n])
    return clips


FRAME_CLIP_FRAMES_TAIL = (0, 1, 16, 17)        # frame counts of the four cuts


# ---- (c) Viterbi + energy gate ----------------------------------------------------------------------------------------------
NC = so.SHS_NCAND
VIT_LENGTHS = (1, 2, 29, 30, 31, 63, 0, 64, 65, 127, 128, 129, 193)     # one ragged call; the zero-frame clip in the middle
GATE_RMS = (0.000999, 0.001, 0.00101)                                   # below, exactly at (kept) and above the energy gate


class VitCase:
    def __init__(self, name, reach, cand, rms, mixed):
        self.name, self.reach = name, reach
        self.cand = np.ascontiguousarray(cand, dtype=np.float64)        # [T, 6, 2] (f0, voicing); f0 = 0: empty slot
        self.rms = np.ascontiguousarray(rms, dtype=np.float64)          # [T] preset pcm_RMSenergy row
        self.mixed = mixed                                              # the oracle track must hold voiced AND unvoiced frames

    @property
    def T(self):
        return self.cand.shape[0]

    def cand3(self):
        """[T, 6, 3] as viterbi_smooth takes it (the score column is not read)."""
        return np.concatenate([self.cand, (self.cand[:, :, :1] > 0).astype(np.float64)], axis=2)

    def expected(self):
        F, V = so.viterbi_smooth(self.cand3())
        return so.energy_gate(F, V, self.rms)


def _random_vit(T, seed):
    """Every slot present with probability 0.6 (any slot, not only the leading ones), F0 log-uniform in [52, 620], voicing
    uniform in (0, 1), about one frame in ten without any candidate; a third of the frames carry one of the three gate values."""
    rng = np.random.default_rng(seed)
    cand = np.zeros((T, NC, 2))
    present = rng.random((T, NC)) < 0.6
    present[rng.random(T) < 0.1] = False
    f = np.exp(rng.uniform(np.log(52.0), np.log(620.0), (T, NC)))
    # Independent draws alone never voice a frame (a transition over a random interval costs 10 per octave against 10 for going
    # unvoiced): two slots in three continue the slot's previous value by a few cents instead of drawing afresh, so that the
    # oracle's track holds voiced runs, octave-free jumps between slots and unvoiced gaps.  The marginal stays inside [52, 620].
    keep = rng.random((T, NC)) < 2.0 / 3.0
    step = np.exp2(0.02 * rng.standard_normal((T, NC)))
    for t in range(1, T):
        f[t] = np.where(keep[t], np.clip(f[t - 1] * step[t], 52.0, 620.0), f[t])
    v = rng.uniform(1e-6, 1.0 - 1e-6, (T, NC))
    cand[:, :, 0] = np.where(present, f, 0.0)
    cand[:, :, 1] = np.where(present, v, 0.0)
    rms = np.where(rng.random(T) < 1.0 / 3.0, np.asarray(GATE_RMS)[rng.integers(0, 3, T)], 0.01)
    return cand, rms


def _frame(*slots):
    """One frame from (slot, f0, voicing) triples."""
    fr = np.zeros((NC, 2))
    for s, f, v in slots:
        fr[s] = (f, v)
    return fr


NONE = _frame()
# Voicing of a candidate at a steady 100 Hz next to a candidate of voicing exactly 0.7 that jumps between 60 and 600 Hz every
# frame (3.3 octaves: never worth following).  Unvoiced costs b = -2 ln(1 - 0.7) + 4 per frame, voiced a = -2 ln(v) + 4 (v < 0.7);
# entering the voiced state costs wTvuv = 10.  With b - a = 0.339 a best path ending INSIDE the stretch is voiced from its first
# frame on once it has seen 30 frames (30 * 0.339 > 10) and not after 29 (29 * 0.339 < 10): the fixed lag of 30 decides the
# stretch's first frame voiced, a lag of 29 would not.
LAG_V = math.exp(-0.5 * (-2.0 * math.log(1.0 - 0.7) + 4.0 - 0.339 - 4.0))


def _lag_stretch(n):
    out = []
    for k in range(n):
        out.append(_frame((0, 100.0, LAG_V), (1, 60.0 if k % 2 == 0 else 600.0, 0.7)))
    return out


def _motifs():
    """(frames, rms values or None) blocks of the structured contour, every block closed by candidate-free frames (forced
    unvoiced, path slope reset to 0).  Costs in the comments: wLocal = 2, wThr = 4, wTvuv = 10, wTvv = 10, wTvvd = 5."""
    m = []
    # exact predecessor tie: 64 Hz in slot 4 and 256 Hz in slot 1, both voicing 1.0 (local cost 0, unvoiced -2 ln(1e-3) + 4 = 17.8),
    # followed by 128 Hz: both transitions cost 10 * 1 + 5 * |+-1 - 0| = 15 exactly; the lowest predecessor index (slot 1, 256 Hz) wins
    m.append(([_frame((4, 64.0, 1.0), (1, 256.0, 1.0)), _frame((2, 128.0, 1.0)), _frame((2, 128.0, 1.0)), NONE], None))
    # voicing exactly 0.7 on a single candidate for 8 frames: voiced 20 + 8 * 0.713 against unvoiced 8 * 6.41; with the
    # threshold penalty on the voiced side as well (v <= cutoff) it would be 20 + 8 * 4.713 and lose
    m.append(([_frame((0, 210.0, 0.7))] * 8 + [NONE, NONE], None))
    # the same candidate in two slots, over the three gate values (the frame at exactly 0.001 is kept)
    m.append(([_frame((0, 300.0, 0.9), (3, 300.0, 0.9))] * 5 + [NONE], [0.01, GATE_RMS[0], GATE_RMS[1], GATE_RMS[2], 0.01, 0.01]))
    # voicing below the 1e-3 clamp: voiced costs -2 ln(1e-3) + 4, the frames stay unvoiced and report v_best = 5e-4
    m.append(([_frame((0, 150.0, 5e-4)), _frame((0, 150.0, 5e-4), (5, 440.0, 5e-4)), _frame((2, 150.0, 5e-4)), NONE], None))
    # voiced stretches of exactly 30 and 31 frames between unvoiced ones, tuned to the fixed lag (see LAG_V)
    m.append((_lag_stretch(30) + [NONE, NONE], None))
    # exact-octave alternatives of a power of two times a constant (55 / 110 / 220 Hz), voicing 1.0, inside one voiced run
    m.append(([_frame((3, 55.0, 1.0), (0, 220.0, 1.0)), _frame((1, 110.0, 1.0)), _frame((1, 110.0, 1.0)),
               _frame((5, 110.0, 1.0), (2, 110.0, 1.0)), NONE],
              [0.01, GATE_RMS[1], GATE_RMS[0], GATE_RMS[2], 0.01]))
    m.append((_lag_stretch(31) + [NONE, NONE], None))
    return m


# the clip's end: 128 Hz entered from an unvoiced frame (slope 0), then 64 Hz (slot 5) and 256 Hz (slot 2) at the same cost
# 15: the best END state ties exactly and the lowest state (slot 2, 256 Hz) is the last frame's decision
_END_TIE = [NONE, _frame((0, 128.0, 1.0)), _frame((5, 64.0, 1.0), (2, 256.0, 1.0))]


def _structured_vit(T):
    frames, rms = [], []
    body = max(0, T - len(_END_TIE)) if T >= len(_END_TIE) else T
    motifs = _motifs()
    k = 0
    while len(frames) < body:
        fr, rm = motifs[k % len(motifs)]
        frames += fr
        rms += list(rm) if rm is not None else [0.01] * len(fr)
        k += 1
    frames, rms = frames[:body], rms[:body]
    if T >= len(_END_TIE):
        frames += _END_TIE
        rms += [0.01] * len(_END_TIE)
    return np.stack(frames) if frames else np.zeros((0, NC, 2)), np.asarray(rms, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def viterbi_cases():
    """Two ragged calls of 13 clips each: seeded random candidates and the structured contour, at every length either side
    of the fixed lag (30) and of the 64-frame chunks (64, 128, 192)."""
    calls = {}
    rnd, stc = [], []
    for k, T in enumerate(VIT_LENGTHS):
        cand, rms = _random_vit(T, 7100 + k)
        rnd.append(VitCase(f"random T={T}", "continuous costs: no ties; chunk pipeline and fixed lag at this length",
                           cand, rms, mixed=T >= 29))
        cand, rms = _structured_vit(T)
        stc.append(VitCase(f"structured T={T}", "exact predecessor / end-state ties, voicing 0.7 / 1.0 / 5e-4, duplicated slot, "
                           "stretches of 30 and 31 tuned to the lag, gate values", cand, rms, mixed=T >= 29))
    calls["random"] = rnd
    calls["structured"] = stc
    return calls


# ---- (d) jitter ---------------------------------------------------------------------------------------------------------------
JIT_VOICING, JIT_RMS = 0.9, 0.01


class JitCase:
    def __init__(self, name, reach, fs, f0, wav, mid=False):
        self.name, self.reach, self.fs = name, reach, fs
        self.f0 = np.ascontiguousarray(f0, dtype=np.float64)            # [T] constructed contour, 0 = unvoiced
        self.wav = np.ascontiguousarray(wav, dtype=np.float32)
        self.mid = mid                                                  # mid-F0: several periods per hop, jitterLocal carries
        assert so.Params(fs).n_frames(len(self.wav)) == len(self.f0)

    def cand(self):
        c = np.zeros((len(self.f0), NC, 2))
        c[:, 0, 0] = self.f0
        c[:, 0, 1] = np.where(self.f0 > 0, JIT_VOICING, 0.0)
        return c

    def cand3(self):
        c = self.cand()
        return np.concatenate([c, (c[:, :, :1] > 0).astype(np.float64)], axis=2)

    def rms(self):
        return np.full(len(self.f0), JIT_RMS)

    def runs(self):
        v = np.concatenate([[False], self.f0 > 0, [False]])
        d = np.diff(v.astype(np.int8))
        return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)))      # [start, end)

    def lag_geometry(self):
        """Largest NL = hi - lo + 1 and W + hi over the voiced frames (the kernel's CCMAX = 1 024 and WCAP = 4 096)."""
        f = self.f0[self.f0 > 0]
        T0 = self.fs / f
        lo, hi = np.ceil(0.75 * T0), np.floor(1.25 * T0)
        return int((hi - lo + 1).max()), int((hi - lo + 1).min()), int((np.floor(T0 + 0.5) + hi).max())


def _n_for_frames(fs, seconds):
    P = so.Params(fs)
    n = int(seconds * fs)
    return n, P.n_frames(n)


def tone(fs, n, f0_frames, seed):
    """Five harmonics (1 / h) following the per-frame contour (frame t owns samples [t hop, (t + 1) hop); unvoiced frames keep
    the last voiced value), every period's length perturbed by 1 % (normal), noise at -30 dB of the 0.5 peak; float32."""
    P = so.Params(fs)
    rng = np.random.default_rng(seed)
    f = np.asarray(f0_frames, dtype=np.float64).copy()
    last = f[f > 0][0]
    for t in range(len(f)):
        if f[t] > 0:
            last = f[t]
        f[t] = last
    phase = np.empty(n)
    pos, ph0 = 0.0, 0.0
    while int(pos) < n:
        t = min(int(pos) // P.hop, len(f) - 1)
        Tp = (fs / f[t]) * (1.0 + 0.01 * rng.standard_normal())
        i0, i1 = int(math.ceil(pos)), min(n, int(math.ceil(pos + Tp)))
        phase[i0:i1] = ph0 + 2.0 * np.pi * (np.arange(i0, i1) - pos) / Tp
        pos += Tp
        ph0 += 2.0 * np.pi
    y = np.zeros(n)
    for h in range(1, 6):
        y += (1.0 / h) * np.sin(h * phase + rng.uniform(0.0, 6.28))
    y = 0.5 * y / np.abs(y).max() + 0.5 * 10.0 ** (-30.0 / 20.0) * rng.standard_normal(n)
    return y.astype(np.float32)


def _cut_runs(T, starts_lengths, f_of_run):
    f0 = np.zeros(T)
    for k, (s, ln) in enumerate(starts_lengths):
        assert ln >= 3 and s + ln <= T and (s == 0 or f0[s - 1] == 0.0) and not f0[s:s + ln].any()
        f0[s:s + ln] = f_of_run(k)
    return f0


JIT_RATES = (5160, 8000, 16000, 48000, 65536)


@functools.lru_cache(maxsize=None)
def jitter_cases():
    """fs -> the cases of that rate's ragged call (built once; callers leave the arrays unchanged)."""
    out = {}

    def add(c):
        out.setdefault(c.fs, []).append(c)

    for fs in (65536, 48000, 16000):                      # low F0: the restaged window, NL up to 631 (ten lag passes of 64)
        n, T = _n_for_frames(fs, 0.6)
        f0 = np.linspace(52.0, 56.0, T)
        add(JitCase(f"low F0 52-56 Hz at {fs}", "NL = hi - lo + 1 up to fs / 104 + 1 lags, W + hi up to 2.25 fs / 52 samples of the "
                    "4 096-sample window (restaged almost every period at 65 536 Hz), the dead exit at the clip's end; fewer "
                    "than two periods per hop: shimmer and logHNR carry the comparison", fs, f0, tone(fs, n, f0, 9000 + fs % 97)))
    n, T = _n_for_frames(16000, 0.6)
    f0 = np.full(T, 110.0)
    add(JitCase("110 Hz at 16000", "NL = 181 - 110 + 1 = 72: two lag passes, the second one partial", 16000, f0, tone(16000, n, f0, 9101), mid=True))
    # the same contour over a tone of 91 Hz: the matched period (176 samples) sits at lag index 66 of the 72, in the SECOND lag
    # pass; with the tone at its nominal 110 Hz the maximum is always found in the first pass (index 35)
    add(JitCase("110 Hz contour over a 91 Hz tone", "the best lag lies in the partial second lag pass", 16000, f0,
                tone(16000, n, np.full(T, 91.0), 9102)))
    for fs in (8000, 5160):                               # the shortest periods
        n, T = _n_for_frames(fs, 0.6)
        f0 = np.linspace(600.0, 620.0, T)
        add(JitCase(f"600-620 Hz at {fs}", "the shortest lag ranges (NL = 4 and W = 8 at 5 160 Hz): most lanes idle", fs, f0,
                    tone(fs, n, f0, 9200 + fs % 89)))
    # 2.2 s at 16 kHz = 218 frames cut into 12 voiced runs of unequal length (more than JWAVES = 8: the round-robin wraps).  One
    # clip cannot start runs at both 63 and 64 (a run needs an unvoiced frame in front of it): A has the starts 63 (straddles the
    # 64-frame block boundary: the carry bit) and 128 (starts on it), B the starts 64 and 126 (straddles 128).  The last run of
    # each reaches the last frame at 110 Hz, where W + hi = 326 samples pass the clip's end (frame - hop = 240): the dead exit.
    n, T = _n_for_frames(16000, 2.2)
    assert T == 218
    layA = [(2, 5), (9, 9), (20, 3), (25, 12), (40, 7), (49, 4), (55, 6), (63, 11), (78, 30), (110, 16), (128, 40), (190, 28)]
    layB = [(0, 4), (6, 10), (18, 3), (23, 13), (38, 8), (48, 5), (55, 7), (64, 20), (86, 31), (126, 9), (140, 44), (200, 18)]
    for tag, lay, seed in (("A", layA, 9301), ("B", layB, 9302)):
        f0 = _cut_runs(T, lay, lambda k: 110.0 if k == 11 else 250.0)
        add(JitCase(f"12 runs {tag}", "12 voiced runs over 8 workgroups; runs that start on a 64-frame block boundary or straddle it; "
                    "the last run ends with the clip (dead exit)", 16000, f0, tone(16000, n, f0, seed), mid=True))
    # steps between 200 and 400 Hz from one frame to the next inside one run.  The level changes every 3 frames, not every frame:
    # a contour that alternated every frame would cost the Viterbi pass 10 + 5 * 2 = 20 per frame against 8.6 unvoiced, and the
    # F0 row would no longer be the constructed contour.
    n, T = _n_for_frames(16000, 0.6)
    f0 = np.where((np.arange(T) // 3) % 2 == 0, 200.0, 400.0)
    add(JitCase("steps 200 / 400 Hz", "lo, hi, W change inside a run while the period chain goes on", 16000, f0,
                tone(16000, n, f0, 9401), mid=True))
    n, T = _n_for_frames(16000, 0.3)
    f0 = np.full(T, 200.0)
    add(JitCase("all-zero waveform", "e0 = 0: every correlation is 0, the first lag wins, A = 0", 16000, f0, np.zeros(n, np.float32)))
    # 0.25: every product is 2^-4 and every partial sum exact in any order, so all correlations are exactly 1 on both sides
    add(JitCase("DC waveform", "all correlations exactly 1: first lag, no refinement; A = 0: the shimmer guard; logHNR at its upper clamp",
                16000, f0, np.full(n, 0.25, np.float32)))
    assert sorted(out) == list(JIT_RATES)
    return out
