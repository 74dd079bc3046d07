"""The Wav2Vec2 front end (window normalisation, conv0 + GroupNorm, the conv stack, the feature projection) on waveforms a
microphone actually produces, against the float64 restatement of tests/w2v2_reference64.py.

Geometry: conv_dim 32 x 7, hidden 128, 1 layer, 2 heads, intermediate 128, 16 positional taps in 8 groups; seeded weights with
conv0's redrawn uniformly in +-10^-1/2 (with conv biases: conv0's bias 3 uniform(0.5, 1)).
Configurations: (a) group norm, do_normalize; (b) group norm, raw samples (HuBERT-base / WavLM-base preprocessing); (c) group
norm with conv biases; (d) layer-norm feature encoder, conv biases, stable layer norm (large-lv60 / XLS-R).
Windows of 400 + 320 (T - 1) samples, T = 2, 33, 129: 143, 2127 and 8271 conv0 frames (one partial statistics slab, five
slabs with a partial last one, seventeen), the three of a waveform kind in ONE ragged call.
Kinds (w2v2_reference64.waveform): control (speech, sd 0.1), dc-mild (0.05 + speech at sd 0.02), dc-strong (0.3 + speech at
sd 0.01), dc-extreme (0.5 + noise at sd 0.002), quiet (speech at sd 1e-4 and at 1e-6, where var + 1e-7 is mostly the
epsilon), loud (a +-1 square wave at 180 Hz + noise), silence, constant 0.25, onset (first half zeros, then control).

Per configuration, kind and window, hidden state 0 and the last hidden state (forward_windows(..., hidden=[0, 1])):
    err = max |got - ref64| / max |ref64|        (silence and constant: the denominator is max(max |ref64|, 1))
    err <= max(8 e32, 2e-6), every value finite
e32 is the same figure for the SAME restatement run in float32 on the CPU: it rises by itself on the ill-conditioned kinds as
far as float32 arithmetic has to.  8 = 2^-21 / 2^-24, the two-plane fp16 operand format (tests/test_gemm_gpu.py) against
float32; 2e-6 is that test's floor for "as good as an fp32 FMA chain".  The bar comes from the reference alone.

Before any launch the reference itself is checked to be as hard as meant: max over the channels of mean^2 / (var + 1e-5) of the
float64 conv0 output is >= 1e4 for dc-extreme in (b), >= 30 for control in (c), <= 1e-2 for control in (a) and (b), and
>= DC_STRONG_MIN for dc-strong in (b).  DC_STRONG_MIN is 8e2, not the 1e3 first asked of it: speech at sd 0.01 varies slowly
against conv0's ten taps, so a channel passes it with the gain it has for the offset, and mean^2 / var cannot exceed
0.3^2 / 0.01^2 = 900 (the 3.5e3 of white noise at that sd comes from the taps averaging the noise down).

A second test repeats every ragged call as one call per window and requires the same bits.

`python tests/test_w2v2_conditioning_gpu.py` prints the table of every cell (profiles/r26/w2v2_conditioning.txt is one run)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import w2v2_reference64 as R                                                                 # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 8.0, 2e-6
DC_STRONG_MIN = 8e2
UNIT_DENOMINATOR = ("silence", "constant")


def _m2v(name, kind):
    cfg, sd = R.conditioned_weights(name)
    return [R.mean2_over_var(R.conv0_output(sd, cfg, R.waveform(kind, n))) for n in R.LENGTHS]


_conditions_checked = []


def _check_reference_conditions():
    """on the reference alone, once, before the first launch"""
    if _conditions_checked:
        return
    assert min(_m2v("b-group-raw", "dc-strong")) >= DC_STRONG_MIN
    assert min(_m2v("b-group-raw", "dc-extreme")) >= 1e4
    assert min(_m2v("c-group-bias", "control")) >= 30
    assert max(_m2v("a-group", "control") + _m2v("b-group-raw", "control")) <= 1e-2
    _conditions_checked.append(True)


def _figure(x, ref, kind):
    den = np.abs(ref).max()
    return float(np.abs(x - ref).max() / (max(den, 1.0) if kind in UNIT_DENOMINATOR else den))


_engines = {}


def _engine(name):
    if name not in _engines:
        from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
        cfg, sd = R.conditioned_weights(name)
        _engines[name] = (cfg, sd, W2V2Engine(cfg, sd))
    return _engines[name]


class Cell:
    """One configuration x kind: the three windows back to back in one buffer, the ragged call's two hidden states, and per
    window the float64 reference and the float32 baseline (computed once, never changed)."""

    def __init__(self, name, kind):
        import torch
        _check_reference_conditions()
        self.name, self.kind = name, kind
        self.cfg, self.sd, self.eng = _engine(name)
        L = self.cfg.num_hidden_layers
        self.wavs = [R.waveform(kind, n) for n in R.LENGTHS]
        self.clip = np.concatenate(self.wavs)
        starts = np.concatenate([[0], np.cumsum(R.LENGTHS)])[:-1]
        self.spec = [(int(s), int(n)) for s, n in zip(starts, R.LENGTHS)]
        assert [self.cfg.frames(n) for n in R.LENGTHS] == list(R.FRAMES)
        self.ref64 = [[h[j] for j in (0, L)] for h in (R.forward64(self.sd, self.cfg, w) for w in self.wavs)]
        self.ref32 = [[h[j] for j in (0, L)] for h in (R.forward64(self.sd, self.cfg, w, dtype=torch.float32) for w in self.wavs)]
        for pair in self.ref64 + self.ref32:
            for a in pair:
                a.setflags(write=False)
        self.rows = np.concatenate([[0], np.cumsum(R.FRAMES)])
        self.dev = torch.from_numpy(self.clip).cuda()
        self.out = torch.full((int(self.rows[-1]), self.cfg.hidden_size), float("nan"), dtype=torch.float32, device="cuda")
        _, planes = self.eng.forward_windows(self.dev, [s for s, _ in self.spec], [n for _, n in self.spec], self.out,
                                             self.rows[:-1], hidden=[0, L])
        torch.cuda.synchronize()
        self.got = planes.cpu().numpy()                           # [2, rows, hidden]
        self.last = self.out.cpu().numpy()

    def table(self):
        """[(T, state, err, e32, bar)] of the cell's windows"""
        out = []
        for k, T in enumerate(R.FRAMES):
            for j, state in enumerate((0, self.cfg.num_hidden_layers)):
                got, ref = self.got[j, self.rows[k]:self.rows[k + 1]], self.ref64[k][j]
                assert got.shape == ref.shape == (T, self.cfg.hidden_size)
                assert np.isfinite(got).all(), (self.name, self.kind, T, state)
                e32 = _figure(self.ref32[k][j], ref, self.kind)
                out.append((T, state, _figure(got, ref, self.kind), e32, max(FACTOR * e32, FLOOR)))
        return out


_cells = {}


def _cell(name, kind):
    if (name, kind) not in _cells:
        _cells[name, kind] = Cell(name, kind)
    return _cells[name, kind]


def _print(name, kind, rows):
    for T, state, err, e32, bar in rows:
        print(f"{name:20s} {kind:11s} T {T:3d} hidden[{state}]  err {err:.3e}  e32 {e32:.3e}  err/e32 {err / max(e32, 1e-300):8.2f}  "
              f"bar {bar:.3e}  {'ok' if err <= bar else 'ABOVE'}")


def test_reference_is_as_hard_as_meant():
    _check_reference_conditions()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_front_end_stays_within_8x_float32_of_float64(rsaf_lib, name, kind):
    c = _cell(name, kind)
    rows = c.table()
    _print(name, kind, rows)
    assert np.array_equal(c.last, c.got[1])                       # the call's output is its last hidden state
    for T, state, err, e32, bar in rows:
        assert err <= bar, (name, kind, T, state, err, e32, bar)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_ragged_call_returns_the_bits_of_one_call_per_window(rsaf_lib, name):
    import torch
    for kind in R.KINDS:
        c = _cell(name, kind)
        L = c.cfg.num_hidden_layers
        alone = torch.zeros_like(c.out)
        planes = np.zeros_like(c.got)
        for k, (s0, n) in enumerate(c.spec):
            _, p = c.eng.forward_windows(c.dev, [s0], [n], alone, [int(c.rows[k])], hidden=[0, L])
            torch.cuda.synchronize()
            planes[:, c.rows[k]:c.rows[k + 1]] = p.cpu().numpy()[:, c.rows[k]:c.rows[k + 1]]
        assert np.isfinite(c.got).all() and np.array_equal(c.got, planes), (name, kind)
        assert np.array_equal(c.last, alone.cpu().numpy()), (name, kind)


if __name__ == "__main__":          # the table of every cell, as the library in the tree gives it
    print("err = max |got - ref64| / max |ref64| per window; e32: the float32 restatement's; bar = max(8 e32, 2e-6)")
    above = 0
    for name in R.CONFIGS:
        for kind in R.KINDS:
            rows = _cell(name, kind).table()
            _print(name, kind, rows)
            above += sum(err > bar for _, _, err, _, bar in rows)
    print(f"cells above the bar: {above}")
