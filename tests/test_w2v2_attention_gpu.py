"""The fused attention kernel (csrc/w2v2_encoder.hip, attn_f16x3_kernel) at the frame counts where its code changes path,
against the float64 restatement of the whole forward (tests/w2v2_reference64.py).

Geometry: conv_dim 32 x 7, hidden 128, 2 heads (width 64: the fused kernel), 1 layer, intermediate 128, 16 positional taps
in 8 groups, seeded weights.  Windows of 400 + 320 (T - 1) samples give exactly T frames, T = 2, 31, 32, 33, 127, 128, 129,
249, 255, 256: either side of the 32-key tile that holds keys to mask, of the switch from one staged key block to two, of the
second query half, and last query waves with few valid rows.

(a) all windows in one ragged call: per window max |got - ref| / max |ref| of the last hidden state stays within 1.25 x the
    figure of the kernel before the softmax was restated in base 2 with the normalisation moved to the output (PARENT_ERR:
    measured once on an MI355X with this file, `python tests/test_w2v2_attention_gpu.py`, at the parent commit;
    profiles/r21/attn_error_parent.txt is that run).  The oracle under oracle/ is float32 and cannot resolve these figures.
(b) the ragged call returns the bits of one call per window.
(c) (a) at T = 33, 129, 249 with the q / k projection weights x 8 (peaked rows: exponents far below the underflow point) and
    x 0.01 (near-uniform rows).
(d) the position-bias instance: WavLM at the small geometry of tests/test_w2v2_families.py (num_buckets 32,
    max_bucket_distance 40) with its 64 channels as ONE head of width 64, at T = 33, 129, 249 against transformers'
    WavLMModel, at the tolerance of tests/test_w2v2_families_gpu.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from robust_speech_analysis_framework_amd import synth                                       # noqa: E402
from robust_speech_analysis_framework_amd.w2v2_config import W2V2Config, random_state_dict   # noqa: E402
from w2v2_reference64 import forward64                                                       # noqa: E402

pytestmark = pytest.mark.gpu

GEOM = dict(conv_dim=(32,) * 7, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
            intermediate_size=128, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=8)
FRAMES = (2, 31, 32, 33, 127, 128, 129, 249, 255, 256)
RANGE_FRAMES = (33, 129, 249)
QK_SCALES = (8.0, 0.01)
SEED = 21

# max |got - ref64| / max |ref64| of the last hidden state per window at the parent commit: {q/k weight scale: {T: figure}}
PARENT_ERR = {1.0: {2: 4.8718e-07, 31: 6.3027e-07, 32: 7.4792e-07, 33: 4.5588e-07, 127: 6.3333e-07, 128: 5.7523e-07, 129: 7.7141e-07,
                    249: 9.8679e-07, 255: 6.9858e-06, 256: 8.2742e-07},
              8.0: {33: 4.0414e-06, 129: 1.1420e-05, 249: 1.2379e-05},
              0.01: {33: 6.6002e-07, 129: 7.2541e-07, 249: 1.4302e-06}}


def _spec(frames):
    return [(37 * i, 400 + 320 * (T - 1)) for i, T in enumerate(frames)]


def _scaled_qk(sd, f):
    out = dict(sd)
    for k in sd:
        if k.endswith(("q_proj.weight", "k_proj.weight")):
            out[k] = (sd[k].astype(np.float64) * f).astype(np.float32)
    return out


def _run(eng, clip, spec):
    """one ragged call -> (packed last hidden state, window row offsets), host arrays"""
    import torch
    T = [eng.cfg.frames(l) for _, l in spec]
    rows = np.concatenate([[0], np.cumsum(T)])
    wav = torch.from_numpy(np.ascontiguousarray(clip, dtype=np.float32)).cuda()
    out = torch.full((int(rows[-1]), eng.cfg.hidden_size), float("nan"), dtype=torch.float32, device="cuda")
    eng.forward_windows(wav, [s for s, _ in spec], [l for _, l in spec], out, rows[:-1])
    torch.cuda.synchronize()
    return out.cpu().numpy(), rows


class Case:
    """The seeded model with its q / k weights scaled by `qk`, the windows of `frames`, the ragged call's output and the
    float64 reference of every window (computed once, never changed)."""

    def __init__(self, qk, frames):
        from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
        self.cfg = W2V2Config(**GEOM)
        assert self.cfg.head_dim == 64
        self.sd = _scaled_qk(random_state_dict(self.cfg, SEED), qk)
        self.eng = W2V2Engine(self.cfg, self.sd)
        self.clip = synth.synth_clip(321, 6.0)
        self.frames, self.spec = frames, _spec(frames)
        assert [self.cfg.frames(l) for _, l in self.spec] == list(frames)
        assert max(s + l for s, l in self.spec) <= len(self.clip)
        self.got, self.rows = _run(self.eng, self.clip, self.spec)
        self.refs = [forward64(self.sd, self.cfg, self.clip[s:s + l])[-1] for s, l in self.spec]
        for r in self.refs:
            r.setflags(write=False)

    def errors(self):
        out = {}
        for k, T in enumerate(self.frames):
            got, ref = self.got[self.rows[k]:self.rows[k + 1]], self.refs[k]
            assert got.shape == ref.shape == (T, self.cfg.hidden_size) and np.isfinite(got).all(), T
            out[T] = float(np.abs(got - ref).max() / np.abs(ref).max())
        return out


_cases = {}


def _case(qk):
    if qk not in _cases:
        _cases[qk] = Case(qk, FRAMES if qk == 1.0 else RANGE_FRAMES)
    return _cases[qk]


def _check_against_parent(qk):
    assert PARENT_ERR is not None, "the parent's figures are missing from this file"
    err = _case(qk).errors()
    for T, e in err.items():
        print(f"q/k x {qk:g} T = {T:3d}: rel {e:.4e}   parent {PARENT_ERR[qk][T]:.4e}   ratio {e / PARENT_ERR[qk][T]:.3f}")
    for T, e in err.items():
        assert e <= 1.25 * PARENT_ERR[qk][T], (qk, T, e, PARENT_ERR[qk][T])


def test_every_window_as_close_to_float64_as_the_parent(rsaf_lib):
    _check_against_parent(1.0)


def test_ragged_call_returns_the_bits_of_one_call_per_window(rsaf_lib):
    import torch
    c = _case(1.0)
    wav = torch.from_numpy(c.clip).cuda()
    alone = torch.zeros((int(c.rows[-1]), c.cfg.hidden_size), device="cuda")
    for k, (s0, l) in enumerate(c.spec):
        c.eng.forward_windows(wav, [s0], [l], alone, [int(c.rows[k])])
    torch.cuda.synchronize()
    assert np.isfinite(c.got).all() and np.array_equal(c.got, alone.cpu().numpy())


@pytest.mark.parametrize("qk", QK_SCALES)
def test_exponent_range_peaked_and_near_uniform_rows(rsaf_lib, qk):
    _check_against_parent(qk)


def test_position_bias_instance_matches_transformers(rsaf_lib):
    """WavLM (REL_POS_BIAS) with heads of width 64: attn_f16x3_kernel<true>."""
    from robust_speech_analysis_framework_amd.w2v2 import W2V2Engine
    from test_w2v2_families import SMALL
    from test_w2v2_families_gpu import TOL, _hf_hidden
    cfg = W2V2Config(**{**SMALL, "num_attention_heads": 1}, model_type="wavlm", num_buckets=32, max_bucket_distance=40)
    assert cfg.head_dim == 64 and cfg.num_hidden_layers == 2
    sd = random_state_dict(cfg, SEED + 1)
    eng = W2V2Engine(cfg, sd)
    clip = synth.synth_clip(322, 6.0)
    spec = _spec(RANGE_FRAMES)
    got, rows = _run(eng, clip, spec)
    refs = _hf_hidden(cfg, sd, [clip[s:s + l] for s, l in spec], [cfg.num_hidden_layers])
    for k, T in enumerate(RANGE_FRAMES):
        w, ref = got[rows[k]:rows[k + 1]], refs[k][0]
        assert w.shape == ref.shape == (T, cfg.hidden_size) and np.isfinite(w).all()
        e = np.abs(w - ref).max() / np.abs(ref).max()
        print(f"wavlm T = {T}: rel {e:.3e}")
        assert e < TOL, (T, e)


if __name__ == "__main__":          # the table of PARENT_ERR, as the library in the tree gives it
    print("max |got - ref64| / max |ref64| of the last hidden state per window (geometry and windows: this file)")
    table = {qk: _case(qk).errors() for qk in (1.0,) + QK_SCALES}
    for qk, err in table.items():
        for T, e in err.items():
            print(f"q/k x {qk:g} T = {T:3d}: {e:.6e}")
    print("PARENT_ERR = {" + ", ".join(f"{qk!r}: {{" + ", ".join(f"{T}: {e:.4e}" for T, e in err.items()) + "}" for qk, err in table.items()) + "}")
