"""The frame kernel at the geometries no natural corpus rate reaches: transforms the frame fills completely, frames one sample
over half the transform, the remaining corpus rates and the ABI's upper bound - at the bars tests/test_smile_gpu.py already
sets (roll-off rows and the voicing pattern exact, every other row at TIGHT, the pitch chain stage by stage).  Parity unpinned:
the oracle is this repository's restatement of the openSMILE components."""
import numpy as np
import pytest

from oracle import smile_oracle as so
import smile_stage_cases as sc
from test_smile_gpu import _MINI_CONF, _assert_all_912, _check_pitch_chain, _check_rows, _run_gpu, voiced_clip

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fs", sorted(sc.RATES))
def test_frame_geometries(rsaf_lib, fs):
    """One ragged call per rate: two voiced clips, noise, and clips of 0, 1, 16 and 17 frames (smile_stage_cases.frame_clips)."""
    P = so.Params(fs)
    assert (P.frame, P.hop, P.nfft) == sc.RATES[fs]
    clips = sc.frame_clips(fs)
    p, g, octv, cand = _run_gpu(clips, fs=fs)
    assert p.frames == [P.n_frames(len(c)) for c in clips] and tuple(p.frames[3:]) == sc.FRAME_CLIP_FRAMES_TAIL
    ref = np.concatenate([so.lld(c, P) for c in clips], axis=1)
    assert g.shape == ref.shape and octv.shape[1] == P.nbins
    _check_pitch_chain(clips, p, g, octv, cand, P)
    _check_rows(g, ref, P)


@pytest.mark.parametrize("fs", [32000, 11025])
def test_dropin_at_untested_file_rates(rsaf_lib, tmp_path, fs):
    """extract_opensmile_features on a 0.8 s WAV of a rate the drop-in test does not have: the whole row of 912."""
    import pandas as pd
    from robust_speech_analysis_framework_amd import smile, synth
    x = voiced_clip(60 + fs % 7, 0.8, fs=fs)
    path = str(tmp_path / f"native_{fs}.wav")
    synth.write_wav(path, np.round(x * 32768.0).astype(np.int16), fs=fs)
    conf = tmp_path / "Androids.conf"
    conf.write_text(_MINI_CONF)
    out = smile.extract_opensmile_features(pd.DataFrame({"filepath": [path]}), "/nonexistent/SMILExtract", str(conf), verbose=False)
    assert list(out.columns) == so.feature_names() + ["filename"] and list(out["filename"]) == [f"native_{fs}.wav"]
    vals = out[so.feature_names()].to_numpy(dtype=np.float64)
    ref = so.extract(x, fs=fs)
    _assert_all_912(vals, ref[None, :])
