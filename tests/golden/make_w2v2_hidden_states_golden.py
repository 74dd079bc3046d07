"""Generate tests/golden/w2v2_hidden_states_small.npz from the installed third-party ``transformers`` module.

``Wav2Vec2Model(..., output_hidden_states=True).hidden_states`` (num_hidden_layers + 1 entries) for every combination of
the three config switches of the large checkpoints (``feat_extract_norm="layer"``, ``conv_bias``, ``do_stable_layer_norm``)
at the small golden geometry of ``make_w2v2_variants_golden.py``, with the build's seeded random weights, on an 8 000- and a
20 000-sample input.  Post-LN models normalise every entry; stable-layer-norm models leave entries 0..L-1 un-normalised.
Run in the build container:  python tests/golden/make_w2v2_hidden_states_golden.py
"""
import json
import os
import sys

import numpy as np
import torch
from transformers import Wav2Vec2FeatureExtractor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_w2v2_variants_golden import LENGTHS, SEED, SMALL, hf_model, variant  # noqa: E402
from robust_speech_analysis_framework_amd.w2v2_config import random_state_dict  # noqa: E402
from robust_speech_analysis_framework_amd import synth  # noqa: E402


def hidden_states(cfg, sd, x: np.ndarray):
    """[L + 1, T, H] float32: transformers' hidden_states of one window."""
    iv = Wav2Vec2FeatureExtractor(do_normalize=cfg.do_normalize)(x, sampling_rate=16000, return_tensors="pt").input_values
    with torch.no_grad():
        o = hf_model(cfg, sd)(iv, output_hidden_states=True)
    hs = np.stack([h.numpy()[0] for h in o.hidden_states])
    assert np.array_equal(hs[-1], o.last_hidden_state.numpy()[0])
    return hs


if __name__ == "__main__":
    torch.set_num_threads(4)
    out = {"cfg": np.array(json.dumps(SMALL)), "seed": np.array(SEED)}
    clip = synth.synth_clip(50, 2.0)                      # the clip of w2v2_variants_small.npz
    for flags in range(8):
        cfg = variant(flags)
        sd = random_state_dict(cfg, seed=SEED)
        for n in LENGTHS:
            hs = hidden_states(cfg, sd, clip[:n])
            out[f"hidden_states_f{cfg.flags}_{n}"] = hs
            print(f"f{cfg.flags}_{n}", hs.shape, [round(float(h.std()), 3) for h in hs])
    np.savez_compressed(os.path.join(HERE, "w2v2_hidden_states_small.npz"), **out)
