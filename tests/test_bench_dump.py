"""bench.py's inputs and --dump-outputs, without a GPU: the column blocks of a result row, the 64 MB cap, and clips
synthesised on worker processes equal to the in-process ones."""
import importlib
import os

import numpy as np
import torch

from robust_speech_analysis_framework_amd import benchlib, synth


def _bench():
    return importlib.import_module("bench")           # by name: spawned workers import their function from it


def test_column_blocks_cover_the_result_row():
    b = _bench()
    # pipeline.Pipeline.run: [mshds 25 | smile 912 | logits 2 | w2v2 frames 1]
    assert b.output_columns(benchlib.CONFIGS["e2e"]) == [("mshds_features", 25), ("smile_functionals", 912),
                                                         ("cnnlstm_logits", 2), ("w2v2_frames", 1)]
    assert b.output_columns(benchlib.CONFIGS["C2"]) == [("mshds_features", 25), ("smile_functionals", 912)]
    assert b.output_columns(benchlib.CONFIGS["C3"]) == [("w2v2_frames", 1)]
    assert b.output_columns(benchlib.CONFIGS["C4"]) == [("cnnlstm_logits", 2)]


def test_dump_writes_every_block_and_samples_above_the_cap(tmp_path, monkeypatch):
    b = _bench()
    stages = benchlib.CONFIGS["e2e"]
    rows = torch.arange(7 * 940, dtype=torch.float32).view(7, 940)
    rows[3, 4] = float("nan")                                   # MSHDS cells may be NaN by contract
    b.dump_outputs(str(tmp_path / "all"), rows, stages)
    got = [np.load(tmp_path / "all" / f"{name}.npy") for name, _ in b.output_columns(stages)]
    assert all(g.dtype == np.float32 for g in got)
    np.testing.assert_array_equal(np.concatenate(got, axis=1), rows.numpy())
    assert not (tmp_path / "all" / "sample_rows.npy").exists()

    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 3 * (4 * 940 + 8))
    for run in ("a", "b"):
        b.dump_outputs(str(tmp_path / run), rows, stages)
    idx = np.load(tmp_path / "a" / "sample_rows.npy")
    assert idx.dtype == np.float64 and len(idx) == 3 and (np.diff(idx) > 0).all()
    np.testing.assert_array_equal(idx, np.load(tmp_path / "b" / "sample_rows.npy"))
    sm = np.load(tmp_path / "a" / "smile_functionals.npy")
    np.testing.assert_array_equal(sm, rows.numpy()[idx.astype(int), 25:937])
    total = sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= 3 * (4 * 940 + 8) + 5 * 128                 # + one .npy header per file


def test_clips_from_worker_processes_equal_in_process_synthesis():
    b = _bench()
    ids = [0, 5, 63]
    got = b.synth_clips(ids, 0.25, 2)
    assert sorted(got) == ids
    for k in ids:
        assert np.array_equal(got[k], synth.synth_clip(k, 0.25))
