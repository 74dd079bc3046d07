"""The float64 restatement of the training step with the input as a leaf (tests/input_grad_restatement.py), without a GPU.

Logits, loss and parameter gradients equal ``oracle.cnnlstm_train_oracle.forward_backward`` on the same inputs to 1e-12
relative (the ops and their order are the same); ``dx`` matches ``x.grad`` of the reference's own module
(tests/golden/cnnlstm_input_grad_*.npz): samples within RTOL of the largest sample, sum of squares within 4 RTOL, the form of
``test_step_matches_reference_vectors``.  The inputs of the GPU tests (tests/test_cnnlstm_input_grad_gpu.py) keep the
max-pool gap on the restatement alone; that is checked here too, since a near-tie reroutes a whole row of ``dx``."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import cnnlstm_geometry as geo  # noqa: E402
import input_grad_cases as igc  # noqa: E402
import input_grad_restatement as igr  # noqa: E402
from cnnlstm_support import RTOL  # noqa: E402
from weights import sample_tensor, synth_input, synth_state_dict  # noqa: E402

from oracle import cnnlstm_train_oracle as to  # noqa: E402

GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "cnnlstm_input_grad_*.npz")))


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


@pytest.mark.parametrize("i", [0, 2, 4, 10], ids=geo.case_id)
def test_restatement_equals_the_oracle(i):
    x, labels, mk = geo.train_inputs(i)
    want = to.forward_backward(geo.state_dict(i), x, labels, geo.CASES[i][3], masks=mk, return_stages=True)
    got = igc.restated(i)
    assert _rel(got["logits"], want["logits"]) <= 1e-12 and abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])
    assert set(got["grads"]) == set(want["grads"])
    for k, g in want["grads"].items():
        assert _rel(got["grads"][k], g) <= 1e-12, k
    for k, v in want["stages"].items():
        assert _rel(got["stages"][k], v) <= 1e-12, k
    for k, (mean, var, n) in want["bn_stats"].items():
        assert _rel(got["bn_stats"][k][0], mean) <= 1e-12 and _rel(got["bn_stats"][k][1], var) <= 1e-12 and got["bn_stats"][k][2] == n
    assert got["dx"].shape == x.shape and np.isfinite(got["dx"]).all() and np.abs(got["dx"]).max() > 0


def test_dx_is_the_derivative_of_the_loss():
    """Central differences of the restated loss along two random directions of x (geometry row 0, the smallest)."""
    x, labels, mk = geo.train_inputs(0)
    sd, act = geo.state_dict(0), geo.CASES[0][3]
    dx = igc.restated(0)["dx"]
    rng = np.random.Generator(np.random.PCG64(77))
    for _ in range(2):
        v = rng.standard_normal(x.shape)
        eps = 1e-6
        x64 = x.astype(np.float64)
        lp = igr.forward_backward(sd, x64 + eps * v, labels, act, masks=mk)["loss"]
        lm = igr.forward_backward(sd, x64 - eps * v, labels, act, masks=mk)["loss"]
        want = (lp - lm) / (2 * eps)
        assert abs((dx * v).sum() - want) <= 1e-6 * max(abs(want), np.abs(dx).max()), ((dx * v).sum(), want)


def test_goldens_are_the_four_training_cases():
    names = [os.path.basename(p)[len("cnnlstm_input_grad_"):] for p in GOLDEN]
    assert names == sorted(os.path.basename(p)[len("cnnlstm_train_"):] for p in glob.glob(os.path.join(HERE, "golden", "cnnlstm_train_*.npz")))
    assert len(names) == 4


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[19:-4] for p in GOLDEN])
def test_restated_dx_matches_reference_vectors(path):
    z = np.load(path)
    t = np.load(path.replace("cnnlstm_input_grad_", "cnnlstm_train_"))
    D, C, H, B, T, seed = [int(v) for v in z["meta"]]
    assert [int(v) for v in t["meta"]] == [D, C, H, B, T, seed]
    got = igr.forward_backward(synth_state_dict(D, C, H, seed), synth_input(B, T, D, seed + 1000), t["labels"], str(z["act"]))
    assert _rel(got["logits"], t["logits"]) <= 1e-9 and abs(got["loss"] - float(t["loss"])) <= 1e-9
    ref, s = z["dx"], sample_tensor(got["dx"])
    err = np.abs(s[:-2] - ref[:-2]).max() / max(np.abs(ref[:-2]).max(), 1e-7)
    print(f"{os.path.basename(path)}: dx samples {err:.2e} of the largest, sum of squares {abs(s[-1] - ref[-1]) / ref[-1]:.2e}")
    assert err < RTOL, err
    assert abs(s[-1] - ref[-1]) <= 4 * RTOL * max(abs(ref[-1]), 1e-12)
    assert got["dx"].shape == (B, T, D) and np.abs(got["dx"][:, -1]).max() > 0      # the last frame carries gradient too


@pytest.mark.parametrize("case", igc.DX_CASES + igc.PAIR_CASES, ids=igc.dx_case_id)
def test_gpu_test_inputs_keep_the_pool_gap(case):
    """Every input of the GPU comparison keeps the closest max-pool pair of the restatement's res1 at POOL_GAP or more."""
    want = igc.restated_case(case)
    gap = geo.pool_gap(want["stages"]["res1"])
    print(f"{igc.dx_case_id(case)}: closest max-pool pair {gap:.2e}")
    assert gap >= igc.POOL_GAP, gap


@pytest.mark.parametrize("i", igc.MIX_ROWS, ids=geo.case_id)
def test_mixed_input_keeps_the_pool_gap(i):
    e = igc.mix_case(i)
    gap = geo.pool_gap(e["want"]["stages"]["res1"])
    print(f"layer mix in front of {geo.case_id(i)}: closest max-pool pair {gap:.2e}")
    assert gap >= igc.POOL_GAP, gap
    # the float64 mix and its gradient hang together: dp . (a direction of p) is the change of the loss along it
    assert e["dp64"].shape == (igc.MIX_L,) and np.isfinite(e["dp64"]).all()
