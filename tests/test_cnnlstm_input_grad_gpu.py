"""The gradient of the loss with respect to the CNN-LSTM's input on the MI355X (``rsaf_cnnlstm_train_backward_dx`` and its
group forms, through ``model(x)`` and ``cnnlstm_train_group``).

Bars.  ``dx`` against the float64 restatement (tests/input_grad_restatement.py) and against ``x.grad`` of the reference's own
module (tests/golden/cnnlstm_input_grad_*.npz): ``cnnlstm_support.RTOL`` = 1e-4 of the largest magnitude of the tensor, the
project's float tolerance (stock torch in float32 against float64 differs by 5.8e-7 to 1.6e-6 of max|dx| on the geometry
rows, so a correct float32 path keeps a factor 60 under it); sum of squares within 4 RTOL.  The parameter gradients by
``check_grads``.  ``POOL_GAP`` = 1e-5 is asserted on the restatement's res1 in every case: a max-pool near-tie reroutes a whole
row of ``dx``.  Between paths (with and without an input gradient, group against single call, the same call twice) the bar is
the bits: the same device code runs in the same order with fixed partitions.

Launch counts of one backward (``_lib.prof_begin`` / ``prof_end`` count the profiler scopes of a family), recorded from the
parent commit (which has no input gradient) at geometry rows 2 and 4 with forced masks:
  row 2 (D 16, C 48, three layers, convolution shortcut): train_attnpool 1, train_bn_reduce 15, train_transpose 36,
        train_wgrad_gemm 14, train_dgrad_gemm 6, train_elementwise 13, lstm_bwd_recurrent 3
  row 4 (D = C = 64, two layers, identity shortcut):      train_attnpool 1, train_bn_reduce 12, train_transpose 28,
        train_wgrad_gemm 10, train_dgrad_gemm 5, train_elementwise 11, lstm_bwd_recurrent 2
With an input gradient: + 1 train_elementwise (the flip of W1) and + 2 train_dgrad_gemm (the shortcut's 1x1 data gradient and
the k = 3 data gradient with the residual epilogue); + 1 and + 1 with the identity shortcut."""
import copy
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
from cnnlstm_support import RTOL, bits, build, check_grads, device_masks, launches, same  # noqa: E402
from test_cnnlstm_train_group_gpu import make_replica, same_step, state_of  # noqa: E402
from weights import sample_tensor, synth_input  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "cnnlstm_input_grad_*.npz")))
PARENT_BACKWARD = {
    2: {"train_attnpool": 1, "train_bn_reduce": 15, "train_transpose": 36, "train_wgrad_gemm": 14, "train_dgrad_gemm": 6,
        "train_elementwise": 13, "lstm_bwd_recurrent": 3},
    4: {"train_attnpool": 1, "train_bn_reduce": 12, "train_transpose": 28, "train_wgrad_gemm": 10, "train_dgrad_gemm": 5,
        "train_elementwise": 11, "lstm_bwd_recurrent": 2},
}
WITH_DX = {2: {"train_elementwise": 1, "train_dgrad_gemm": 2}, 4: {"train_elementwise": 1, "train_dgrad_gemm": 1}}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def step(m, x_host, labels, requires_grad=True, profile=False):
    """One training step through ``model(x)``; ``dx``: x.grad (None when the input does not require one)."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    m.zero_grad()
    x = dev(x_host).requires_grad_(requires_grad)
    out = m(x)
    loss = torch.nn.CrossEntropyLoss()(out, dev(np.asarray(labels)))
    if profile:
        torch.cuda.synchronize()
        _lib.prof_begin()
    loss.backward()
    torch.cuda.synchronize()
    res = dict(state_of(m), logits=out.detach().cpu().numpy(), loss=loss.item(), dx=x.grad)
    if profile:
        res["prof"] = {k: v["launches"] for k, v in _lib.prof_end().items()}
    return res


def test_input_receives_a_gradient(rsaf_lib):
    """What failed before: ``x.grad is None`` after ``loss.backward()``, and a module in front of the drop-in never learned."""
    import torch
    case = igc.DX_CASES[0]
    sd, x, labels, mk = igc.setup(case)
    m = igc.model_of(case)
    m.forced_masks = device_masks(mk)
    got = step(m, x, labels)
    assert got["dx"] is not None and got["dx"].dtype == torch.float32 and got["dx"].shape == x.shape and got["dx"].is_cuda
    assert torch.isfinite(got["dx"]).all() and got["dx"].abs().max() > 0
    # a leaf behind other ops receives it through them
    m.zero_grad()
    scale = torch.ones(x.shape[2], device="cuda", requires_grad=True)
    m(dev(x) * scale).square().sum().backward()
    assert scale.grad is not None and scale.grad.shape == (x.shape[2],) and scale.grad.abs().max() > 0
    # eval mode builds no graph, for the input as for the parameters
    m.eval()
    out = m(dev(x).requires_grad_(True))
    assert not out.requires_grad


_runs = {}


def guarded_run(case):
    """The step of a case with forced masks, once for the tests that read it: workspace, training scratch, ``dx`` and
    ``dx_scratch`` are the size the ABI asks for followed by a guard tail, which must keep its pattern."""
    import torch
    from robust_speech_analysis_framework_amd import _lib, cnnlstm_train
    if case in _runs:
        return _runs[case]
    D, C, H, act, NC, L = igc.dims_of(case)
    sd, x, labels, mk = igc.setup(case)
    B, T = x.shape[:2]
    m = igc.model_of(case)
    m.forced_masks = device_masks(mk)
    check = geo.guard_buffers(m, B, T)
    n_scr = int(_lib.load().rsaf_cnnlstm_train_dx_scratch_floats(D, C))
    assert n_scr == (D * 3 * C + 3) // 4 * 4
    dx_scr, dx_buf = geo.guarded(n_scr), geo.guarded(B * T * D)
    m._train_dx_scratch = dx_scr
    new_dx, cnnlstm_train._new_dx = cnnlstm_train._new_dx, lambda t: dx_buf[:t.numel()].view(t.shape)
    try:
        got = step(m, x, labels)
    finally:
        cnnlstm_train._new_dx = new_dx
    check()
    assert m._train_dx_scratch is dx_scr, "a dx_scratch that was large enough has been replaced"
    for name, buf in (("dx", dx_buf), ("dx_scratch", dx_scr)):
        tail = buf.view(torch.int32)[-geo.GUARD_FLOATS:].cpu().numpy()
        assert (tail == geo.GUARD_PATTERN).all(), f"{name}: written behind the requested size"
    dx = got["dx"].cpu().numpy()
    same(dx_buf[:dx.size].cpu().numpy().view(np.uint32), dx.reshape(-1).view(np.uint32), "x.grad against the buffer the kernels wrote")
    assert not (dx.view(np.uint32) == geo.GUARD_PATTERN).any(), "a float of dx was not written"
    _runs[case] = dict(got, dx=dx)
    return _runs[case]


@pytest.mark.parametrize("case", igc.DX_CASES, ids=igc.dx_case_id)
def test_dx_matches_the_float64_restatement(rsaf_lib, case):
    want = igc.restated_case(case)
    gap = geo.pool_gap(want["stages"]["res1"])
    assert gap >= igc.POOL_GAP, gap
    got = guarded_run(case)
    scale = np.abs(want["dx"]).max()
    err = np.abs(got["dx"] - want["dx"]).max() / scale
    e_logits = np.abs(got["logits"] - want["logits"]).max() / max(np.abs(want["logits"]).max(), 1.0)
    print(f"{igc.dx_case_id(case)}: dx {err:.2e} of max|dx| = {scale:.2e}, logits {e_logits:.2e}, pool gap {gap:.2e}")
    assert got["dx"].shape == want["dx"].shape
    assert err < RTOL, err
    assert e_logits < RTOL and abs(got["loss"] - want["loss"]) < RTOL


@pytest.mark.parametrize("case", igc.DX_CASES, ids=igc.dx_case_id)
def test_parameter_gradients_beside_dx_match_the_float64_restatement(rsaf_lib, case):
    """The parameter gradients of the same steps by ``check_grads``.

    (B, T) = (1, 4) leaves block 2 two values per channel to normalise over.  There BatchNorm's backward is
    (dz_a - dz_b) / 2 * eps / (var + eps), and the general float32 form loses the small factor to the cancellation in
    1 - xhat^2: row 0 was 2.4e-4 to 3.9e-4 off in three tensors of block 2 (stock torch in float32: 0.8e-4 to 1.25e-4 on the
    same inputs).  The step forms the factor directly for a BatchNorm over two rows (``bn_bwd_pair_kernel``); measured with
    it on the MI355X: 3.2e-6 at row 0, 2.7e-5 at row 4."""
    want = igc.restated_case(case)
    assert geo.pool_gap(want["stages"]["res1"]) >= igc.POOL_GAP
    got = guarded_run(case)
    errs = {k: np.abs(got["grads"][k] - g).max() / max(np.abs(g).max(), 1e-7) for k, g in want["grads"].items()
            if not k.endswith(("conv1.bias", "conv2.bias", "shortcut.0.bias", "attention_weights.bias"))}
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print(f"{igc.dx_case_id(case)}: worst parameter gradients " + ", ".join(f"{k} {v:.2e}" for k, v in top))
    check_grads(got["grads"], want["grads"])


@pytest.mark.parametrize("case", igc.PAIR_CASES, ids=igc.dx_case_id)
def test_batchnorm_over_two_rows_keeps_the_bar(rsaf_lib, case):
    """Block 2 normalising over B T' = 2 values per channel (``bn_bwd_pair_kernel``) at further geometries: every parameter
    gradient by ``check_grads`` and ``dx`` within RTOL, with and without an input gradient the same bits."""
    want = igc.restated_case(case)
    assert geo.pool_gap(want["stages"]["res1"]) >= igc.POOL_GAP
    sd, x, labels, mk = igc.setup(case)
    assert x.shape[0] * (x.shape[1] // 2) == 2
    models = [igc.model_of(case) for _ in range(2)]
    for m in models:
        m.forced_masks = device_masks(mk)
    got, plain = step(models[0], x, labels), step(models[1], x, labels, requires_grad=False)
    same_step(got, plain, f"{igc.dx_case_id(case)} with against without an input gradient")
    err = np.abs(got["dx"].cpu().numpy() - want["dx"]).max() / np.abs(want["dx"]).max()
    worst = check_grads(got["grads"], want["grads"])
    print(f"{igc.dx_case_id(case)}: dx {err:.2e}, worst parameter gradient {worst[1]:.2e} ({worst[0]})")
    assert err < RTOL, err


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[19:-4] for p in GOLDEN])
def test_dx_matches_reference_vectors(rsaf_lib, path):
    z = np.load(path)
    t = np.load(path.replace("cnnlstm_input_grad_", "cnnlstm_train_"))
    D, C, H, B, T, seed = [int(v) for v in z["meta"]]
    m, _ = build(D, C, H, seed, str(z["act"]))
    got = step(m, synth_input(B, T, D, seed + 1000), t["labels"])
    assert np.abs(got["logits"] - t["logits"]).max() < RTOL * max(np.abs(t["logits"]).max(), 1.0)
    ref, s = z["dx"], sample_tensor(got["dx"].cpu().numpy())
    err = np.abs(s[:-2] - ref[:-2]).max() / max(np.abs(ref[:-2]).max(), 1e-7)
    print(f"{os.path.basename(path)}: dx samples {err:.2e} of the largest, sum of squares {abs(s[-1] - ref[-1]) / ref[-1]:.2e}")
    assert err < RTOL, err
    assert abs(s[-1] - ref[-1]) <= 4 * RTOL * max(abs(ref[-1]), 1e-12)


@pytest.mark.parametrize("i", [2, 4, 10], ids=geo.case_id)
def test_parameter_gradients_keep_their_bits_and_dx_repeats(rsaf_lib, i):
    case = igc.DX_CASES[i]
    sd, x, labels, mk = igc.setup(case)
    models = [igc.model_of(case) for _ in range(3)]
    for m in models:
        m.forced_masks = device_masks(mk)
    plain = step(models[0], x, labels, requires_grad=False)
    first, second = step(models[1], x, labels), step(models[2], x, labels)
    assert plain["dx"] is None
    same_step(first, plain, f"{geo.case_id(i)} with against without an input gradient")
    same(bits(first["dx"]), bits(second["dx"]), "dx of the same call twice")
    # and again on a model that has stepped before: the cached scratch is reused
    same(bits(step(models[1], x, labels)["dx"]), bits(first["dx"]), "dx of a second step of one model")


def group_dx(reps, wants, mixed):
    """One group step; ``wants[k]``: input k requires a gradient.  Returns the per-replica results with ``dx``."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_group
    models = [r["model"] for r in reps]
    for m in models:
        m.zero_grad()
    xs = [dev(r["x"]).requires_grad_(w) for r, w in zip(reps, wants)]
    outs = cnnlstm_train_group(models, xs, masks=[device_masks(r["masks"]) for r in reps], mixed=mixed)
    ce = torch.nn.CrossEntropyLoss()
    losses = [ce(o, dev(r["labels"])) for o, r in zip(outs, reps)]
    torch.stack(losses).sum().backward()
    torch.cuda.synchronize()
    return [dict(state_of(m), logits=o.detach().cpu().numpy(), loss=ls.item(), dx=x.grad) for m, o, ls, x in zip(models, outs, losses, xs)]


@pytest.mark.parametrize("mixed", [False, True], ids=["one_architecture", "mixed"])
def test_group_dx_equals_the_single_calls_bit_for_bit(rsaf_lib, mixed):
    """Replicas that share D = 16, two classes and two layers; ``mixed``: different C, H and activation, one of them with the
    identity shortcut (C = D).  First every input requires a gradient, then only some."""
    archs = [(32, 64, "silu"), (48, 128, "gelu"), (16, 64, "gelu")] if mixed else [(32, 64, "silu")] * 3
    shapes = [(3, 9), (2, 12), (4, 6)]
    reps = [make_replica(16, C, H, act, B, T, 9900 + 10 * k) for k, ((C, H, act), (B, T)) in enumerate(zip(archs, shapes))]
    singles = []
    for r in reps:
        m = copy.deepcopy(r["model"])
        m.forced_masks = device_masks(r["masks"])
        singles.append(step(m, r["x"], r["labels"]))
    for wants in ([True, True, True], [False, True, False], [True, False, True]):
        got = group_dx([dict(r, model=copy.deepcopy(r["model"])) for r in reps], wants, mixed)
        for k, (g, s, w) in enumerate(zip(got, singles, wants)):
            same_step(g, s, f"replica {k} of the group {wants}")
            if w:
                same(bits(g["dx"]), bits(s["dx"]), f"dx of replica {k} of the group {wants}")
            else:
                assert g["dx"] is None


@pytest.mark.parametrize("i", [2, 4], ids=geo.case_id)
def test_backward_launches(rsaf_lib, i):
    case = igc.DX_CASES[i]
    sd, x, labels, mk = igc.setup(case)
    m = igc.model_of(case)
    m.forced_masks = device_masks(mk)
    plain = step(m, x, labels, requires_grad=False, profile=True)["prof"]
    with_dx = step(m, x, labels, profile=True)["prof"]
    print(f"{geo.case_id(i)}: backward {plain}; with an input gradient {with_dx}")
    assert plain == PARENT_BACKWARD[i]
    assert with_dx == {k: v + WITH_DX[i].get(k, 0) for k, v in PARENT_BACKWARD[i].items()}


def test_fused_step_refuses_an_input_that_requires_grad(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, cnnlstm_train_step_group
    reps = [make_replica(16, 32, 64, "silu", B, T, 9950 + 10 * k) for k, (B, T) in enumerate([(3, 9), (2, 12)])]
    twins = [dict(r, model=copy.deepcopy(r["model"])) for r in reps]

    def run(rs, grad_on=None):
        models = [r["model"] for r in rs]
        opts = [FusedAdam(m, lr=1e-3) for m in models]
        xs = [dev(r["x"]).requires_grad_(k == grad_on) for k, r in enumerate(rs)]
        return cnnlstm_train_step_group(models, opts, xs, [dev(r["labels"]) for r in rs], masks=[device_masks(r["masks"]) for r in rs])

    before = [state_of(r["model"])["buffers"] for r in reps]
    params = [[bits(p) for p in r["model"].parameters()] for r in reps]
    with pytest.raises(ValueError, match="cnnlstm_train_group") as e:
        run(reps, grad_on=1)
    assert "replica 1" in str(e.value) and "cnnlstm_train_step_group" in str(e.value)
    for r, b, ps in zip(reps, before, params):                         # refused before anything ran
        for k, v in state_of(r["model"])["buffers"].items():
            same(v, b[k], k)
        for p, q in zip(r["model"].parameters(), ps):
            same(bits(p), q, "parameter")
    losses, logits = run(reps)
    losses2, logits2 = run(twins)
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and len(logits) == 2
    same(bits(losses), bits(losses2), "losses of the fused step")
    for a, b in zip(logits, logits2):
        same(bits(a), bits(b), "logits of the fused step")
    for r, t in zip(reps, twins):
        for p, q in zip(r["model"].parameters(), t["model"].parameters()):
            same(bits(p), bits(q), "parameter after the fused step")
