"""``LayerMix`` on the MI355X: the softmax-weighted sum of encoder layers (``rsaf_layer_mix_forward``) and the gradient of the
loss with respect to the mixing probabilities (``rsaf_layer_mix_backward``), alone and in front of the CNN-LSTM.

Bars, both from the arithmetic and not from the code under test.
Forward, against the float64 sum with the device's own p: |x - x64| <= 2 L 2^-24 sum_l p_l |h_l|, elementwise: one rounding
per product and per add (L products, L - 1 adds, each at most 2^-24 of a partial sum that sum_l p_l |h_l| bounds); it holds
with or without FMA contraction.  L = 1 with p = [1] returns h bit for bit.
Backward: |dp_l - dp64_l| <= 2^-24 |dp64_l| + 2 n 2^-53 sum|h_l dx|, n = B T D: a product of two floats is exact in double,
a double sum of n terms is off by at most (n - 1) 2^-53 of the sum of magnitudes to first order, one final rounding to float,
a factor 2 of margin.  Two calls give the same bits (fixed partition, no atomics).
End to end: dL/dp within ``cnnlstm_support.RTOL`` of max|dp64|, the CNN-LSTM's gradients by ``check_grads``; the mixed input
keeps ``POOL_GAP`` on the restatement (asserted here and, without a GPU, in tests/test_cnnlstm_input_grad.py).

Shapes (B, L, T, D): L of 1, 2, 13 and 25; D of 4, 20 and 768; float4 counts that are no multiple of 256 (10, 105, 165,
14 208); 524 928 float4, more than the 2 048 x 256 threads of a launch and 129 parts of the backward."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cnnlstm_geometry as geo  # noqa: E402
import input_grad_cases as igc  # noqa: E402
import input_grad_restatement as igr  # noqa: E402
from cnnlstm_support import RTOL, bits, check_grads, device_masks, same  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 5, 4), (3, 2, 7, 20), (2, 13, 37, 768), (1, 25, 33, 20), (1, 1, 3, 768), (2, 2, 1367, 768)]
_cache = {}


def shape_id(s):
    return "b%d_l%d_t%d_d%d" % s


def data(shape):
    """(h, dx, weights) of a shape from numpy PCG64 streams, computed once."""
    if shape not in _cache:
        B, L, T, D = shape
        rng = np.random.Generator(np.random.PCG64(9600 + 7 * L + D + T))
        _cache[shape] = (rng.standard_normal((B, L, T, D)).astype(np.float32),
                         (1e-3 * rng.standard_normal((B, T, D))).astype(np.float32), rng.uniform(-1.5, 1.5, L).astype(np.float32))
    return _cache[shape]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_forward_matches_the_float64_sum(rsaf_lib, shape):
    import torch
    from src.models import LayerMix
    B, L, T, D = shape
    h, _, w = data(shape)
    mix = LayerMix(L).cuda()
    assert mix.weights.shape == (L,) and not mix.weights.detach().any()               # initialised to zeros
    with torch.no_grad():
        mix.weights.copy_(dev(w))
    x = mix(dev(h))
    p = torch.softmax(mix.weights.detach(), dim=0).cpu().numpy().astype(np.float64)    # the device's own p
    assert x.shape == (B, T, D) and x.dtype == torch.float32 and x.requires_grad
    h64 = h.astype(np.float64)
    bar = 2 * L * 2.0 ** -24 * np.einsum("l,bltd->btd", p, np.abs(h64))
    err = np.abs(x.detach().cpu().numpy() - igr.layer_mix(h, p))
    print(f"{shape_id(shape)}: worst |x - x64| / bar {np.max(err / np.maximum(bar, 1e-300)):.3f}")
    assert (err <= bar).all(), float(np.max(err / np.maximum(bar, 1e-300)))
    if L == 1:
        assert p[0] == 1.0
        same(bits(x), h[:, 0].view(np.uint32), "L = 1 returns h")


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_backward_matches_the_float64_sums_and_repeats(rsaf_lib, shape):
    import torch
    from robust_speech_analysis_framework_amd.layer_mix import LayerMix, layer_mix_backward
    B, L, T, D = shape
    h, dx, w = data(shape)
    hd, dxd = dev(h), dev(dx)
    dp = layer_mix_backward(hd, dxd)
    again = layer_mix_backward(hd, dxd)
    assert dp.shape == (L,) and dp.dtype == torch.float32
    same(bits(dp), bits(again), "dp of two calls")
    dp64, mag = igr.layer_mix_dp(h, dx)
    bar = 2.0 ** -24 * np.abs(dp64) + 2 * (B * T * D) * 2.0 ** -53 * mag
    err = np.abs(dp.cpu().numpy().astype(np.float64) - dp64)
    print(f"{shape_id(shape)}: worst |dp - dp64| / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all(), (err / bar).max()
    # through the module: weights.grad is torch's softmax Jacobian applied to that dp
    mix = LayerMix(L).cuda()
    with torch.no_grad():
        mix.weights.copy_(dev(w))
    mix(hd).backward(dxd)
    wt = dev(w).requires_grad_(True)
    torch.softmax(wt, dim=0).backward(dp)
    same(bits(mix.weights.grad), bits(wt.grad), "weights.grad")


def test_gradient_of_h_is_the_outer_product(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd.layer_mix import layer_mix
    shape = SHAPES[1]
    h, dx, w = data(shape)
    hd = dev(h).requires_grad_(True)
    p = torch.softmax(dev(w), dim=0)
    layer_mix(hd, p).backward(dev(dx))
    want = p.cpu().numpy()[None, :, None, None] * dx[:, None]
    same(bits(hd.grad), want.view(np.uint32), "h.grad")


def test_arguments_are_checked(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.layer_mix import LayerMix
    for bad in (0, 33):
        with pytest.raises(ValueError):
            LayerMix(bad)
    mix = LayerMix(3).cuda()
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        mix(torch.zeros(1, 3, 2, 4))
    for shape in ((1, 2, 2, 4), (1, 3, 2, 6), (3, 2, 4)):
        with pytest.raises(ValueError):
            mix(torch.zeros(shape, device="cuda"))
    with pytest.raises(ValueError):
        mix(torch.zeros((1, 3, 2, 4), device="cuda", dtype=torch.float64))


@pytest.mark.parametrize("i", igc.MIX_ROWS, ids=geo.case_id)
def test_layer_mix_in_front_of_the_cnnlstm(rsaf_lib, i):
    """One step of LayerMix(3) in front of CNNLSTM: the mix learns (dL/dp through the input gradient of the training step)."""
    import torch
    from src.models import LayerMix
    from robust_speech_analysis_framework_amd.layer_mix import layer_mix
    e = igc.mix_case(i)
    want = e["want"]
    gap = geo.pool_gap(want["stages"]["res1"])
    assert gap >= igc.POOL_GAP, gap
    m = geo.model_of(i, e["sd"], train=True)
    m.forced_masks = device_masks(e["masks"])
    mix = LayerMix(igc.MIX_L).cuda()
    with torch.no_grad():
        mix.weights.copy_(dev(np.asarray(igc.MIX_WEIGHTS, np.float32)))
    p = torch.softmax(mix.weights, dim=0)
    p.retain_grad()
    out = m(layer_mix(dev(e["h"]), p))
    loss = torch.nn.CrossEntropyLoss()(out, dev(np.asarray(e["labels"])))
    loss.backward()
    torch.cuda.synchronize()
    dp = p.grad.cpu().numpy().astype(np.float64)
    err = np.abs(dp - e["dp64"]).max() / np.abs(e["dp64"]).max()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in m.named_parameters()}
    worst = check_grads(grads, want["grads"])
    print(f"layer mix in front of {geo.case_id(i)}: dL/dp {err:.2e} of max|dp64| = {np.abs(e['dp64']).max():.2e}, "
          f"worst gradient {worst[1]:.2e} ({worst[0]}), pool gap {gap:.2e}")
    assert err < RTOL, err
    assert abs(loss.item() - want["loss"]) < RTOL
    assert mix.weights.grad is not None and torch.isfinite(mix.weights.grad).all() and mix.weights.grad.abs().max() > 0
    # the module itself gives the same step
    m.zero_grad()
    mix.weights.grad = None
    torch.nn.CrossEntropyLoss()(m(mix(dev(e["h"]))), dev(np.asarray(e["labels"]))).backward()
    wt = mix.weights.detach().clone().requires_grad_(True)
    torch.softmax(wt, dim=0).backward(p.grad)
    same(bits(mix.weights.grad), bits(wt.grad), "weights.grad through the module")
