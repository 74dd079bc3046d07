"""The mix inside the collate launch on the MI355X (``rsaf_collate_mix_group`` / ``rsaf_collate_mix_backward_group``): layer stacks
resident in a ``DeviceSequenceStore(layers=L)``, the mixed padded batch and dL/dp without the padded stack.

The oracle is the dense path on the zero-padded stack ``h [B, L, T, D]`` that iterating the layered loader yields (itself compared
with the stack padded on the host, bit for bit): forward and backward must have the BITS of ``layer_mix_forward(h, p)`` and
``layer_mix_backward(h, dx)``.  The float64 bars are those of tests/test_layer_mix_gpu.py, derived there:
forward |x - x64| <= 2 L 2^-24 sum_l p_l |h_l| elementwise; backward |dp_l - dp64_l| <= 2^-24 |dp64_l| + 2 n 2^-53 sum|h_l dx|,
n = B T D.  Shapes: tests/collate_mix_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import collate_mix_cases as cmc  # noqa: E402
import input_grad_restatement as igr  # noqa: E402
from cnnlstm_support import bits, same  # noqa: E402

pytestmark = pytest.mark.gpu

RSAF_ERR_WORKSPACE = 3
_cache = {}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def resident(case):
    """(store, loader, plan of its one batch, h_padded from iterating the loader, labels) of a case, built once."""
    if case not in _cache:
        import torch
        from robust_speech_analysis_framework_amd.cnnlstm import DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore
        lengths, L, D = case
        seqs = cmc.stacks(case)[0]
        store = DeviceSequenceStore(seqs, layers=L)
        labels = np.arange(len(lengths)) % 3
        loader = DeviceBatchLoader(DeviceSequenceDataset(store, labels), batch_size=len(lengths))
        (h, lab), = list(loader)
        torch.cuda.synchronize()
        _cache[case] = (store, loader, next(loader.plans()), h, lab)
    return _cache[case]


@pytest.mark.parametrize("case", cmc.CASES + cmc.GROUP_CASES[1:2], ids=cmc.case_id)
def test_store_and_padded_stack(rsaf_lib, case):
    """The store keeps every block as it lay in memory, and the loader's stack is the host's zero-padded one, bit for bit."""
    import torch
    lengths, L, D = case
    seqs, _, _, h = cmc.stacks(case)
    store, loader, plan, hd, lab = resident(case)
    assert store.layers == L and store.width == D and store.arena.shape == (L * sum(lengths), D)
    assert store.lengths.tolist() == list(lengths) and store.frame_off.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    for i, s in enumerate(seqs):
        assert store.sequence(i).shape == (L, lengths[i], D)
        same(bits(store.sequence(i)), s.view(np.uint32), f"sequence {i}")
        row = L * int(store.frame_off[i])
        same(bits(store.arena[row:row + L * lengths[i]]), s.reshape(-1, D).view(np.uint32), f"block {i}")
    assert plan.layers == L and plan.B == len(lengths) and plan.T == max(lengths) and plan.frames == sum(lengths)
    assert hd.shape == h.shape and hd.dtype == torch.float32 and hd.is_contiguous()
    same(bits(hd), h.view(np.uint32), "padded stack")
    assert lab.dtype == torch.int64 and lab.cpu().tolist() == (np.arange(len(lengths)) % 3).tolist()


@pytest.mark.parametrize("case", cmc.CASES, ids=cmc.case_id)
def test_forward_has_the_bits_of_the_dense_mix(rsaf_lib, case):
    import torch
    from robust_speech_analysis_framework_amd.layer_mix import layer_mix_forward
    from robust_speech_analysis_framework_amd.layer_mix_train import collate_mix_forward
    lengths, L, D = case
    _, p, _, h = cmc.stacks(case)
    store, loader, plan, hd, lab = resident(case)
    pd = dev(p)
    (x, xl), = collate_mix_forward([plan], [pd])
    want = layer_mix_forward(hd, pd)
    torch.cuda.synchronize()
    assert x.shape == (len(lengths), max(lengths), D) and x.dtype == torch.float32
    same(bits(x), bits(want), "mixed batch against layer_mix_forward on the padded stack")
    assert torch.equal(xl, lab)
    xb = bits(x)
    for b, n in enumerate(lengths):
        assert not xb[b, n:].any(), f"padding of member {b} is not +0.0"
    p64 = p.astype(np.float64)
    bar = 2 * L * 2.0 ** -24 * np.einsum("l,bltd->btd", p64, np.abs(h.astype(np.float64)))
    err = np.abs(x.cpu().numpy() - igr.layer_mix(h, p64))
    print(f"{cmc.case_id(case)}: worst |x - x64| / bar {np.max(err / np.maximum(bar, 1e-300)):.3f}")
    assert (err <= bar).all(), float(np.max(err / np.maximum(bar, 1e-300)))


def test_one_layer_with_p_one_is_the_plain_collate(rsaf_lib):
    from robust_speech_analysis_framework_amd.cnnlstm import DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore
    from robust_speech_analysis_framework_amd.layer_mix_train import collate_mix_forward
    case = cmc.CASES[0]
    lengths, L, D = case
    assert L == 1
    seqs = cmc.stacks(case)[0]
    plan = resident(case)[2]
    (x, _), = collate_mix_forward([plan], [dev(np.ones(1, np.float32))])
    plain = DeviceSequenceStore([s[0] for s in seqs])
    assert plain.layers is None
    (want, _), = list(DeviceBatchLoader(DeviceSequenceDataset(plain, np.zeros(len(lengths), np.int64)), batch_size=len(lengths)))
    same(bits(x), bits(want), "L = 1, p = [1] against rsaf_collate_pad_group")


def test_a_block_outside_the_arena_gives_zeros(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd.device_data import BatchPlan
    from robust_speech_analysis_framework_amd.layer_mix_train import collate_mix_forward, collate_mix_backward
    case = cmc.CASES[1]
    lengths, L, D = case
    _, p, dx, h = cmc.stacks(case)
    store, loader, plan, hd, lab = resident(case)
    rows = int(store.arena.shape[0])
    pd = dev(p)
    (ref, _), = collate_mix_forward([plan], [pd])
    for b, start in ((0, -1), (1, rows - L * lengths[1] + 1), (2, rows), (0, -(1 << 40)), (2, 1 << 40)):
        rs = plan.row_start.clone()
        rs[b] = start
        moved = BatchPlan(plan.dataset, rs, plan.row_count, plan.label_index, 0, plan.B, plan.T, plan.frames, None, L)
        (x, _), = collate_mix_forward([moved], [pd])
        want = ref.clone()
        want[b] = 0
        same(bits(x), bits(want), f"member {b} at row {start}")
        hz = hd.clone()
        hz[b] = 0
        from robust_speech_analysis_framework_amd.layer_mix import layer_mix_backward
        dp, = collate_mix_backward([moved], [dev(dx)])
        same(bits(dp), bits(layer_mix_backward(hz, dev(dx))), f"dp with member {b} at row {start}")
    torch.cuda.synchronize()


def test_one_call_over_three_items_equals_three_calls(rsaf_lib):
    from robust_speech_analysis_framework_amd.layer_mix_train import collate_mix_backward, collate_mix_forward
    plans = [resident(c)[2] for c in cmc.GROUP_CASES]
    ps = [dev(cmc.stacks(c)[1]) for c in cmc.GROUP_CASES]
    dxs = [dev(cmc.stacks(c)[2]) for c in cmc.GROUP_CASES]
    assert [p.layers for p in plans] == [2, 13, 32]
    from robust_speech_analysis_framework_amd import _lib
    _lib.prof_begin()
    together = collate_mix_forward(plans, ps)
    dps = collate_mix_backward(plans, dxs)
    prof = _lib.prof_end()
    assert prof["train_collate_mix"]["launches"] == 1 and prof["train_collate_mix_backward"]["launches"] == 2
    for k, (plan, p, dx) in enumerate(zip(plans, ps, dxs)):
        (x, lab), = collate_mix_forward([plan], [p])
        same(bits(together[k][0]), bits(x), f"item {k} of the K = 3 forward")
        assert together[k][1].tolist() == lab.tolist()
        dp, = collate_mix_backward([plan], [dx])
        same(bits(dps[k]), bits(dp), f"item {k} of the K = 3 backward")


@pytest.mark.parametrize("case", cmc.CASES, ids=cmc.case_id)
def test_backward_has_the_bits_of_the_dense_sums_and_repeats(rsaf_lib, case):
    import torch
    from robust_speech_analysis_framework_amd.layer_mix import layer_mix_backward
    from robust_speech_analysis_framework_amd.layer_mix_train import collate_mix_backward
    lengths, L, D = case
    _, _, dx, h = cmc.stacks(case)
    store, loader, plan, hd, lab = resident(case)
    dxd = dev(dx)
    dp, = collate_mix_backward([plan], [dxd])
    again, = collate_mix_backward([plan], [dxd])
    want = layer_mix_backward(hd, dxd)
    torch.cuda.synchronize()
    assert dp.shape == (L,) and dp.dtype == torch.float32
    same(bits(dp), bits(again), "dp of two calls")
    same(bits(dp), bits(want), "dp against layer_mix_backward on the padded stack")
    dp64, mag = igr.layer_mix_dp(h, dx)
    bar = 2.0 ** -24 * np.abs(dp64) + 2 * h[:, 0].size * 2.0 ** -53 * mag
    err = np.abs(dp.cpu().numpy().astype(np.float64) - dp64)
    print(f"{cmc.case_id(case)}: worst |dp - dp64| / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all(), (err / bar).max()


def test_short_partials_are_refused(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    case = cmc.CASES[4]
    lengths, L, D = case
    store, loader, plan, hd, lab = resident(case)
    n = rsaf_lib.rsaf_layer_mix_partials(plan.B, L, plan.T, D)
    assert n == 129 * L
    part = torch.empty(n, dtype=torch.float64, device="cuda")
    dp = torch.empty(L, dtype=torch.float32, device="cuda")
    dx = dev(cmc.stacks(case)[2])
    it = _lib.CollateMixBackwardItem()
    it.arena, it.arena_rows = store.arena.data_ptr(), int(store.arena.shape[0])
    it.row_start, it.row_count = plan.row_start.data_ptr(), plan.row_count.data_ptr()
    it.B, it.T, it.L, it.dx, it.dp_out, it.frames = plan.B, plan.T, L, dx.data_ptr(), dp.data_ptr(), plan.frames
    it.partials, it.partials_count = part.data_ptr(), n - 1
    assert rsaf_lib.rsaf_collate_mix_backward_group(C.pointer(it), 1, D, _lib.stream_ptr(None)) == RSAF_ERR_WORKSPACE
    assert b"rsaf_layer_mix_partials" in rsaf_lib.rsaf_last_error()


@pytest.mark.parametrize("case", cmc.CASES[1:3], ids=cmc.case_id)
def test_collate_mix_batches_is_layer_mix_on_the_padded_stack(rsaf_lib, case):
    """Through the public names: x and weights.grad of ``collate_mix_batches`` have the bits of ``LayerMix(h_padded)``."""
    import torch
    from src.models import LayerMix, collate_mix_batches
    lengths, L, D = case
    _, p, dx, _ = cmc.stacks(case)
    store, loader, plan, hd, lab = resident(case)
    mix, twin = LayerMix(L).cuda(), LayerMix(L).cuda()
    with torch.no_grad():
        mix.weights.copy_(dev(np.log(p)))
        twin.weights.copy_(mix.weights)
    (x, xl), = collate_mix_batches([plan], [mix])
    assert x.requires_grad and torch.equal(xl, lab)
    want = twin(hd)
    same(bits(x), bits(want), "x")
    x.backward(dev(dx))
    want.backward(dev(dx))
    same(bits(mix.weights.grad), bits(twin.weights.grad), "weights.grad")
    with torch.no_grad():
        (y, _), = collate_mix_batches([plan], [mix])
    assert not y.requires_grad
    same(bits(y), bits(want), "x under no_grad")


def test_python_refusals(rsaf_lib):
    from robust_speech_analysis_framework_amd.cnnlstm import (AugmentStream, DeviceBatchLoader, DeviceSequenceDataset,
                                                               DeviceSequenceStore, Scale)
    from src.models import LayerMix, collate_mix_batches
    case = cmc.CASES[1]
    store, loader, plan, hd, lab = resident(case)
    with pytest.raises(ValueError, match="num_layers=3.*layers=2"):
        collate_mix_batches([plan], [LayerMix(3).cuda()])
    with pytest.raises(ValueError, match="is on 'cpu'"):
        collate_mix_batches([plan], [LayerMix(2)])
    plain = DeviceSequenceStore([s[0] for s in cmc.stacks(case)[0]])
    plain_plan = next(DeviceBatchLoader(DeviceSequenceDataset(plain, np.zeros(3, np.int64)), batch_size=3).plans())
    with pytest.raises(ValueError, match="plain DeviceSequenceStore"):
        collate_mix_batches([plain_plan], [LayerMix(2).cuda()])
    with pytest.raises(ValueError, match="transform is not supported over a store of layer stacks"):
        DeviceSequenceDataset(store, np.zeros(3, np.int64), transform=Scale(0.9, 1.1), augment_stream=AugmentStream(1))
