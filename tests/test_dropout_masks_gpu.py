"""Dropout masks from the counter-based generator on the MI355X: rsaf_dropout_masks_group against the NumPy restatement of
the mapping in include/rsaf.h (tests/dropout_restatement.py) bit for bit, its argument checks, ``DropoutStream`` /
``draw_masks_group`` at model level, and what the streams are for: training steps whose results do not depend on how the
replicas are grouped or ordered, and lock-step loops that equal sequential trainings bit for bit with dropout on.

Every comparison here is of bits: the masks are a pure integer function of (seed, step, slot, element) followed by one
select, and the group paths promise the bits of the single calls, so no tolerance applies anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dropout_restatement as dr  # noqa: E402
from test_cnnlstm_fused_step_gpu import bits, build, freeze_zero_grad, same  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "golden"))
from weights import synth_input  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 8
D, CH, H, B, T = 16, 32, 64, 2, 7


# ---- 1. the raw entry --------------------------------------------------------------------------------------------------
def call(items):
    from robust_speech_analysis_framework_amd import _lib
    arr = (_lib.DropoutItem * max(len(items), 1))()
    for it, (seed, step, slots) in zip(arr, items):
        it.seed, it.step = seed, step
        for slot, (ptr, n, p) in slots.items():
            it.mask[slot], it.n[slot], it.p[slot] = ptr, n, p
    return _lib.load().rsaf_dropout_masks_group(arr, len(items), _lib.stream_ptr(None))


def last_error():
    from robust_speech_analysis_framework_amd import _lib
    return _lib.load().rsaf_last_error().decode()


def sentinel_buffer(n):
    import torch
    return torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")


def test_raw_call_equals_the_restatement_and_stays_inside_its_masks():
    import torch
    plan = [   # (seed, step, {slot: (n, p)}): every n in every position, NULL slots, p = 1 and an odd p
        (dr.SEEDS[2], 1, {0: (1, 0.37), 1: (3, 0.37), 2: (5, 1.0), 3: (1023, 0.37), 4: (1025, 0.37), 5: (4099, 0.37)}),
        (dr.SEEDS[3], 2 ** 32 + 7, {0: (4099, 1.0), 2: (1023, 0.37), 4: (1, 0.37)}),
        (dr.SEEDS[1], 0, {1: (1025, 0.37), 3: (5, 0.37), 5: (3, 1.0)}),
    ]
    offs, total = {}, GUARD
    for k, (_, _, slots) in enumerate(plan):
        for slot, (n, _) in slots.items():
            offs[k, slot] = total
            total += (n + GUARD + 3) // 4 * 4                  # at least 8 sentinel floats behind every mask
    buf = sentinel_buffer(total)
    base = buf.data_ptr()
    assert base % 16 == 0
    rc = call([(seed, step, {slot: (base + 4 * offs[k, slot], n, p) for slot, (n, p) in slots.items()})
               for k, (seed, step, slots) in enumerate(plan)])
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    untouched = np.ones(total, dtype=bool)
    for k, (seed, step, slots) in enumerate(plan):
        for slot, (n, p) in slots.items():
            o = offs[k, slot]
            same(got[o:o + n].view(np.uint32), dr.mask(seed, step, slot, n, p).view(np.uint32), f"item {k} slot {slot} n {n} p {p}")
            assert np.all(got[o + n:o + n + GUARD] == np.float32(SENTINEL)), f"item {k} slot {slot}: wrote past mask + n"
            untouched[o:o + n] = False
    assert np.all(got[untouched] == np.float32(SENTINEL)), "a float outside every mask was written"


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    buf = sentinel_buffer(64)
    base = buf.data_ptr()
    ok = (5, 1, {0: (base, 8, 0.3)})
    cases = [
        ([], None, "K must be in [1, 16]"),
        ([ok] * 17, None, "K must be in [1, 16]"),
        ([ok, (5, 1, {3: (base + 64 + 4, 8, 0.3)})], (1, 3), "16-byte aligned"),
        ([ok, (5, 1, {2: (base + 64, 0, 0.3)})], (1, 2), "n >= 1"),
        ([(5, 1, {4: (base, 8, 0.0)})], (0, 4), "p > 0"),
        ([ok, (5, 1, {1: (base + 64, 8, float("nan"))})], (1, 1), "NaN"),
        ([ok, (5, 1, {0: (base + 128, 8, 0.3), 5: (base + 16, 8, 0.3)})], (1, 5), "overlaps the mask of item 0, slot 0"),
        ([(5, 1, {0: (base, 8, 0.3), 1: (base + 16, 8, 0.3)})], (0, 1), "overlaps the mask of item 0, slot 0"),
        ([(5, 1, {0: (base, 2 ** 32 + 1, 0.3)})], (0, 0), "n must be in [0, 2^32]"),
    ]
    for items, where, text in cases:
        assert call(items) == 1, (where, text)
        msg = last_error()
        assert text in msg, msg
        if where is not None:
            assert f"item {where[0]}: slot {where[1]}:" in msg, msg
    torch.cuda.synchronize()
    assert torch.all(buf == SENTINEL).item(), "a refused call wrote to a mask"
    # nothing to draw is no error (and no launch): NULL slots only
    assert call([(5, 1, {}), (6, 1, {0: (None, 0, 0.0)})]) == 0, last_error()


@pytest.mark.parametrize("p", [0.2, 0.3, 0.37, 0.5])
def test_kept_value_is_the_one_draw_masks_writes(p):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import draw_masks
    m, _ = build(D, CH, H, 900, "silu", p_rate=p, p_block=p)
    old = draw_masks(m, B, T, "cuda")["res_block1"]
    want = np.unique(bits(old[old != 0]))
    buf = torch.zeros(256, dtype=torch.float32, device="cuda")
    assert call([(1, 1, {0: (buf.data_ptr(), 256, p)})]) == 0, last_error()
    got = np.unique(bits(buf[buf != 0]))
    assert len(want) == 1 and np.array_equal(got, want), (p, got, want)
    assert got[0] == dr.keep_value(p).view(np.uint32)


# ---- 2. model level -----------------------------------------------------------------------------------------------------
def rates(m):
    return (float(m.res_block1.dropout.p), float(m.res_block2.dropout.p), float(m.lstm.dropout), float(m.dropout.p))


def assert_masks(got, want, what):
    assert sorted(got) == ["fc", "lstm", "res_block1", "res_block2"] and len(got["lstm"]) == len(want["lstm"]), what
    for key, g, w in [(k, got[k], want[k]) for k in ("res_block1", "res_block2", "fc")] + \
                     [(f"lstm{l}", g, w) for l, (g, w) in enumerate(zip(got["lstm"], want["lstm"]))]:
        if w is None:
            assert g is None, (what, key)
        else:
            assert tuple(g.shape) == w.shape and g.is_contiguous() and g.data_ptr() % 16 == 0, (what, key)
            same(bits(g), w.view(np.uint32), f"{what} {key}")


@pytest.mark.parametrize("layers", [1, 2, 4])
def test_draw_masks_group_at_model_level(layers):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import DropoutStream, draw_masks, draw_masks_group
    seeds = (dr.SEEDS[3], 77)
    models = [build(D, CH, H, 910 + k, "silu", p_rate=0.37, p_block=0.2, layers=layers)[0] for k in range(2)]
    models[1].res_block2.dropout.p = 0.0                              # a slot that is not drawn
    streams = [DropoutStream(s, step=5) for s in seeds]
    shapes = [(B, T), (3, 9)]
    want = lambda k, step: dr.model_masks(models[k].dims, *shapes[k], *rates(models[k]), seeds[k], step)     # noqa: E731
    first = draw_masks_group(models, shapes, streams, "cuda")
    state = [st.state_dict() for st in streams]
    assert state == [{"seed": s, "step": 6} for s in seeds]
    second = draw_masks_group(models, shapes, streams, "cuda")
    torch.cuda.synchronize()
    for k, m in enumerate(models):
        old = draw_masks(m, *shapes[k], "cuda")
        assert [None if old[key] is None else tuple(old[key].shape) for key in ("res_block1", "res_block2", "fc")] == \
               [None if first[k][key] is None else tuple(first[k][key].shape) for key in ("res_block1", "res_block2", "fc")]
        assert [tuple(t.shape) for t in old["lstm"]] == [tuple(t.shape) for t in first[k]["lstm"]] and len(old["lstm"]) == layers - 1
        assert_masks(first[k], want(k, 5), f"replica {k} step 5")
        assert_masks(second[k], want(k, 6), f"replica {k} step 6")
        assert not np.array_equal(bits(first[k]["res_block1"]), bits(second[k]["res_block1"]))
    assert models[1].res_block2.dropout.p == 0.0 and first[1]["res_block2"] is None
    for st in streams:
        st.load_state_dict({"seed": st.seed, "step": 5})
    again = draw_masks_group(models, shapes, streams, "cuda")
    for k in range(2):
        assert_masks(again[k], want(k, 5), f"replica {k} after load_state_dict")
    with pytest.raises(ValueError):
        DropoutStream(2 ** 64)
    with pytest.raises(ValueError):
        DropoutStream(-1)
    with pytest.raises(ValueError):
        draw_masks_group(models, shapes, [streams[0], streams[0]], "cuda")


def test_stream_leaves_the_torch_rng_alone_and_counts_consulted_steps():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import DropoutStream, draw_masks
    m, _ = build(D, CH, H, 920, "silu", p_rate=0.3, p_block=0.3)
    x = torch.from_numpy(synth_input(B, T, D, 921)).cuda()
    assert m.dropout_stream is None and "dropout_stream" not in " ".join(m.state_dict())
    before = torch.cuda.get_rng_state()
    m(x)
    assert not torch.equal(before, torch.cuda.get_rng_state()), "without a stream the masks come from torch's RNG"
    keys = sorted(m.state_dict())
    m.dropout_stream = DropoutStream(3)
    assert sorted(m.state_dict()) == keys
    before = torch.cuda.get_rng_state()
    out = m(x)
    out.sum().backward()
    assert torch.equal(before, torch.cuda.get_rng_state()), "a model with a stream drew from torch's RNG"
    assert m.dropout_stream.step == 1
    # not consulted: forced masks, eval mode, a model without dropout
    m.forced_masks = draw_masks(m, B, T, "cuda")
    m(x)
    m.forced_masks = None
    m.eval()
    m(x)
    assert m.dropout_stream.step == 1
    m.train()
    for mod in (m.res_block1.dropout, m.res_block2.dropout, m.dropout):
        mod.p = 0.0
    m.lstm.dropout = 0.0
    m(x)
    assert m.dropout_stream.step == 1


# ---- 3. grouping freedom --------------------------------------------------------------------------------------------------
SHAPES3 = [(4, 24), (3, 31), (5, 18)]


def three_replicas(seed, fused):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import DropoutStream, FusedAdam
    models, opts, xs, labs = [], [], [], []
    for k, (b, t) in enumerate(SHAPES3):
        m, _ = build(D, CH, H, seed + k, "silu", p_rate=0.3, p_block=0.3)
        freeze_zero_grad(m)
        m.dropout_stream = DropoutStream(1000 + k)
        models.append(m)
        opts.append(FusedAdam(m, lr=1e-3) if fused else None)
        xs.append(torch.from_numpy(synth_input(b, t, D, seed + 10 + k)).cuda())
        labs.append(torch.from_numpy(np.random.Generator(np.random.PCG64(seed + 20 + k)).integers(0, 2, b)).cuda())
    return models, opts, xs, labs


def state_bits(m):
    out = {k: bits(v) if v.dtype.is_floating_point else v.cpu().numpy() for k, v in m.state_dict().items()}
    out.update({f"grad {k}": bits(p.grad) for k, p in m.named_parameters() if p.grad is not None})
    return out


def assert_same_states(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        same(a[k], b[k], f"{what} {k}")


ORDERS = {"one group": [[0, 1, 2]], "three single calls": [[0], [1], [2]], "reversed": [[2, 1, 0]]}


def test_fused_step_does_not_depend_on_grouping_or_order():
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_step_group
    results = {}
    for name, calls in ORDERS.items():
        models, opts, xs, labs = three_replicas(930, True)
        losses = {}
        for step in range(2):
            for ks in calls:
                ls, _ = cnnlstm_train_step_group([models[k] for k in ks], [opts[k] for k in ks], [xs[k] for k in ks], [labs[k] for k in ks])
                for k, v in zip(ks, bits(ls)):
                    losses[step, k] = v
        assert [m.dropout_stream.step for m in models] == [2, 2, 2]
        results[name] = (losses, [state_bits(m) for m in models])
    want = results["one group"]
    for name in ("three single calls", "reversed"):
        assert results[name][0] == want[0], f"losses: {name}"
        for k in range(3):
            assert_same_states(results[name][1][k], want[1][k], f"{name}: replica {k}")


def test_autograd_step_does_not_depend_on_grouping_or_order():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_group
    results = {}
    for name, calls in ORDERS.items():
        models, _, xs, labs = three_replicas(940, False)
        logits = {}
        for ks in calls:
            outs = cnnlstm_train_group([models[k] for k in ks], [xs[k] for k in ks])
            torch.stack([torch.nn.functional.cross_entropy(o, labs[k]) for o, k in zip(outs, ks)]).sum().backward()
            for k, o in zip(ks, outs):
                logits[k] = bits(o)
        results[name] = (logits, [state_bits(m) for m in models])
    want = results["one group"]
    assert any(k.startswith("grad ") for k in want[1][0])
    for name in ("three single calls", "reversed"):
        for k in range(3):
            same(results[name][0][k], want[0][k], f"{name}: logits of replica {k}")
            assert_same_states(results[name][1][k], want[1][k], f"{name}: replica {k}")


# ---- 4. the promise this closes: lock step == sequential trainings, with dropout on -------------------------------------
def lockstep_replica(k, fused):
    import torch
    from torch.utils.data import DataLoader
    from robust_speech_analysis_framework_amd.cnnlstm import DropoutStream, FusedAdam, collate_zero_pad

    def collate(batch):
        return collate_zero_pad([b[0] for b in batch], device="cpu"), torch.tensor([b[1] for b in batch], dtype=torch.long)

    m, _ = build(D, CH, H, 950 + k, "silu", p_rate=0.3, p_block=0.3)
    freeze_zero_grad(m)
    m.dropout_stream = DropoutStream(dr.SEEDS[2] + k)
    rng = np.random.Generator(np.random.PCG64(960 + k))
    data = [(synth_input(1, int(rng.integers(10, 31)), D, 970 + 100 * k + i)[0], int(rng.integers(0, 2))) for i in range((12, 8)[k])]
    loader = DataLoader(data, batch_size=4, shuffle=True, collate_fn=collate, generator=torch.Generator().manual_seed(980 + k))
    opt = FusedAdam(m, lr=1e-3) if fused else torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    return m, opt, loader


@pytest.mark.parametrize("optimizer", ["FusedAdam", "torch.optim.Adam"])
def test_lockstep_equals_sequential_trainings_with_dropout(optimizer):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import train_replicas_lockstep
    fused, epochs, loss_fn = optimizer == "FusedAdam", 2, torch.nn.CrossEntropyLoss()
    together = [lockstep_replica(k, fused) for k in range(2)]
    assert [len(r[2]) for r in together] == [3, 2]                         # replica 1 sits out the third step of every epoch
    hist = train_replicas_lockstep(*zip(*together), loss_fn, epochs, "cuda")
    assert [r[0].dropout_stream.step for r in together] == [6, 4]
    for k in range(2):
        m, opt, loader = lockstep_replica(k, fused)
        alone = train_replicas_lockstep([m], [opt], [loader], loss_fn, epochs, "cuda")[0]
        assert m.dropout_stream.state_dict() == together[k][0].dropout_stream.state_dict()
        assert alone == hist[k], (k, alone, hist[k])
        assert_same_states(state_bits(together[k][0]), state_bits(m), f"replica {k}")
