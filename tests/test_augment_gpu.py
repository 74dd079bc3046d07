"""Device-side augmentations on the GPU: rsaf_collate_augment_group against the NumPy restatement of the mapping in
include/rsaf.h (tests/augment_restatement.py) over the store of tests/test_device_data_gpu.py, the purity of the mapping
(grouping, batch, T, store path), DeviceBatchLoader with a transform, and train_eval_replicas_lockstep over augmented loaders
against the same trainings run one after another.  Scale, TimeMask and FeatureMask are integer or single-rounded arithmetic:
every comparison of theirs is bit for bit.  Only the normals carry a bar:
    |out - ref| <= amp * 2^-17 + 2^-23 * |ref|        per element, ref the float64 restatement
|z| <= sqrt(48 ln 2) = 5.77 < 8; logf, sqrtf and sincospif are each within about 2 ulp, together a few ulp of a value below 8,
i.e. below 2^-19; 2^-17 leaves a factor of 4.  The second term is the rounding of the final fmaf."""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_restatement as ar
from cnnlstm_support import GEOMETRIES, RAGGED, bits, build, freeze_zero_grad, launches, same, synth_input
from test_device_data_gpu import BATCHES, LENGTHS, WIDTHS, kernel_data, reference_cast, run_items  # noqa: F401  (kernel_data: fixture)

pytestmark = pytest.mark.gpu

SEED, EPOCH = 0x5EED + 25, 3
CHUNK = 2048                                        # elements (float4 or float) of one workgroup

# (kind, a, b, p) as the restatement takes them; the tests build the library's table from the same tuples
PIPELINES = {
    "scale_p1": [(ar.SCALE, 0.5, 1.5, 1.0)],
    "scale_half": [(ar.SCALE, 0.5, 1.5, 0.5)],
    "time_p1": [(ar.TIME_MASK, 0.05, 0.5, 1.0)],
    "time_half": [(ar.TIME_MASK, 0.05, 0.5, 0.5)],
    "feature_p1": [(ar.FEATURE_MASK, 0.2, 0.7, 1.0)],
    "feature_half": [(ar.FEATURE_MASK, 0.2, 0.7, 0.5)],
    # a negative factor last: a masked value becomes -0.0 on both sides, and padding that were scaled would show as -0.0
    "composed": [(ar.SCALE, 0.5, 1.5, 0.5), (ar.TIME_MASK, 0.05, 0.5, 1.0), (ar.FEATURE_MASK, 0.2, 0.7, 0.5), (ar.TIME_MASK, 0.0, 1.0, 0.5),
                 (ar.SCALE, -1.5, -0.5, 1.0)],
}
NOISE = [(ar.GAUSSIAN_NOISE, 0.001, 0.015, 1.0)]
FULL = [(ar.SCALE, 0.5, 1.5, 1.0), (ar.GAUSSIAN_NOISE, 0.001, 0.015, 1.0), (ar.TIME_MASK, 0.0, 0.5, 1.0), (ar.FEATURE_MASK, 0.0, 0.5, 1.0)]


def op_table(ops):
    """(host table, device tensor) of a pipeline given as restatement tuples, through the package's own classes."""
    from robust_speech_analysis_framework_amd.augment import Compose, FeatureMask, GaussianNoise, Scale, TimeMask
    cls = {ar.SCALE: Scale, ar.GAUSSIAN_NOISE: GaussianNoise, ar.TIME_MASK: TimeMask, ar.FEATURE_MASK: FeatureMask}
    tf = Compose([cls[kind](a, b, p=p) for kind, a, b, p in ops])
    return tf, tf.table("cuda")


def run_augmented(store, batches, ops, seed=SEED, epoch=EPOCH, T_of=None, sample_of=None, one_call=True, off_grid=False):
    """rsaf_collate_augment_group over `batches` (lists of sequence indices of the store) with pipeline `ops` (`ops[k]` per
    batch if a list of lists), outputs pre-filled with NaN.  one_call=False: one call per batch.  off_grid: every `out`
    starts 4 bytes off the 16-byte grid (the float in front is returned as well)."""
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    per_batch = ops if ops and isinstance(ops[0], list) else [ops] * len(batches)
    items = (_lib.CollateAugmentItem * len(batches))()
    keep, outs = [], []
    for it, members, pipeline in zip(items, batches, per_batch):
        idx = torch.tensor(members, dtype=torch.int64, device="cuda")
        start = store.frame_off_device[idx].contiguous()
        count = (store.frame_off_device[idx + 1] - start).to(torch.int32).contiguous()
        T = max(int(store.lengths[list(members)].max()), 1) if T_of is None else T_of
        buf = torch.full((len(members) * T * store.width + 4,), float("nan"), dtype=torch.float32, device="cuda")
        x = buf[1:1 + len(members) * T * store.width] if off_grid else buf[4:]
        assert buf.data_ptr() % 16 == 0
        sample = idx if sample_of is None else torch.tensor([sample_of(i) for i in members], dtype=torch.int64, device="cuda")
        it.arena, it.arena_rows, it.row_start, it.row_count = store.arena.data_ptr(), store.arena.shape[0], start.data_ptr(), count.data_ptr()
        it.B, it.T, it.out, it.frames = len(members), T, x.data_ptr(), -1
        tf, table = op_table(pipeline)
        it.ops, it.ops_host, it.n_ops = table.data_ptr(), C.addressof(tf.table_host), len(tf)
        it.seed, it.epoch, it.sample_id = seed, epoch, sample.data_ptr()
        keep += [idx, start, count, sample, tf, table, buf]
        outs.append((x.view(len(members), T, store.width), buf[0]))
    calls = [(items, len(batches))] if one_call else [(C.pointer(items[k]), 1) for k in range(len(batches))]
    for first, n in calls:
        _lib.check(lib.rsaf_collate_augment_group(first, n, store.width, _lib.stream_ptr(None)), "rsaf_collate_augment_group")
    torch.cuda.synchronize()
    return [x for x, _ in outs] if not off_grid else outs


@pytest.fixture(scope="module")
def stores(kernel_data):  # noqa: F811
    """The store of every width (one upload each) and its float32 sequences on the host."""
    from robust_speech_analysis_framework_amd.device_data import DeviceSequenceStore
    return {width: (DeviceSequenceStore(seqs), [reference_cast(s).numpy() for s in seqs]) for width, (seqs, _) in kernel_data.items()}


def restated(seqs32, members, T, ops, seed=SEED, epoch=EPOCH):
    """(ref [B, T, D], amp [B, T, D]) of a batch: every member augmented by the restatement, then padded with +0.0."""
    D = seqs32[0].shape[1]
    ref, amp = np.zeros((len(members), T, D), dtype=np.float64), np.zeros((len(members), T, D), dtype=np.float64)
    exact = True
    for b, i in enumerate(members):
        r, a = ar.apply(seqs32[i], ops, seed, epoch, i)
        exact = exact and r.dtype == np.float32
        n = min(seqs32[i].shape[0], T)
        ref[b, :n], amp[b, :n] = r[:n], a[:n]
    return (ref.astype(np.float32) if exact else ref), amp


def test_the_conditions_the_seed_was_chosen_for():
    """Asserted on the restatement, met by the choice of SEED: at p = 0.5 some tested members fire and some do not; at width
    16 a feature band starts off a multiple of 4 with len > 0; the time span of the 450-frame member crosses a workgroup
    boundary on both store paths."""
    members = sorted({i for b in BATCHES for i in b})
    for name in ("scale_half", "time_half", "feature_half"):
        fired = {ar.decisions(PIPELINES[name], SEED, EPOCH, i, LENGTHS[i], 16)[0]["fires"] for i in members}
        assert fired == {True, False}, name
    bands = [ar.decisions(PIPELINES["feature_p1"], SEED, EPOCH, i, LENGTHS[i], 16)[0] for i in members]
    assert any(d["start"] % 4 != 0 and d["len"] > 0 for d in bands), bands
    d = ar.decisions(PIPELINES["time_p1"], SEED, EPOCH, 9, 450, 768)[0]
    for row_elements in (768 // 4, 16 // 4, 6, 5):                # elements of a row: float4 at 768 and 16, dwords at 6 and 5
        lo, hi = d["start"] * row_elements, (d["start"] + d["len"]) * row_elements
        if 450 * row_elements > CHUNK:
            assert lo // CHUNK != (hi - 1) // CHUNK, (row_elements, d)


@pytest.mark.parametrize("width", WIDTHS)
def test_no_ops_equals_the_plain_collate_bit_for_bit(stores, kernel_data, width):  # noqa: F811
    store, _ = stores[width]
    labels_device = torch.from_numpy(kernel_data[width][1]).cuda()
    plain = run_items(store, labels_device, BATCHES)
    got = run_augmented(store, BATCHES, [])
    for members, (want, _), x in zip(BATCHES, plain, got):
        assert not torch.isnan(x).any()
        same(bits(x), bits(want), f"width {width} batch {members}")


@pytest.mark.parametrize("name", sorted(PIPELINES))
@pytest.mark.parametrize("width", WIDTHS)
def test_deterministic_ops_equal_the_restatement_bit_for_bit(stores, width, name):
    store, seqs32 = stores[width]
    got = run_augmented(store, BATCHES, PIPELINES[name])
    for members, x in zip(BATCHES, got):
        want, _ = restated(seqs32, members, x.shape[1], PIPELINES[name])
        assert want.dtype == np.float32 and not torch.isnan(x).any(), f"batch {members}: elements left unwritten"
        same(bits(x), want.view(np.uint32), f"{name} width {width} batch {members}")
        for b, i in enumerate(members):                       # the padding is +0.0: no sign bit
            assert not bits(x[b, LENGTHS[i]:]).any(), (name, width, members, b)


@pytest.mark.parametrize("name,ops", [("noise", NOISE), ("full", FULL)])
@pytest.mark.parametrize("width", WIDTHS)
def test_noise_is_within_the_bar_of_the_float64_restatement(stores, width, name, ops):
    store, seqs32 = stores[width]
    got = run_augmented(store, BATCHES, ops)
    worst = 0.0
    for members, x in zip(BATCHES, got):
        ref, amp = restated(seqs32, members, x.shape[1], ops)
        out = x.cpu().numpy().astype(np.float64)
        assert not np.isnan(out).any()
        bar = amp * 2.0 ** -17 + 2.0 ** -23 * np.abs(ref)
        err = np.abs(out - ref)
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all(), (name, width, members, float(err.max()), float((err - bar).max()))
        for b, i in enumerate(members):
            assert not bits(x[b, LENGTHS[i]:]).any(), (name, width, members, b)
        if name == "noise":                                # noise was added: members with frames differ from the plain copy
            for b, i in enumerate(members):
                if LENGTHS[i]:
                    assert (out[b, :LENGTHS[i]] != seqs32[i]).mean() > 0.9
    print(f"{name} width {width}: worst error {worst:.3f} of its bar")


def test_purity_grouping_batch_and_T(stores):
    store, _ = stores[768]
    together = run_augmented(store, BATCHES, FULL)
    alone = run_augmented(store, BATCHES, FULL, one_call=False)
    for members, a, b in zip(BATCHES, together, alone):
        same(bits(a), bits(b), f"batch {members}: one K = 6 call against six K = 1 calls")
    # member 10 (30 frames) next to the 450-frame member, and in a batch of its own T with another neighbour
    (long_batch,), (short_batch,) = run_augmented(store, [(10, 9)], FULL), run_augmented(store, [(1, 10, 4)], FULL)
    assert long_batch.shape[1] == 450 and short_batch.shape[1] == 30
    same(bits(long_batch[0, :30]), bits(short_batch[1]), "member 10 at T = 450 and at T = 30")
    same(bits(together[4][0, :30]), bits(short_batch[1]), "member 10 in the K = 6 call")
    # the same (seed, epoch, sample) twice in one call
    (twice,) = run_augmented(store, [(10, 9, 10)], FULL)
    same(bits(twice[0]), bits(twice[2]), "member 10 twice in one batch")
    base = bits(short_batch[1])
    for what, kw in (("another epoch", {"epoch": EPOCH + 1}), ("another seed", {"seed": SEED + 1}),
                     ("another sample id", {"sample_of": lambda i: i + 100})):
        (other,) = run_augmented(store, [(1, 10, 4)], FULL, **kw)
        # the masks of FULL leave at least 0.5 * 0.5 of a member standing, and every standing element carries its own noise
        assert (bits(other[1]) != base).mean() > 0.2, what


@pytest.mark.parametrize("width", (16, 768))
def test_float4_and_dword_paths_give_the_same_bits(stores, width):
    store, _ = stores[width]
    batches = [(1, 10, 0), (9,)]
    aligned = run_augmented(store, batches, FULL)
    shifted = run_augmented(store, batches, FULL, off_grid=True)
    for members, a, (b, front) in zip(batches, aligned, shifted):
        assert b.data_ptr() % 16 == 4 and torch.isnan(front)          # the float in front of `out` is not touched
        same(bits(a), bits(b), f"width {width} batch {members}: float4 path against the dword path")


# ---- loader level -----------------------------------------------------------------------------------------------------------
def loader_data(seed, n=11, D=16):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [synth_input(1, int(rng.integers(3, 20)), D, seed + 1 + i)[0] for i in range(n)], rng.integers(0, 2, n)


def full_transform():
    from robust_speech_analysis_framework_amd.augment import Compose, FeatureMask, GaussianNoise, Scale, TimeMask
    return Compose([Scale(0.5, 1.5), GaussianNoise(p=1.0), TimeMask(), FeatureMask()])


def test_loader_epochs_streams_and_checkpoints():
    from robust_speech_analysis_framework_amd.cnnlstm import AugmentStream, DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore
    seqs, labels = loader_data(2500)
    store = DeviceSequenceStore(seqs)

    def loader(stream, gen_seed=2501):
        ds = DeviceSequenceDataset(store, labels, transform=full_transform(), augment_stream=stream)
        return DeviceBatchLoader(ds, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(gen_seed))

    def epoch(ld):
        return [(bits(x), lab.cpu().numpy()) for x, lab in ld]

    def same_epoch(a, b, what):
        assert len(a) == len(b) == 3
        for j, ((xa, la), (xb, lb)) in enumerate(zip(a, b)):
            same(xa, xb, f"{what} batch {j}")
            assert np.array_equal(la, lb)

    s1, s2 = AugmentStream(77), AugmentStream(77)
    l1, l2 = loader(s1), loader(s2)
    run1 = [epoch(l1) for _ in range(3)]
    assert s1.epoch == 3                                        # one per epoch drawn
    first = epoch(l2)
    assert s2.epoch == 1
    same_epoch(first, run1[0], "equal streams, epoch 0")
    assert any(a[0].shape != b[0].shape or not np.array_equal(a[0], b[0]) for a, b in zip(run1[0], run1[1]))
    # continue the second run from its checkpoint: the stream's two keys and the sampler's generator
    s3 = AugmentStream(0)
    s3.load_state_dict(s2.state_dict())
    l3 = loader(s3)
    l3.generator.set_state(l2.generator.get_state())
    for e in (1, 2):
        same_epoch(epoch(l3), run1[e], f"continued run, epoch {e}")
    assert s3.state_dict() == {"seed": 77, "epoch": 3}
    # the same order without a transform is the plain copy: the transform changed the values, not the batches
    plain = DeviceBatchLoader(DeviceSequenceDataset(store, labels), batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(2501))
    for (xa, la), (xb, lb) in zip(epoch(plain), run1[0]):
        assert np.array_equal(la, lb) and xa.shape == xb.shape and not np.array_equal(xa, xb)


def test_plain_loaders_keep_the_old_entry_and_a_group_step_is_one_launch():
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import (AugmentStream, DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore,
                                                              collate_batches)
    seqs, labels = loader_data(2510)
    store = DeviceSequenceStore(seqs)
    whole = DeviceSequenceDataset(store, labels)
    plain = DeviceBatchLoader(whole, batch_size=4)
    _lib.prof_begin()
    want = list(plain)
    prof = _lib.prof_end()
    assert launches(prof, "train_collate") == 3 and launches(prof, "train_collate_augment") == 0
    # a group step: two augmented training plans (own streams) and one plain validation plan, one launch
    train = [DeviceBatchLoader(DeviceSequenceDataset(store, labels, transform=full_transform(), augment_stream=AugmentStream(5 + k)),
                               batch_size=4) for k in range(2)]
    plans = [next(iter(ld.plans())) for ld in train] + [next(iter(plain.plans()))]
    assert [p.epoch for p in plans] == [0, 0, None]
    _lib.prof_begin()
    got = collate_batches(plans)
    prof = _lib.prof_end()
    assert launches(prof, "train_collate_augment") == 1 and launches(prof, "train_collate") == 0
    same(bits(got[2][0]), bits(want[0][0]), "the plain plan of a mixed call")
    assert torch.equal(got[2][1], want[0][1]) and torch.equal(got[0][1], want[0][1])
    assert not np.array_equal(bits(got[0][0]), bits(got[1][0]))            # two streams, two augmentations of one batch
    # the same plan assembled again gives the same bits: it recorded its epoch
    again = collate_batches(plans[:1])
    same(bits(again[0][0]), bits(got[0][0]), "a plan assembled twice")


# ---- the loops --------------------------------------------------------------------------------------------------------------
def augmented_replica(k, store_cache={}):
    """Replica k of the loop test: model with dropout from a DropoutStream, FusedAdam, an augmented training loader and a
    plain validation loader over views of one store per replica."""
    from robust_speech_analysis_framework_amd.cnnlstm import (AugmentStream, DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore,
                                                              DropoutStream, FusedAdam)
    D, CH, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    B, T = RAGGED[k]
    m, _ = build(D, CH, H, 2520 + k, act, p_rate=0.2, p_block=0.2)
    freeze_zero_grad(m)
    m.dropout_stream = DropoutStream(2530 + k)
    if k not in store_cache:
        rng = np.random.Generator(np.random.PCG64(2540 + k))
        n = 2 * B + 1 + B                                         # training: two full batches and a ragged one; validation: one
        seqs = [synth_input(1, int(rng.integers(T // 2, T + 1)), D, 2550 + 100 * k + i)[0] for i in range(n)]
        store_cache[k] = (DeviceSequenceStore(seqs), rng.integers(0, 2, n))
    store, labels = store_cache[k]
    n_train = 2 * B + 1
    train = DeviceSequenceDataset(store, labels, np.arange(n_train), transform=full_transform(), augment_stream=AugmentStream(2560 + k))
    val = DeviceSequenceDataset(store, labels, np.arange(n_train, len(store)))
    return (m, FusedAdam(m, lr=2e-3), DeviceBatchLoader(train, batch_size=B, shuffle=True, generator=torch.Generator().manual_seed(2570 + k)),
            DeviceBatchLoader(val, batch_size=B))


def test_lockstep_over_augmented_loaders_equals_sequential_trainings():
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import train_eval_replicas_lockstep
    epochs, patience, loss_fn = 2, 5, torch.nn.CrossEntropyLoss()

    def state(m):
        return {name: bits(t) if t.dtype == torch.float32 else t.cpu().numpy() for name, t in m.state_dict().items()}

    together = [augmented_replica(k) for k in range(3)]
    models, opts, train, val = zip(*together)
    _lib.prof_begin()
    res = train_eval_replicas_lockstep(models, opts, [None] * 3, train, val, loss_fn, epochs, patience, "cuda")
    prof = _lib.prof_end()
    # per epoch three group steps of augmented plans and one validation pass of plain ones
    assert launches(prof, "train_collate_augment") == epochs * 3 and launches(prof, "train_collate") == epochs
    assert [ld.dataset.augment_stream.epoch for ld in train] == [epochs] * 3
    for k in range(3):
        m, opt, tl, vl = augmented_replica(k)
        (_, train_hist, val_hist), = train_eval_replicas_lockstep([m], [opt], [None], [tl], [vl], loss_fn, epochs, patience, "cuda")
        assert train_hist == res[k][1] and val_hist == res[k][2], (k, train_hist, res[k][1], val_hist, res[k][2])
        assert len(train_hist) == epochs and all(np.isfinite(train_hist)) and all(np.isfinite(val_hist))
        a, b = state(models[k]), state(m)
        assert sorted(a) == sorted(b)
        for name in a:
            assert np.array_equal(a[name], b[name]), f"replica {k}: {name} differs"
