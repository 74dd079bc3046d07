"""Device-resident training data on the GPU: rsaf_collate_pad_group against pad_sequence, DeviceBatchLoader against a
DataLoader, and the three lock-step loops fed by device loaders against the same loops fed by DataLoaders.  Everything
compared is copies and zeros, so every comparison is bit for bit; the batch reference is torch's pad_sequence on the CPU,
the order reference a DataLoader."""
import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import DataLoader

from cnnlstm_support import bits, launches, lockstep_setup, same

pytestmark = pytest.mark.gpu

WIDTHS = (768, 16, 4, 6, 5)         # 6 and 5: the dword path, rows off the 16-byte grid
# sequence lengths of the kernel test's store; a workgroup takes 2 048 float4 or float elements, so 450 frames make a
# member of several workgroups on the float4 path (43 at width 768) and on the dword path (2 at widths 5 and 6); 7 is the T
# of the first batches, 0 an empty member
LENGTHS = (1, 7, 0, 3, 5, 7, 7, 7, 2, 450, 30)
BATCHES = ((0, 1, 2, 3, 4),         # B = 5: lengths 1, T, 0 and two in between
           (8,),                    # B = 1
           (5, 6, 7),               # equal lengths: no padding
           (9, 0, 2),               # T = 450: several workgroups per member, a member of 1 frame, an empty one
           (10, 9),                 # a member that is not the longest spanning workgroups
           (2,))                    # would be T = 0 with pad_sequence; here asked for with T = 1: a block of zeros


def reference_cast(seq):
    return torch.FloatTensor(seq.copy())          # SequenceDataset.__getitem__, src/dl_cv_strategies.py:62


@pytest.fixture(scope="module")
def kernel_data():
    rng = np.random.Generator(np.random.PCG64(2400))
    data = {}
    for width in WIDTHS:
        # float64 values that float32 cannot hold: the cast is part of what is compared
        seqs = [rng.standard_normal((n, width)) * 10.0 ** rng.integers(-3, 4) for n in LENGTHS]
        labels = rng.integers(0, 5, len(LENGTHS))
        data[width] = (seqs, labels)
    return data


def run_items(store, labels_device, batches, T_of=None):
    """One rsaf_collate_pad_group call over `batches` (lists of sequence indices of the store), outputs pre-filled with
    NaN / -7 so that every element is shown to be written."""
    from robust_speech_analysis_framework_amd import _lib
    lib = _lib.load()
    items = (_lib.CollateItem * len(batches))()
    keep, outs = [], []
    for it, members in zip(items, batches):
        idx = torch.tensor(members, dtype=torch.int64, device="cuda")
        start = store.frame_off_device[idx].contiguous()
        count = (store.frame_off_device[idx + 1] - start).to(torch.int32).contiguous()
        T = max(int(store.lengths[list(members)].max()), 1) if T_of is None else T_of
        x = torch.full((len(members), T, store.width), float("nan"), dtype=torch.float32, device="cuda")
        lab = torch.full((len(members),), -7, dtype=torch.int64, device="cuda")
        it.arena, it.arena_rows, it.row_start, it.row_count = store.arena.data_ptr(), store.arena.shape[0], start.data_ptr(), count.data_ptr()
        it.B, it.T, it.out = len(members), T, x.data_ptr()
        it.label_src, it.label_count, it.label_index, it.label_out = labels_device.data_ptr(), labels_device.numel(), idx.data_ptr(), lab.data_ptr()
        it.frames = int(np.minimum(store.lengths[list(members)], T).sum())
        keep += [idx, start, count]
        outs.append((x, lab))
    _lib.check(lib.rsaf_collate_pad_group(items, len(batches), store.width, _lib.stream_ptr(None)), "rsaf_collate_pad_group")
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("width", WIDTHS)
def test_collate_kernel_equals_pad_sequence(kernel_data, width):
    from robust_speech_analysis_framework_amd.device_data import DeviceSequenceStore
    seqs, labels = kernel_data[width]
    store = DeviceSequenceStore(seqs)
    assert len(store) == len(LENGTHS) and store.width == width and store.nbytes == sum(LENGTHS) * width * 4
    assert list(store.lengths) == list(LENGTHS) and store.frame_off[-1] == sum(LENGTHS)
    same(bits(store.sequence(4)), bits(reference_cast(seqs[4])), "store.sequence(4)")
    assert store.arena.data_ptr() % 16 == 0
    labels_device = torch.from_numpy(labels).cuda()
    outs = run_items(store, labels_device, BATCHES)            # one call, items of different B and T
    for members, (x, lab) in zip(BATCHES, outs):
        want = pad_sequence([reference_cast(seqs[i]) for i in members], batch_first=True, padding_value=0)
        if want.shape[1] == 0:
            want = torch.zeros((len(members), 1, width))
        assert not torch.isnan(x).any(), f"batch {members}: elements left unwritten"
        same(bits(x), bits(want), f"width {width} batch {members}")
        assert lab.tolist() == [int(labels[i]) for i in members]


def test_collate_truncates_at_T_and_takes_unaligned_outputs(kernel_data):
    """T below a member's length copies its first T frames (the contract's min(row_count, T)); an `out` off the 16-byte
    grid takes the dword path at a width that would allow float4."""
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.device_data import DeviceSequenceStore
    seqs, labels = kernel_data[16]
    store = DeviceSequenceStore(seqs)
    labels_device = torch.from_numpy(labels).cuda()
    (x, _), = run_items(store, labels_device, [(1, 10, 0)], T_of=4)
    want = torch.zeros((3, 4, 16))
    for b, i in enumerate((1, 10, 0)):
        s = reference_cast(seqs[i])[:4]
        want[b, :s.shape[0]] = s
    same(bits(x), bits(want), "T = 4 below the members' lengths")
    # the same batch into a buffer that starts 4 bytes off the grid
    lib = _lib.load()
    idx = torch.tensor([1, 10, 0], dtype=torch.int64, device="cuda")
    start = store.frame_off_device[idx].contiguous()
    count = (store.frame_off_device[idx + 1] - start).to(torch.int32).contiguous()
    buf = torch.full((3 * 30 * 16 + 1,), float("nan"), dtype=torch.float32, device="cuda")
    item = (_lib.CollateItem * 1)()
    it = item[0]
    it.arena, it.arena_rows, it.row_start, it.row_count = store.arena.data_ptr(), store.arena.shape[0], start.data_ptr(), count.data_ptr()
    it.B, it.T, it.out, it.frames = 3, 30, buf.data_ptr() + 4, -1
    _lib.check(lib.rsaf_collate_pad_group(item, 1, 16, _lib.stream_ptr(None)), "rsaf_collate_pad_group")
    torch.cuda.synchronize()
    want = pad_sequence([reference_cast(seqs[i]) for i in (1, 10, 0)], batch_first=True)
    assert torch.isnan(buf[0])                                   # the float in front of `out` is not touched
    same(bits(buf[1:].view(3, 30, 16)), bits(want), "unaligned out")


def fold_data(loaders):
    """The (sequence, label) lists of lockstep_setup's DataLoaders."""
    return [ld.dataset for ld in loaders]


def device_loaders(loaders, shuffle, generators):
    """DeviceBatchLoaders over ONE store that holds the data of all `loaders`, each a view of its own part."""
    from robust_speech_analysis_framework_amd.device_data import DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore
    folds = fold_data(loaders)
    store = DeviceSequenceStore([s for fold in folds for s, _ in fold])
    whole = DeviceSequenceDataset(store, [lab for fold in folds for _, lab in fold])
    out, first = [], 0
    for fold, ld, gen in zip(folds, loaders, generators):
        view = whole.subset(np.arange(first, first + len(fold)))
        out.append(DeviceBatchLoader(view, batch_size=ld.batch_size, shuffle=shuffle, generator=gen))
        first += len(fold)
    return out


def test_collate_batches_chunks_like_every_group_call():
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import collate_batches, train_group_max
    _, _, loaders = lockstep_setup(2410, lambda k, m: None, shuffle=False)
    dls = device_loaders(loaders, False, [None] * 3)
    K = train_group_max() + 1
    plans = [p for dl in dls for p in dl.plans()] * 2
    plans = plans[:K]
    assert len(plans) == K == 17
    _lib.prof_begin()
    together = collate_batches(plans)
    prof = _lib.prof_end()
    assert launches(prof, "train_collate") == 2
    written = sum(p.B * p.T for p in plans) * 16 * 4
    read = sum(p.frames for p in plans) * 16 * 4
    assert prof["train_collate"]["bytes"] == written + read          # floats read + written, times four
    host = [b for ld in loaders for b in ld] * 2
    for k, (p, (x, lab)) in enumerate(zip(plans, together)):
        (x1, lab1), = collate_batches([p])
        same(bits(x), bits(x1), f"item {k} of the chunked call against a call of its own")
        assert torch.equal(lab, lab1)
        same(bits(x), bits(host[k][0]), f"item {k} against the DataLoader's batch")
        assert torch.equal(lab.cpu(), host[k][1])


@pytest.mark.parametrize("rng", ["own_generator", "global_rng"])
def test_device_loader_equals_dataloader(rng):
    from robust_speech_analysis_framework_amd.device_data import DeviceBatchLoader
    seed = 2420
    _, _, loaders = lockstep_setup(seed, lambda k, m: None)
    own = rng == "own_generator"
    if not own:                                    # the same data and collate, permutations from torch's global RNG
        loaders = [DataLoader(ld.dataset, batch_size=4, shuffle=True, collate_fn=ld.collate_fn) for ld in loaders]
    dls = device_loaders(loaders, True, [torch.Generator().manual_seed(seed + k) if own else None for k in range(3)])
    assert [len(d) for d in dls] == [len(ld) for ld in loaders] == [5, 3, 4]
    for k, (ld, dl) in enumerate(zip(loaders, dls)):
        assert isinstance(dl, DeviceBatchLoader)
        torch.manual_seed(seed + 50 + k)
        want = [list(ld) for _ in range(2)]
        want_state = ld.generator.get_state() if own else torch.get_rng_state()
        torch.manual_seed(seed + 50 + k)
        got = [list(dl) for _ in range(2)]
        got_state = dl.generator.get_state() if own else torch.get_rng_state()
        assert torch.equal(got_state, want_state), f"loader {k}: RNG state after two epochs"
        for e in range(2):
            assert len(got[e]) == len(want[e])
            for j, ((x, lab), (wx, wlab)) in enumerate(zip(got[e], want[e])):
                assert x.is_cuda and lab.is_cuda and x.dtype == torch.float32 and lab.dtype == torch.int64
                same(bits(x), bits(wx), f"loader {k} epoch {e} batch {j}")
                assert torch.equal(lab.cpu(), wlab), (k, e, j)
    # a dataset item is (device view, device int64 label)
    x0, y0 = dls[1].dataset[2]
    same(bits(x0), bits(torch.as_tensor(loaders[1].dataset[2][0])), "dataset[2] of the second view")
    assert y0.is_cuda and y0.dtype == torch.int64 and int(y0) == loaders[1].dataset[2][1]


def state_of(models, opts):
    out = {}
    for k, (m, o) in enumerate(zip(models, opts)):
        for name, t in m.state_dict().items():
            out[f"{k}.{name}"] = t.detach().cpu().numpy().copy()
        if o is not None:
            for name, p in m.named_parameters():
                for moment in ("exp_avg", "exp_avg_sq"):
                    if moment in o.state.get(p, {}):
                        out[f"{k}.{name}.{moment}"] = bits(o.state[p][moment])
    return out


def same_state(got, want, what):
    assert sorted(got) == sorted(want)
    for name in want:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {name} differs"


@pytest.mark.parametrize("optimizer", ["fused_adam", "torch_adam"])
def test_lockstep_training_with_device_loaders_equals_dataloaders(optimizer):
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_replicas_lockstep
    seed, epochs, lr = 2430, 2, 2e-3
    mk = (lambda k, m: FusedAdam(m, lr=lr)) if optimizer == "fused_adam" else (lambda k, m: torch.optim.Adam(m.parameters(), lr=lr))
    loss_fn = torch.nn.CrossEntropyLoss()
    gens = lambda: [torch.Generator().manual_seed(seed + k) for k in range(3)]            # noqa: E731  (lockstep_setup's seeds)

    models, opts, loaders = lockstep_setup(seed, mk)
    _lib.prof_begin()
    want = train_replicas_lockstep(models, opts, loaders, loss_fn, epochs, "cuda")
    prof = _lib.prof_end()
    assert launches(prof, "train_collate") == 0
    assert launches(prof, "train_adam") == (epochs * 5 if optimizer == "fused_adam" else 0)
    want_state = state_of(models, opts)

    models, opts, loaders = lockstep_setup(seed, mk)
    dls = device_loaders(loaders, True, gens())
    _lib.prof_begin()
    got = train_replicas_lockstep(models, opts, dls, loss_fn, epochs, "cuda")
    prof = _lib.prof_end()
    assert launches(prof, "train_collate") == epochs * max(len(d) for d in dls) == 10        # one per group step
    assert launches(prof, "gather_rows") == 0
    assert got == want, (got, want)
    same_state(state_of(models, opts), want_state, "device loaders")

    models, opts, loaders = lockstep_setup(seed, mk)
    dls = device_loaders(loaders, True, gens())
    mixed = [dls[0], loaders[1], dls[2]]
    _lib.prof_begin()
    got = train_replicas_lockstep(models, opts, mixed, loss_fn, epochs, "cuda")
    assert launches(_lib.prof_end(), "train_collate") == 10
    assert got == want, (got, want)
    same_state(state_of(models, opts), want_state, "one DataLoader and two device loaders")


def test_train_eval_and_eval_lockstep_with_device_loaders_equal_dataloaders():
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import (FusedAdam, eval_model_grouped, eval_replicas_lockstep,
                                                              train_eval_replicas_lockstep)
    seed, epochs, patience = 2440, 3, 1
    mk = lambda k, m: FusedAdam(m, lr=2e-3)                                                 # noqa: E731
    loss_fn = torch.nn.CrossEntropyLoss()

    def run(device_side):
        models, opts, loaders = lockstep_setup(seed, mk, p=0.2)
        _, _, val_loaders = lockstep_setup(seed + 50, lambda k, m: None, shuffle=False)
        if device_side:
            loaders = device_loaders(loaders, True, [torch.Generator().manual_seed(seed + k) for k in range(3)])
            val_loaders = device_loaders(val_loaders, False, [None] * 3)
        torch.manual_seed(seed)                       # the dropout masks come from torch's device RNG
        torch.cuda.manual_seed(seed)
        _lib.prof_begin()
        res = train_eval_replicas_lockstep(models, opts, [None] * 3, loaders, val_loaders, loss_fn, epochs, patience, "cuda")
        prof = _lib.prof_end()
        _lib.prof_begin()
        ev = eval_replicas_lockstep(models, val_loaders, "cuda")
        ev_prof = _lib.prof_end()
        one = eval_model_grouped(models[1], val_loaders[1], "cuda")
        return res, ev, one, state_of(models, [None] * 3), prof, ev_prof

    want, want_ev, want_one, want_state, prof, ev_prof = run(False)
    assert launches(prof, "train_collate") == 0 and launches(ev_prof, "train_collate") == 0
    got, got_ev, got_one, got_state, prof, ev_prof = run(True)
    # the 12 validation batches of a pass fit one group call: at most one collate launch per batch, here one per pass
    assert launches(ev_prof, "train_collate") == 1
    assert 0 < launches(prof, "train_collate") <= epochs * (5 + 1)
    for k in range(3):
        assert got[k][1] == want[k][1], (k, "training history", got[k][1], want[k][1])
        assert got[k][2] == want[k][2], (k, "validation history", got[k][2], want[k][2])
        for name, a, b in zip(("labels", "predictions", "probabilities"), got_ev[k], want_ev[k]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (k, name)
    for a, b in zip(got_one, want_one):
        assert a.tobytes() == b.tobytes()
    same_state(got_state, want_state, "best weights")


def test_store_on_another_device_than_the_models_is_refused_by_name():
    from robust_speech_analysis_framework_amd.cnnlstm import eval_replicas_lockstep, train_replicas_lockstep
    models, opts, loaders = lockstep_setup(2450, lambda k, m: None, shuffle=False)
    dls = device_loaders(loaders, False, [None] * 3)
    with pytest.raises(ValueError, match="loader 1 is a DeviceBatchLoader whose DeviceSequenceStore is on 'cuda:0', but the models are on 'cpu'"):
        train_replicas_lockstep(models, opts, [loaders[0], dls[1], dls[2]], torch.nn.CrossEntropyLoss(), 1, "cpu")
    with pytest.raises(ValueError, match="eval_replicas_lockstep: loader 0 is a DeviceBatchLoader"):
        eval_replicas_lockstep(models, dls, "cpu")


def test_from_interview_clips_equals_aggregate_interview_sequences():
    import pandas as pd
    from robust_speech_analysis_framework_amd.aggregate import aggregate_interview_sequences
    from robust_speech_analysis_framework_amd.device_data import DeviceSequenceStore
    rng = np.random.Generator(np.random.PCG64(2460))
    files = [f"clip{i}.wav" for i in range(9)]
    meta = pd.DataFrame({"filename": files + ["missing.wav"],
                         "unique_participant_id": ["p2", "p0", "p2", "p1", "p0", "p3", "p2", "p1", "p0", "p4"]})
    clips = {f: rng.standard_normal((int(rng.integers(1, 9)), 12)).astype(np.float32) for f in files if f != "clip5.wav"}
    want = aggregate_interview_sequences(clips, meta)                 # p3 and p4 have no sequence: absent
    store, pids = DeviceSequenceStore.from_interview_clips(clips, meta)
    assert pids == list(want) == ["p0", "p1", "p2"] and len(store) == 3 and store.width == 12
    host = store.arena.cpu().numpy()                                  # one copy back
    for i, pid in enumerate(pids):
        got = host[store.frame_off[i]:store.frame_off[i + 1]]
        assert got.shape == want[pid].shape and got.tobytes() == want[pid].tobytes(), pid
        assert store.sequence(i).shape == want[pid].shape
