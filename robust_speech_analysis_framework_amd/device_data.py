"""Device-resident training data for the lock-step loops: the sequences of a data set uploaded once, every batch assembled
on the device in ``DataLoader``'s order and with ``collate_fn``'s bits, the K batches of a group step in one launch
(``rsaf_collate_pad_group``; ``rsaf_collate_augment_group`` where a data set has a ``transform``, see ``augment``).

The reference feeds a model through ``DataLoader(SequenceDataset(X[idx], y[idx]), batch_size, shuffle, collate_fn)``
(``src/dl_cv_strategies.py:19-84,234-235``): every batch is padded on the CPU and uploaded again, per fold, per epoch and
per trial, although all of them draw from one ``sequences_dict``.  Here

* ``DeviceSequenceStore`` holds all sequences back to back in one float32 arena on the device (one upload);
* ``DeviceSequenceDataset`` is a fold's view of it (indices and labels), the counterpart of ``SequenceDataset``;
* ``DeviceBatchLoader`` is the counterpart of the ``DataLoader``: same batches in the same order, same use of the random
  number generators, ``(x [B, T, D] float32, labels [B] int64)`` on the device;
* ``collate_batches`` assembles any number of planned batches (``DeviceBatchLoader.plans()``) in one launch per
  ``train_group_max()`` of them, which is how the lock-step loops of ``cnnlstm_loops`` consume such loaders.

A store may hold layer stacks instead (``DeviceSequenceStore(..., layers=L)``: every sequence ``[L, T_i, D]``, the hidden
states of L encoder layers) for a learned ``LayerMix``: its plans carry the blocks' first rows, ``layer_mix_train`` mixes the
layers inside the collate launch, and the loader iterated on its own yields the zero-padded stack ``[B, L, T, D]``.

There is no CPU fallback: the store refuses a device that is not a HIP device.  ``cnnlstm`` re-exports the names of this
module.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .augment import AugmentStream, as_compose
from .layer_mix import LAYER_MIX_MAX

_STAGE_BYTES = 64 << 20             # pinned staging of an upload: two buffers of this size, however large the data set


def _draw_base_seed(generator):
    """The draw that ``iter(DataLoader)`` makes before anything else (``_BaseDataLoaderIter.__init__``)."""
    torch.empty((), dtype=torch.int64).random_(generator=generator)


def _draw_batches(n, batch_size, shuffle, generator, drop_last):
    """The index lists of one epoch out of torch's own samplers, as ``DataLoader`` composes them."""
    from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
    source = range(n)
    sampler = RandomSampler(source, generator=generator) if shuffle else SequentialSampler(source)
    return [list(b) for b in BatchSampler(sampler, batch_size, drop_last)]


def batch_indices(n, batch_size, shuffle=False, generator=None, drop_last=False):
    """The index lists of one epoch of ``DataLoader(dataset of n, batch_size, shuffle, generator=generator,
    drop_last=drop_last)``, drawn as ``iter(DataLoader)`` followed by its exhaustion draws them: first the loader's one
    base-seed draw, then torch's ``RandomSampler`` / ``SequentialSampler`` under ``BatchSampler``.  ``generator=None`` draws
    from torch's global RNG, as the ``DataLoader`` does.  The order and the state of the generator afterwards are those of
    the ``DataLoader``.  Pure host function."""
    _draw_base_seed(generator)
    return _draw_batches(int(n), batch_size, shuffle, generator, drop_last)


def _hip_device(device, who):
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{who}: the sequences must live on a HIP device (device='cuda'), not on '{device}': there is no CPU fallback")
    return device


def _resolved(device):
    """``device`` with its index spelled out (``cuda`` -> ``cuda:<current>``)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class DeviceSequenceStore:
    """All sequences of a data set in one float32 arena ``[sum T_i, D]`` on the device, uploaded once.

    ``sequences``: a sequence or object array of ``[T_i, D]`` arrays, as ``X_data`` is built at
    ``src/dl_cv_strategies.py:300``; values are cast to float32 as ``torch.FloatTensor(seq.copy())`` casts them
    (``SequenceDataset.__getitem__``).  The upload goes through two pinned staging buffers of bounded size, so no second
    full copy of the data is made on the host.  ``frame_off`` (host, int64 ``[n + 1]``) and ``frame_off_device`` give the
    arena rows of sequence i as ``frame_off[i] .. frame_off[i + 1]``.

    ``layers=L`` (1 <= L <= 32, ``RSAF_LAYER_MIX_MAX``): a store of layer stacks for a learned ``LayerMix``.  Every sequence
    is ``[L, T_i, D]`` with D a multiple of 4, what ``extract_wav2vec2_sequences(output_layers=[...])`` returns per file, and
    its block is uploaded as it lies in memory: ``L * T_i`` arena rows, layer-major, the arena row of (i, l, t) being
    ``L * frame_off[i] + l * T_i + t``.  ``frame_off`` and ``lengths`` stay in frames; ``layers`` is L (``None`` for a plain
    store) and ``sequence(i)`` the ``[L, T_i, D]`` view.  ``collate_mix_batches`` mixes the layers inside the collate launch;
    a ``DeviceBatchLoader`` iterated on its own yields the zero-padded stack ``[B, L, T, D]``."""

    layers = None                       # a plain store, unless ``_adopt`` says otherwise

    def __init__(self, sequences, device="cuda", layers=None):
        device = _hip_device(device, "DeviceSequenceStore")
        seqs = [s if torch.is_tensor(s) else np.asarray(s) for s in sequences]
        if not seqs:
            raise ValueError("DeviceSequenceStore: no sequences")
        if layers is not None:
            if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or not 1 <= layers <= LAYER_MIX_MAX:
                raise ValueError(f"DeviceSequenceStore: layers must be an integer in [1, {LAYER_MIX_MAX}] (or None: a plain store), "
                                 f"got {layers!r}")
            layers = int(layers)
        for i, s in enumerate(seqs):
            if layers is None and s.ndim != 2:
                raise ValueError(f"DeviceSequenceStore: sequence {i} has shape {tuple(s.shape)}, expected [T, D]")
            if layers is not None and (s.ndim != 3 or int(s.shape[0]) != layers):
                raise ValueError(f"DeviceSequenceStore: sequence {i} has shape {tuple(s.shape)}, expected [{layers}, T, D] (layers={layers})")
        width = int(seqs[0].shape[-1])
        for i, s in enumerate(seqs):
            if int(s.shape[-1]) != width:
                raise ValueError(f"DeviceSequenceStore: sequence {i} has width {int(s.shape[-1])}, sequence 0 has {width}: "
                                 "one store holds sequences of one width")
        if width < 1:
            raise ValueError("DeviceSequenceStore: sequences of width 0")
        if layers is not None and width % 4:
            raise ValueError(f"DeviceSequenceStore: a store of layer stacks needs a width that is a multiple of 4, got {width}")
        _lib.load()
        _lib.require_gpu()
        lengths = np.array([int(s.shape[-2]) for s in seqs], dtype=np.int64)
        rows = int(lengths.sum()) * (layers or 1)
        self._adopt(torch.empty((rows, width), dtype=torch.float32, device=_resolved(device)), lengths, layers)
        self._upload([s.reshape(-1, width) for s in seqs] if layers is not None else seqs)

    def _adopt(self, arena, lengths, layers=None):
        self.arena = arena
        self.layers = layers
        self.device = arena.device
        self.width = int(arena.shape[1])
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.frame_off = np.zeros(len(self.lengths) + 1, dtype=np.int64)
        np.cumsum(self.lengths, out=self.frame_off[1:])
        self.frame_off_device = torch.from_numpy(self.frame_off).to(self.device)

    @classmethod
    def _from_arena(cls, arena, lengths):
        store = cls.__new__(cls)
        store._adopt(arena, lengths)
        return store

    def _upload(self, seqs):
        """Pieces of at most ``_STAGE_BYTES`` through two pinned buffers in turn: the host fills one (casting to float32)
        while the other one's copy is in flight."""
        rows_cap = max(1, _STAGE_BYTES // (4 * self.width))
        rows_cap = min(rows_cap, max(1, int(self.arena.shape[0])))
        stage = [torch.empty((rows_cap, self.width), dtype=torch.float32).pin_memory() for _ in range(2)]
        done = [None, None]
        with torch.cuda.device(self.device):
            turn, fill, dst = 0, 0, 0

            def flush():
                nonlocal turn, fill, dst
                if fill:
                    self.arena[dst:dst + fill].copy_(stage[turn][:fill], non_blocking=True)
                    done[turn] = torch.cuda.Event()
                    done[turn].record()
                    dst += fill
                    turn, fill = 1 - turn, 0
                    if done[turn] is not None:
                        done[turn].synchronize()         # the buffer about to be refilled has been read

            for s in seqs:
                a, n = 0, int(s.shape[0])
                while a < n:
                    m = min(n - a, rows_cap - fill)
                    piece = s[a:a + m] if torch.is_tensor(s) else torch.from_numpy(np.ascontiguousarray(s[a:a + m]))
                    stage[turn][fill:fill + m].copy_(piece)                 # the cast of torch.FloatTensor(ndarray)
                    a, fill = a + m, fill + m
                    if fill == rows_cap:
                        flush()
            flush()
            torch.cuda.current_stream().synchronize()

    @classmethod
    def from_interview_clips(cls, clip_sequences, interview_metadata_df):
        """``(store, participant_ids)``: sequence i of the store is the stack of participant ``participant_ids[i]``'s clip
        sequences in metadata order, the arrays of ``aggregate.aggregate_interview_sequences`` (same skip rules, same
        ``gather_rows`` launch), left on the device."""
        from .aggregate import _stack_interview_clips
        out, spans = _stack_interview_clips(clip_sequences, interview_metadata_df)
        if not spans:
            raise ValueError("DeviceSequenceStore.from_interview_clips: no participant has a clip sequence")
        pids = list(spans)
        return cls._from_arena(out, [spans[p][1] - spans[p][0] for p in pids]), pids

    def __len__(self):
        return len(self.lengths)

    @property
    def nbytes(self):
        return int(self.arena.numel()) * 4

    def sequence(self, i):
        """Sequence i as a device view ``[T_i, D]`` of the arena (``[L, T_i, D]`` in a store of layer stacks)."""
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(f"sequence {i} of {len(self)}")
        i %= len(self)
        if self.layers is not None:
            L = self.layers
            return self.arena[L * int(self.frame_off[i]):L * int(self.frame_off[i + 1])].view(L, -1, self.width)
        return self.arena[int(self.frame_off[i]):int(self.frame_off[i + 1])]


class DeviceSequenceDataset:
    """A fold's view of a store: the counterpart of ``SequenceDataset(X[idx], y[idx])`` (``src/dl_cv_strategies.py:19-62``).

    ``labels``: one integer label per sequence of the STORE (``y_data``); ``indices``: the sequences of this view in
    order (``None``: all of them).  ``subset(idx)`` is the view of ``idx`` within this one, as ``X[idx]`` of an ``X`` that
    is already a subset.  ``dataset[i]`` is ``(device view [T, D], device int64 label)``, the sequence as stored.
    ``transform`` (a ``Compose`` or one op of ``augment``) with ``augment_stream`` (an ``AugmentStream``) is the
    counterpart of ``SequenceDataset``'s ``transform``: it is applied to every member of every batch a ``DeviceBatchLoader``
    assembles, inside the collate launch, a new draw per epoch of the stream; the two go together, and views made by
    ``subset`` share both.  A host callable is refused: those stay with the ``DataLoader`` path."""

    def __init__(self, store, labels, indices=None, transform=None, augment_stream=None):
        if not isinstance(store, DeviceSequenceStore):
            raise TypeError(f"DeviceSequenceDataset: store is a {type(store).__name__}, not a DeviceSequenceStore")
        if torch.is_tensor(labels):
            if labels.dtype != torch.int64 or labels.device != store.device:
                raise ValueError("DeviceSequenceDataset: a tensor of labels must be int64 on the store's device")
            labels_device = labels.contiguous()
        else:
            host = np.asarray(labels)
            if host.dtype.kind not in "iub":
                raise ValueError(f"DeviceSequenceDataset: labels must be integers, got {host.dtype}")
            labels_device = torch.from_numpy(host.astype(np.int64).reshape(-1)).to(store.device)
        if labels_device.dim() != 1 or labels_device.numel() != len(store):
            raise ValueError(f"DeviceSequenceDataset: {labels_device.numel()} labels for a store of {len(store)} sequences "
                             "(labels are per sequence of the store; `indices` selects)")
        self.store, self.labels = store, labels_device
        idx = np.arange(len(store), dtype=np.int64) if indices is None else np.asarray(indices)
        if idx.dtype == np.bool_:
            idx = np.flatnonzero(idx)
        if idx.size and idx.dtype.kind not in "iu":
            raise ValueError(f"DeviceSequenceDataset: indices must be integers, got {idx.dtype}")
        idx = idx.astype(np.int64).reshape(-1)
        if idx.size and (idx.min() < -len(store) or idx.max() >= len(store)):
            raise IndexError(f"DeviceSequenceDataset: index outside a store of {len(store)} sequences")
        self.indices = np.where(idx < 0, idx + len(store), idx)
        if (transform is None) != (augment_stream is None):
            raise ValueError("DeviceSequenceDataset: transform and augment_stream go together: "
                             f"{'augment_stream' if transform is not None else 'transform'} is missing")
        if transform is not None and store.layers is not None:
            raise ValueError("DeviceSequenceDataset: transform is not supported over a store of layer stacks "
                             f"(layers={store.layers}): augmentations apply to plain [T, D] sequences")
        if transform is not None:
            transform = as_compose(transform, "DeviceSequenceDataset")
            if not isinstance(augment_stream, AugmentStream):
                raise TypeError(f"DeviceSequenceDataset: augment_stream is a {type(augment_stream).__name__}, not an AugmentStream")
            if len(store) > 2 ** 32:
                raise ValueError("DeviceSequenceDataset: a transform numbers the sequences of the store in 32 bits")
        self.transform, self.augment_stream = transform, augment_stream

    def subset(self, idx):
        return DeviceSequenceDataset(self.store, self.labels, self.indices[np.asarray(idx)], self.transform, self.augment_stream)

    def __len__(self):
        return int(self.indices.size)

    def __getitem__(self, i):
        s = int(self.indices[i])
        return self.store.sequence(s), self.labels[s]


class BatchPlan:
    """One batch of an epoch, not yet assembled: where its members' rows, counts and label indices stand in the
    epoch's device arrays, and the host-side sizes (``B``, ``T`` = its longest member, ``frames`` = what it copies).
    ``epoch``: the epoch of the data set's ``AugmentStream`` that this batch is drawn at (``None``: no transform);
    ``label_index`` holds the members' store indices, which are also their sample ids.  Over a store of layer stacks
    ``row_start`` holds the first arena row of every member's block (``layers * frame_off``) and ``layers`` is the store's L;
    ``row_count`` and ``frames`` stay in frames."""
    __slots__ = ("dataset", "row_start", "row_count", "label_index", "first", "B", "T", "frames", "epoch", "layers")

    def __init__(self, dataset, row_start, row_count, label_index, first, B, T, frames, epoch=None, layers=None):
        self.dataset, self.row_start, self.row_count, self.label_index = dataset, row_start, row_count, label_index
        self.first, self.B, self.T, self.frames, self.epoch, self.layers = first, B, T, frames, epoch, layers


class _EpochPlans:
    """Iterator over the ``BatchPlan`` of one epoch.  Like ``iter(DataLoader)`` it draws the base seed when it is made and
    the epoch's order when the first batch is asked for."""

    def __init__(self, loader):
        self.loader = loader
        _draw_base_seed(loader.generator)
        self.plans = None

    def __iter__(self):
        return self

    def _prepare(self):
        ld = self.loader
        ds, store = ld.dataset, ld.dataset.store
        batches = _draw_batches(len(ds), ld.batch_size, ld.shuffle, ld.generator, ld.drop_last)
        epoch = ds.augment_stream.take_epoch() if ds.transform is not None else None
        plans = []
        if batches:
            order = ds.indices[np.concatenate([np.asarray(b, dtype=np.int64) for b in batches])]    # store indices, epoch order
            with torch.cuda.device(store.device):
                staged = torch.from_numpy(order).pin_memory()
                order_device = staged.to(store.device, non_blocking=True)
                row_start = store.frame_off_device[order_device]
                row_count = (store.frame_off_device[order_device + 1] - row_start).to(torch.int32)
                if store.layers is not None:
                    row_start = row_start * store.layers                        # first arena row of the member's block
            lengths = store.lengths[order]
            first = 0
            for b in batches:
                ln = lengths[first:first + len(b)]
                plans.append(BatchPlan(ds, row_start, row_count, order_device, first, len(b), int(ln.max()), int(ln.sum()), epoch, store.layers))
                first += len(b)
        self.plans = iter(plans)

    def __next__(self):
        if self.plans is None:
            self._prepare()
        return next(self.plans)


class DeviceBatchLoader:
    """The counterpart of ``DataLoader(dataset, batch_size, shuffle, collate_fn=collate_fn, generator=generator,
    drop_last=drop_last)`` over a ``DeviceSequenceDataset``: the same batches in the same order (``batch_indices``), each
    ``(x [B, T, D] float32 right-zero-padded to the longest member, labels [B] int64)`` on the device, equal bit for bit to
    what ``collate_fn`` builds.  Every ``iter()`` uploads the epoch's order once (pinned, non-blocking), derives the
    members' arena rows, frame counts and label indices on the device, and takes each batch's T from the lengths the
    host keeps.  ``plans()`` gives the epoch's batches without assembling them, for ``collate_batches``.  Where the
    data set has a ``transform``, every epoch takes the next epoch number of its ``AugmentStream`` at the point where it
    draws its order (the first batch asked for)."""

    def __init__(self, dataset, batch_size=1, shuffle=False, generator=None, drop_last=False):
        if not isinstance(dataset, DeviceSequenceDataset):
            raise TypeError(f"DeviceBatchLoader: dataset is a {type(dataset).__name__}, not a DeviceSequenceDataset")
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size <= 0:
            raise ValueError(f"batch_size should be a positive integer value, but got batch_size={batch_size}")
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), bool(shuffle)
        self.generator, self.drop_last = generator, bool(drop_last)

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def plans(self):
        """Iterator over the ``BatchPlan`` of one epoch; it draws from the generator as ``iter()`` does."""
        return _EpochPlans(self)

    def __iter__(self):
        for plan in self.plans():
            yield collate_batches([plan])[0]


def _layer_members(plan):
    """The B * L (member, layer) pairs of a plan over a store of layer stacks as a plain plan of B * L members: pair
    (b, l) is the ``row_count[b]`` frames from arena row ``row_start[b] + l * row_count[b]`` on; no labels."""
    L, sl = plan.layers, slice(plan.first, plan.first + plan.B)
    count = plan.row_count[sl].to(torch.int64)
    layer = torch.arange(L, dtype=torch.int64, device=count.device)
    start = (plan.row_start[sl, None] + layer[None, :] * count[:, None]).reshape(-1).contiguous()
    count = count[:, None].expand(-1, L).reshape(-1).to(torch.int32).contiguous()
    return BatchPlan(plan.dataset, start, count, None, 0, plan.B * L, plan.T, plan.frames * L)


def collate_batches(plans):
    """``[(x, labels)]`` of the planned batches, assembled by one ``rsaf_collate_pad_group`` launch per
    ``train_group_max()`` plans of one store width (lists longer than that are split like every other group call).  Where
    any plan of a width comes from a data set with a ``transform``, all plans of that width go through
    ``rsaf_collate_augment_group`` instead, the plain ones with ``n_ops = 0``: still one launch, so the training and the
    validation batches of a step may share a call.

    A plan over a store of layer stacks gives ``(h [B, L, T, D], labels)``, the zero-padded stack, through the same launch:
    its B * L (member, layer) pairs are the members, their rows derived on the device.  That is the input of
    ``LayerMix.forward``; ``collate_mix_batches`` returns the mixed batch without building it."""
    from .cnnlstm_train import _launch_chunked
    plans = list(plans)
    for k, p in enumerate(plans):
        if not isinstance(p, BatchPlan):
            raise TypeError(f"collate_batches: entry {k} is a {type(p).__name__}, not a BatchPlan")
    stacked = [k for k, p in enumerate(plans) if p.layers is not None]
    if stacked:
        flat = list(plans)
        for k in stacked:
            flat[k] = _layer_members(plans[k])
        outs = collate_batches(flat)
        for k in stacked:
            p = plans[k]
            outs[k] = (outs[k][0].view(p.B, p.layers, p.T, p.dataset.store.width), p.dataset.labels[p.label_index[p.first:p.first + p.B]])
        return outs
    outs = [None] * len(plans)
    groups = {}
    for k, p in enumerate(plans):
        store = p.dataset.store
        groups.setdefault((store.device, store.width), []).append(k)
    for (device, width), members in groups.items():
        with torch.cuda.device(device):
            for k in members:
                p = plans[k]
                outs[k] = (torch.empty((p.B, p.T, width), dtype=torch.float32, device=device),
                           torch.empty((p.B,), dtype=torch.int64, device=device))
                if p.T == 0 and p.label_index is not None:      # members of no frames only: pad_sequence's [B, 0, D]; nothing to launch
                    outs[k][1].copy_(p.dataset.labels[p.label_index[p.first:p.first + p.B]])
            members = [k for k in members if plans[k].T > 0]

            def fill(it, k, j):
                p, store = plans[k], plans[k].dataset.store
                it.arena, it.arena_rows = store.arena.data_ptr(), int(store.arena.shape[0])
                it.row_start = p.row_start.data_ptr() + 8 * p.first
                it.row_count = p.row_count.data_ptr() + 4 * p.first
                it.B, it.T, it.out = p.B, p.T, outs[k][0].data_ptr()
                it.frames = p.frames
                if p.label_index is None:                       # the (member, layer) pairs of a stack: labels by the caller
                    return
                it.label_src, it.label_count = p.dataset.labels.data_ptr(), int(p.dataset.labels.numel())
                it.label_index = p.label_index.data_ptr() + 8 * p.first
                it.label_out = outs[k][1].data_ptr()

            if all(plans[k].epoch is None for k in members):
                _launch_chunked("rsaf_collate_pad_group", _lib.CollateItem, members, fill, width)
                continue

            def fill_augmented(it, k, j):
                fill(it, k, j)
                p = plans[k]
                if p.epoch is None:
                    it.n_ops = 0
                    return
                tf = p.dataset.transform
                it.ops, it.ops_host, it.n_ops = tf.table(device).data_ptr(), C.addressof(tf.table_host), len(tf)
                it.seed, it.epoch = p.dataset.augment_stream.seed, p.epoch
                it.sample_id = p.label_index.data_ptr() + 8 * p.first

            _launch_chunked("rsaf_collate_augment_group", _lib.CollateAugmentItem, members, fill_augmented, width)
    return outs


def epoch_iterator(loader):
    """What a lock-step loop iterates: the plans of a ``DeviceBatchLoader`` (assembled later, many per launch), or the
    batches of anything else."""
    return loader.plans() if isinstance(loader, DeviceBatchLoader) else iter(loader)


def batches_to_device(batches, device):
    """``batches``: ``(x, labels)`` pairs of ``DataLoader``s and ``BatchPlan`` of device loaders in any mix -> list of
    ``(x, labels)`` on ``device``: the pairs copied as before, all plans assembled together by ``collate_batches``."""
    planned = [k for k, b in enumerate(batches) if isinstance(b, BatchPlan)]
    done = collate_batches([batches[k] for k in planned]) if planned else []
    out = [None if isinstance(b, BatchPlan) else (b[0].to(device), b[1].to(device)) for b in batches]
    for k, xb in zip(planned, done):
        out[k] = xb
    return out


def check_loader_devices(loaders, device, who):
    """A ``DeviceBatchLoader`` whose store is on another device than the models is refused by name."""
    for k, ld in enumerate(loaders):
        if not isinstance(ld, DeviceBatchLoader):
            continue
        want = _resolved(device)
        if ld.dataset.store.device != want:
            raise ValueError(f"{who}: loader {k} is a DeviceBatchLoader whose DeviceSequenceStore is on "
                             f"'{ld.dataset.store.device}', but the models are on '{want}'")
