"""Augmentations of the device-resident training data: the counterpart of ``SequenceDataset(..., transform=...)``
(``src/dl_cv_strategies.py:19-62``) for ``DeviceSequenceDataset``.

The transforms here run inside the collate launch (``rsaf_collate_augment_group``): every augmented value is a pure function
of (seed, epoch, sample, op, element) through the counter-based Philox4x32-10 that ``DropoutStream`` uses for the dropout
masks, so an augmented member has the same bits in any batch, in any group of replicas and in a sequential or a lock-step
training.  The mapping is documented in ``include/rsaf.h`` and coded once in ``csrc/augment_rng.h``.

* ``Scale``, ``GaussianNoise``, ``TimeMask``, ``FeatureMask``: ops on one sequence ``[T, D]``; none changes T;
* ``Compose``: up to ``RSAF_AUGMENT_MAX`` of them, applied in list order;
* ``AugmentStream``: ``seed`` names the stream, ``epoch`` counts the epochs that consulted it.

All of it is host state.  There is no CPU implementation: the ops describe what the kernel does.  ``cnnlstm`` re-exports
the names of this module.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

RSAF_AUGMENT_MAX = 8

_KIND_SCALE, _KIND_GAUSSIAN_NOISE, _KIND_TIME_MASK, _KIND_FEATURE_MASK = 0, 1, 2, 3


def _number(who, name, value):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: {name} must be a number, got {type(value).__name__}")
    value = float(value)
    if not math.isfinite(value):
        raise ValueError(f"{who}: {name} must be finite, got {value}")
    return value


class _Op:
    """One op of a pipeline: ``kind`` and the range ``[lo, hi]`` its parameter is drawn from, applied with probability
    ``p``.  ``lo_name`` / ``hi_name``: what the arguments are called, for the messages."""
    kind = None
    lo_name = hi_name = None

    def _init(self, lo, hi, p):
        who = type(self).__name__
        self.lo, self.hi, self.p = _number(who, self.lo_name, lo), _number(who, self.hi_name, hi), _number(who, "p", p)
        if not 0.0 <= self.p <= 1.0:
            raise ValueError(f"{who}: p must be in [0, 1], got {self.p}")
        if self.lo > self.hi:
            raise ValueError(f"{who}: {self.lo_name} must be <= {self.hi_name}, got {self.lo} > {self.hi}")

    def row(self):
        """``(kind, fire_threshold, always, a, b)`` as ``rsaf_augment_op`` takes them."""
        always = self.p >= 1.0
        return self.kind, 0xFFFFFFFF if always else int(math.floor(self.p * 2.0 ** 32)), int(always), self.lo, self.hi

    def __repr__(self):
        return f"{type(self).__name__}({self.lo_name}={self.lo}, {self.hi_name}={self.hi}, p={self.p})"


class Scale(_Op):
    """Multiplies the whole sequence by one factor drawn from ``[min_factor, max_factor]``."""
    kind, lo_name, hi_name = _KIND_SCALE, "min_factor", "max_factor"

    def __init__(self, min_factor, max_factor, p=0.5):
        self._init(min_factor, max_factor, p)


class GaussianNoise(_Op):
    """Adds ``amplitude * z``, ``z ~ N(0, 1)`` per element, one amplitude per sequence drawn from ``[min_amplitude,
    max_amplitude]`` (the parameters of audiomentations' ``AddGaussianNoise``)."""
    kind, lo_name, hi_name = _KIND_GAUSSIAN_NOISE, "min_amplitude", "max_amplitude"

    def __init__(self, min_amplitude=0.001, max_amplitude=0.015, p=0.5):
        self._init(min_amplitude, max_amplitude, p)
        if self.lo < 0.0:
            raise ValueError(f"GaussianNoise: min_amplitude must be >= 0, got {self.lo}")


class _Mask(_Op):
    lo_name, hi_name = "min_band_part", "max_band_part"

    def __init__(self, min_band_part=0.0, max_band_part=0.5, p=0.5):
        self._init(min_band_part, max_band_part, p)
        for name, v in ((self.lo_name, self.lo), (self.hi_name, self.hi)):
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"{type(self).__name__}: {name} must be in [0, 1], got {v}")


class TimeMask(_Mask):
    """Zeroes a contiguous span of frames: between ``min_band_part`` and ``max_band_part`` of the sequence's own T."""
    kind = _KIND_TIME_MASK


class FeatureMask(_Mask):
    """Zeroes a contiguous band of the D columns in every frame."""
    kind = _KIND_FEATURE_MASK


class Compose:
    """At most ``RSAF_AUGMENT_MAX`` ops, applied in list order (repeats allowed).  The op table is kept as one small
    device tensor per device, uploaded when first used there and not again."""

    def __init__(self, ops):
        ops = list(ops)
        for k, op in enumerate(ops):
            if not isinstance(op, _Op):
                raise TypeError(f"Compose: entry {k} is a {type(op).__name__}, not one of Scale, GaussianNoise, TimeMask, FeatureMask")
        if len(ops) > RSAF_AUGMENT_MAX:
            raise ValueError(f"Compose: {len(ops)} ops, at most RSAF_AUGMENT_MAX = {RSAF_AUGMENT_MAX}")
        self.ops = tuple(ops)
        self.table_host = (_lib.AugmentOp * max(len(ops), 1))()      # what the entry's checks read
        for row, op in zip(self.table_host, ops):
            row.kind, row.fire_threshold, row.always, row.a, row.b = op.row()
        self._tables = {}

    def __len__(self):
        return len(self.ops)

    def table(self, device):
        """The op table on ``device`` (uint8 view of ``rsaf_augment_op[len(self)]``)."""
        device = torch.device(device)
        if device not in self._tables:
            host = np.frombuffer(self.table_host, dtype=np.uint8).copy()
            self._tables[device] = torch.from_numpy(host).to(device)
        return self._tables[device]

    def __repr__(self):
        return f"Compose([{', '.join(repr(op) for op in self.ops)}])"


def as_compose(transform, who):
    """``transform`` as a ``Compose``; anything that is no transform of this module is refused by name."""
    if isinstance(transform, Compose):
        return transform
    if isinstance(transform, _Op):
        return Compose([transform])
    what = "a host callable" if callable(transform) else f"a {type(transform).__name__}"
    raise TypeError(f"{who}: transform is {what}; the device path takes Compose, Scale, GaussianNoise, TimeMask and FeatureMask of "
                    "this package (they run inside the collate launch).  Host callables stay with "
                    "torch.utils.data.DataLoader(SequenceDataset(..., transform=...))")


class AugmentStream:
    """Where a data set's augmentations come from: ``seed`` (0 <= seed < 2**64) names the stream, ``epoch``
    (0 <= epoch < 2**32) counts the epochs that consulted it.  Every augmented value is a pure function of (seed, epoch,
    sample, op, element) (``rsaf_collate_augment_group``, include/rsaf.h), so ``state_dict()`` is all a checkpoint needs to
    continue a run.  Host state only."""

    def __init__(self, seed, epoch=0):
        self.load_state_dict({"seed": seed, "epoch": epoch})

    def state_dict(self):
        return {"seed": self.seed, "epoch": self.epoch}

    def load_state_dict(self, state):
        seed, epoch = int(state["seed"]), int(state["epoch"])
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"AugmentStream: seed must be in [0, 2**64), got {seed}")
        if not 0 <= epoch < 2 ** 32:
            raise ValueError(f"AugmentStream: epoch must be in [0, 2**32), got {epoch}")
        self.seed, self.epoch = seed, epoch

    def take_epoch(self):
        """The epoch number of the epoch that starts now; the stream moves on to the next."""
        if self.epoch >= 2 ** 32 - 1:
            raise ValueError("AugmentStream: epoch would reach 2**32")
        self.epoch += 1
        return self.epoch - 1

    def __repr__(self):
        return f"AugmentStream(seed={self.seed}, epoch={self.epoch})"
