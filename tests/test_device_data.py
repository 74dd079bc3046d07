"""Device-resident training data, the part that needs no GPU: batch_indices against DataLoader (order and RNG state), the
argument checks of rsaf_collate_pad_group (all before any launch), the item's size, and what DeviceSequenceStore refuses."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

PACKAGE = "robust_speech_analysis_framework_amd"


def _state(gen):
    return gen.get_state() if gen is not None else torch.get_rng_state()


@pytest.mark.parametrize("own_generator", [True, False], ids=["own_generator", "global_rng"])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("batch_size", [4, 5, 8])
@pytest.mark.parametrize("n", [1, 8, 12, 14, 19])
def test_batch_indices_equal_dataloader_order_and_rng_state(n, batch_size, drop_last, own_generator):
    from robust_speech_analysis_framework_amd.device_data import batch_indices
    for shuffle in (True, False):
        gen = torch.Generator().manual_seed(1234 + n) if own_generator else None
        torch.manual_seed(77)
        loader = DataLoader(list(range(n)), batch_size=batch_size, shuffle=shuffle, generator=gen, drop_last=drop_last,
                            collate_fn=lambda b: [int(v) for v in b])
        want = [list(loader) for _ in range(3)]
        want_state = _state(gen)
        gen = torch.Generator().manual_seed(1234 + n) if own_generator else None
        torch.manual_seed(77)
        got = [batch_indices(n, batch_size, shuffle, gen, drop_last) for _ in range(3)]
        assert got == want, (shuffle, got, want)
        assert torch.equal(_state(gen), want_state), "RNG state after three epochs differs from the DataLoader's"
        assert all(len(epoch) == len(loader) for epoch in got)


def test_names_are_on_cnnlstm_where_the_loops_are():
    import importlib
    mod, dd = importlib.import_module(f"{PACKAGE}.cnnlstm"), importlib.import_module(f"{PACKAGE}.device_data")
    for name in ("batch_indices", "DeviceSequenceStore", "DeviceSequenceDataset", "DeviceBatchLoader", "collate_batches"):
        assert getattr(mod, name) is getattr(dd, name), name


def test_collate_item_matches_the_header(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    it = _lib.CollateItem
    assert C.sizeof(it) == 88                     # static_assert(sizeof(rsaf_collate_item) == 88) in aggregate.hip
    assert [getattr(it, f).offset for f, _ in it._fields_] == [0, 8, 16, 24, 32, 36, 40, 48, 56, 64, 72, 80]
    assert rsaf_lib.rsaf_cnnlstm_train_group_max() == 16 and 16 * 88 <= 3584
    assert rsaf_lib.rsaf_abi_version() == 7


def _items(n, **over):
    """n well-formed items over fake, disjoint device addresses: nothing is launched when a check fires, nothing read."""
    from robust_speech_analysis_framework_amd import _lib
    items = (_lib.CollateItem * max(n, 1))()
    for k in range(n):
        it = items[k]
        it.arena, it.arena_rows, it.row_start, it.row_count = 0x10000000, 100, 0x20000000 + 64 * k, 0x21000000 + 64 * k
        it.B, it.T, it.out = 2, 3, 0x30000000 + 0x10000 * k
        it.label_src, it.label_count, it.label_index, it.label_out = 0x40000000, 50, 0x41000000 + 64 * k, 0x42000000 + 64 * k
        it.frames = -1
    for name, (k, v) in over.items():
        setattr(items[k], name, v)
    return items


CHECKS = {
    # name: (items, K, width, what rsaf_last_error() must contain)
    "K_0": (lambda: _items(1), 0, 8, "K must be in [1, 16]"),
    "K_17": (lambda: _items(17), 17, 8, "K must be in [1, 16]"),
    "items_NULL": (lambda: None, 1, 8, "items_host is NULL"),
    "width_0": (lambda: _items(2), 2, 0, "width"),
    "arena_NULL": (lambda: _items(3, arena=(2, None)), 3, 8, "item 2: NULL pointer"),
    "out_NULL": (lambda: _items(3, out=(1, None)), 3, 8, "item 1: NULL pointer"),
    "row_start_NULL": (lambda: _items(2, row_start=(1, None)), 2, 8, "item 1: NULL pointer"),
    "row_count_NULL": (lambda: _items(2, row_count=(0, None)), 2, 8, "item 0: NULL pointer"),
    "B_0": (lambda: _items(3, B=(2, 0)), 3, 8, "item 2: B and T must be >= 1"),
    "T_0": (lambda: _items(3, T=(1, 0)), 3, 8, "item 1: B and T must be >= 1"),
    "too_large": (lambda: _items(2, B=(1, 1 << 20), T=(1, 1 << 20)), 2, 8, "item 1: B * T * width must be < 2^40"),
    "label_out_alone_missing": (lambda: _items(3, label_out=(2, None)), 3, 8, "item 2: label_src, label_count, label_index and label_out"),
    "label_src_alone": (lambda: _items(2, label_index=(1, None), label_out=(1, None)), 2, 8, "item 1: label_src, label_count"),
    "label_count_alone": (lambda: _items(2, label_src=(0, None), label_index=(0, None), label_out=(0, None)), 2, 8,
                          "item 0: label_src, label_count"),
    "shared_out": (lambda: _items(3, out=(2, 0x30000000)), 3, 8, "item 2: `out` overlaps `out` of item 0"),
    "out_inside_another": (lambda: _items(3, out=(2, 0x30010000 + 2 * 3 * 8 * 4 - 4)), 3, 8, "item 2: `out` overlaps `out` of item 1"),
    "shared_label_out": (lambda: _items(2, label_out=(1, 0x42000000 + 8)), 2, 8, "item 1: `label_out` overlaps `label_out` of item 0"),
}


@pytest.mark.parametrize("case", sorted(CHECKS))
def test_collate_argument_checks_fire_before_any_launch(rsaf_lib, case):
    make, K, width, message = CHECKS[case]
    rc = rsaf_lib.rsaf_collate_pad_group(make(), K, width, None)
    err = rsaf_lib.rsaf_last_error().decode()
    assert rc == 1, (case, rc, err)                    # RSAF_ERR_ARG: refused by a check, not by a failed launch
    assert err.startswith("rsaf_collate_pad_group: ") and message in err, err


def test_store_refuses_a_cpu_device_and_mixed_widths():
    from robust_speech_analysis_framework_amd.device_data import (DeviceBatchLoader, DeviceSequenceDataset,
                                                                  DeviceSequenceStore)
    seqs = [np.zeros((3, 4)), np.zeros((5, 4))]
    with pytest.raises(ValueError, match="there is no CPU fallback"):
        DeviceSequenceStore(seqs, device="cpu")
    with pytest.raises(ValueError, match="sequence 1 has width 6, sequence 0 has 4"):
        DeviceSequenceStore([np.zeros((3, 4)), np.zeros((5, 6))])
    with pytest.raises(ValueError, match=r"expected \[T, D\]"):
        DeviceSequenceStore([np.zeros(3)])
    with pytest.raises(TypeError, match="not a DeviceSequenceStore"):
        DeviceSequenceDataset(seqs, [0, 1])
    with pytest.raises(TypeError, match="not a DeviceSequenceDataset"):
        DeviceBatchLoader(seqs, batch_size=4)
