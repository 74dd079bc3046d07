"""The argument checks of the input-gradient entries (rsaf_cnnlstm_train_backward_dx, _backward_group_dx,
_backward_group_mixed_dx), which all run before the first HIP call and name the item.  The pointers are never dereferenced:
every call below returns from the checks."""
import ctypes as C

import pytest

DIMS = (16, 32, 64, 2, 2)            # input_dim, channels, hidden, num_classes, lstm_layers
ACT_SILU = 2
RSAF_ERR_ARG = 1
RSAF_ERR_WORKSPACE = 3
FAKE = 0x10000
FAR = 1 << 32                        # between any two fake buffers: nothing overlaps unless a test makes it


def make_items(lib, shapes, dx=None):
    """Backward items of DIMS; ``dx[k]`` false: item k wants no input gradient (dx and dx_scratch NULL)."""
    from robust_speech_analysis_framework_amd import _lib
    D, Cc, H, NC, L = DIMS
    items = (_lib.TrainDxItem * len(shapes))()
    base = FAKE
    for k, (it, (B, T)) in enumerate(zip(items, shapes)):
        it.B, it.T = B, T
        it.saved_floats = int(lib.rsaf_cnnlstm_train_saved_floats(B, T, D, Cc, H, L))
        it.scratch_floats = int(lib.rsaf_cnnlstm_train_scratch_floats(B, T, D, Cc, H, L))
        names = ["x", "params", "saved", "scratch", "dlogits", "grads"]
        if dx is None or dx[k]:
            names += ["dx", "dx_scratch"]
            it.dx_scratch_floats = int(lib.rsaf_cnnlstm_train_dx_scratch_floats(D, Cc))
        for name in names:
            setattr(it, name, base)
            base += FAR
    return items


def entries(lib):
    from robust_speech_analysis_framework_amd import _lib
    arch = (_lib.Arch * 16)(*[_lib.Arch(DIMS[1], DIMS[2], ACT_SILU)] * 16)
    return (("rsaf_cnnlstm_train_backward_group_dx", lambda items, K: lib.rsaf_cnnlstm_train_backward_group_dx(items, K, *DIMS, ACT_SILU, None)),
            ("rsaf_cnnlstm_train_backward_group_mixed_dx",
             lambda items, K: lib.rsaf_cnnlstm_train_backward_group_mixed_dx(items, arch, K, DIMS[0], DIMS[3], DIMS[4], None)))


def test_dx_item_extends_the_train_item():
    """``rsaf_cnnlstm_train_dx_item`` = the fields of ``rsaf_cnnlstm_train_item``, then dx, dx_scratch, dx_scratch_floats."""
    from robust_speech_analysis_framework_amd import _lib
    assert _lib.TrainDxItem._fields_[:len(_lib.TrainItem._fields_)] == _lib.TrainItem._fields_
    assert [n for n, _ in _lib.TrainDxItem._fields_[len(_lib.TrainItem._fields_):]] == ["dx", "dx_scratch", "dx_scratch_floats"]
    assert C.sizeof(_lib.TrainDxItem) == 144 and _lib.TrainDxItem.dx.offset == 120
    for name, _ in _lib.TrainItem._fields_:
        assert getattr(_lib.TrainDxItem, name).offset == getattr(_lib.TrainItem, name).offset, name


def test_the_checks_of_the_plain_entries_apply(rsaf_lib):
    for name, fn in entries(rsaf_lib):
        for K in (0, 17):
            assert fn(make_items(rsaf_lib, [(2, 8)] * max(K, 1)), K) == RSAF_ERR_ARG
            assert name in rsaf_lib.rsaf_last_error().decode()
        items = make_items(rsaf_lib, [(2, 8), (3, 1), (2, 8)])
        items[1].saved_floats = items[1].scratch_floats = 1 << 20
        assert fn(items, 3) == RSAF_ERR_ARG
        assert "item 1" in rsaf_lib.rsaf_last_error().decode() and "sequence length" in rsaf_lib.rsaf_last_error().decode()
        items = make_items(rsaf_lib, [(2, 8), (2, 8)])
        items[1].grads = items[0].grads
        assert fn(items, 2) == RSAF_ERR_ARG
        assert "item 1: shares `grads` with item 0" in rsaf_lib.rsaf_last_error().decode()
        items = make_items(rsaf_lib, [(2, 8), (2, 8)])
        items[1].dlogits = None
        assert fn(items, 2) == RSAF_ERR_ARG
        assert "item 1: NULL pointer" in rsaf_lib.rsaf_last_error().decode()


def test_dx_scratch_is_required_and_sized(rsaf_lib):
    for name, fn in entries(rsaf_lib):
        items = make_items(rsaf_lib, [(2, 8), (3, 6)])
        items[1].dx_scratch = None
        assert fn(items, 2) == RSAF_ERR_ARG
        assert "item 1: dx without dx_scratch" in rsaf_lib.rsaf_last_error().decode()
        items = make_items(rsaf_lib, [(2, 8), (3, 6)])
        items[0].dx_scratch_floats -= 1
        assert fn(items, 2) == RSAF_ERR_WORKSPACE
        msg = rsaf_lib.rsaf_last_error().decode()
        assert name in msg and "item 0" in msg and "dx_scratch too small" in msg


@pytest.mark.parametrize("mine", ["dx", "dx_scratch"])
@pytest.mark.parametrize("other", ["x", "saved", "scratch", "grads"])
def test_dx_buffers_inside_the_items_own_buffers_are_refused(rsaf_lib, mine, other):
    for name, fn in entries(rsaf_lib):
        items = make_items(rsaf_lib, [(2, 8), (3, 6)])
        setattr(items[1], mine, getattr(items[1], other) + 16)              # four floats into the other buffer
        assert fn(items, 2) == RSAF_ERR_ARG, (name, mine, other)
        assert f"item 1: `{mine}` overlaps `{other}`" in rsaf_lib.rsaf_last_error().decode()
    items = make_items(rsaf_lib, [(2, 8)])
    items[0].dx_scratch = items[0].dx + 4 * (2 * 8 * 16 - 1)                # the last float of dx
    assert entries(rsaf_lib)[0][1](items, 1) == RSAF_ERR_ARG
    assert "`dx` overlaps `dx_scratch`" in rsaf_lib.rsaf_last_error().decode()


@pytest.mark.parametrize("mine", ["dx", "dx_scratch"])
@pytest.mark.parametrize("other", ["saved", "scratch", "grads", "dx", "dx_scratch"])
def test_dx_buffers_inside_another_items_buffers_are_refused(rsaf_lib, mine, other):
    for name, fn in entries(rsaf_lib):
        for a, b in ((1, 0), (0, 1)):                                       # the later item's into the earlier one's, and back
            items = make_items(rsaf_lib, [(2, 8), (3, 6)])
            setattr(items[a], mine, getattr(items[b], other))
            assert fn(items, 2) == RSAF_ERR_ARG, (name, mine, other, a)
            msg = rsaf_lib.rsaf_last_error().decode()
            assert "item 1: its `" in msg and "of item 0" in msg and f"`{mine}`" in msg and f"`{other}`" in msg, msg


def test_items_without_dx_pass_the_dx_checks(rsaf_lib):
    """dx == NULL: dx_scratch and its size are not looked at, and the item joins no dx overlap check."""
    from robust_speech_analysis_framework_amd import _lib
    D, Cc, H, NC, L = DIMS
    items = make_items(rsaf_lib, [(2, 8), (3, 6)], dx=[False, True])
    items[0].dx_scratch, items[0].dx_scratch_floats = items[1].dx, 0
    items[1].dx_scratch_floats -= 1                                         # so that the call still ends in the checks
    for name, fn in entries(rsaf_lib):
        assert fn(items, 2) == RSAF_ERR_WORKSPACE
        assert "item 1" in rsaf_lib.rsaf_last_error().decode()
    # the single entry: the same checks, and a message without an item
    it = make_items(rsaf_lib, [(2, 8)])[0]
    args = (it.x, 2, 8, *DIMS, ACT_SILU, it.params, None, None, None, None, it.saved, it.saved_floats, it.scratch, it.scratch_floats,
            it.dlogits, it.grads)
    assert rsaf_lib.rsaf_cnnlstm_train_backward_dx(*args, it.dx, it.dx_scratch, it.dx_scratch_floats - 1, None) == RSAF_ERR_WORKSPACE
    msg = rsaf_lib.rsaf_last_error().decode()
    assert "rsaf_cnnlstm_train_backward_dx:" in msg and "item" not in msg
    assert rsaf_lib.rsaf_cnnlstm_train_backward_dx(*args, it.dx, None, 0, None) == RSAF_ERR_ARG
    assert rsaf_lib.rsaf_cnnlstm_train_backward_dx(*args, it.saved + 64, it.dx_scratch, it.dx_scratch_floats, None) == RSAF_ERR_ARG
    assert "`dx` overlaps `saved`" in rsaf_lib.rsaf_last_error().decode()
    assert _lib.SIGNATURES["rsaf_cnnlstm_train_backward_dx"][1][:-4] == _lib.SIGNATURES["rsaf_cnnlstm_train_backward"][1][:-1]

