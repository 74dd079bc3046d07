"""Group training step of the CNN-LSTM (K replicas in one step), the part that needs no GPU: the argument checks of
rsaf_cnnlstm_train_forward_group / _backward_group, which all run before the first HIP call, and the refusals of the
Python layer, which come before its device check."""
import ctypes as C

import pytest

DIMS = (16, 32, 64, 2, 2)            # input_dim, channels, hidden, num_classes, lstm_layers
ACT_SILU = 2
RSAF_ERR_ARG = 1
RSAF_ERR_WORKSPACE = 3
FAKE = 0x10000                       # never dereferenced: every call below returns from the checks


def make_items(lib, shapes):
    from robust_speech_analysis_framework_amd import _lib
    D, Cc, H, NC, L = DIMS
    items = (_lib.TrainItem * len(shapes))()
    base = FAKE
    for it, (B, T) in zip(items, shapes):
        it.B, it.T = B, T
        it.saved_floats = max(int(lib.rsaf_cnnlstm_train_saved_floats(B, T, D, Cc, H, L)), 0)
        it.scratch_floats = max(int(lib.rsaf_cnnlstm_train_scratch_floats(B, T, D, Cc, H, L)), 0)
        for name in ("x", "params", "saved", "scratch", "logits", "dlogits", "grads"):
            setattr(it, name, base)
            base += 1 << 32          # far apart: nothing overlaps unless a test makes it
    return items


def both(lib):
    return (("rsaf_cnnlstm_train_forward_group", lib.rsaf_cnnlstm_train_forward_group),
            ("rsaf_cnnlstm_train_backward_group", lib.rsaf_cnnlstm_train_backward_group))


def test_group_max_is_sixteen(rsaf_lib):
    assert rsaf_lib.rsaf_cnnlstm_train_group_max() == 16


@pytest.mark.parametrize("K", [0, 17, -1])
def test_group_size_out_of_range_is_refused(rsaf_lib, K):
    items = make_items(rsaf_lib, [(2, 8)] * 17)
    for name, fn in both(rsaf_lib):
        assert fn(items, K, *DIMS, ACT_SILU, None) == RSAF_ERR_ARG
        msg = rsaf_lib.rsaf_last_error().decode()
        assert name in msg and "K must be in [1, 16]" in msg


def test_null_item_array_is_refused(rsaf_lib):
    for name, fn in both(rsaf_lib):
        assert fn(None, 2, *DIMS, ACT_SILU, None) == RSAF_ERR_ARG
        assert "items_host is NULL" in rsaf_lib.rsaf_last_error().decode()


def test_item_with_one_frame_is_refused_and_named(rsaf_lib):
    items = make_items(rsaf_lib, [(2, 8), (3, 12), (2, 1)])
    for name, fn in both(rsaf_lib):
        assert fn(items, 3, *DIMS, ACT_SILU, None) == RSAF_ERR_ARG
        msg = rsaf_lib.rsaf_last_error().decode()
        assert "item 2" in msg and "sequence length must be >= 2" in msg


def test_items_sharing_saved_are_refused_and_named(rsaf_lib):
    items = make_items(rsaf_lib, [(2, 8), (3, 12), (2, 8)])
    items[2].saved = items[0].saved
    for name, fn in both(rsaf_lib):
        assert fn(items, 3, *DIMS, ACT_SILU, None) == RSAF_ERR_ARG
        msg = rsaf_lib.rsaf_last_error().decode()
        assert "item 2" in msg and "saved" in msg and "item 0" in msg


def test_items_sharing_scratch_logits_or_grads_are_refused(rsaf_lib):
    for field, fns in (("scratch", (0, 1)), ("logits", (0,)), ("grads", (1,))):
        items = make_items(rsaf_lib, [(2, 8), (2, 8)])
        setattr(items[1], field, getattr(items[0], field))
        for i in fns:
            name, fn = both(rsaf_lib)[i]
            assert fn(items, 2, *DIMS, ACT_SILU, None) == RSAF_ERR_ARG, (field, name)
            msg = rsaf_lib.rsaf_last_error().decode()
            assert "item 1" in msg and field in msg


def test_per_item_checks_of_the_single_entries_apply(rsaf_lib):
    items = make_items(rsaf_lib, [(2, 8), (2, 8)])
    items[1].params = None
    for name, fn in both(rsaf_lib):
        assert fn(items, 2, *DIMS, ACT_SILU, None) == RSAF_ERR_ARG
        assert "item 1: NULL pointer" in rsaf_lib.rsaf_last_error().decode()
    items = make_items(rsaf_lib, [(2, 8), (2, 8)])
    items[0].saved_floats -= 1
    for name, fn in both(rsaf_lib):
        assert fn(items, 2, *DIMS, ACT_SILU, None) == RSAF_ERR_WORKSPACE
        assert "item 0" in rsaf_lib.rsaf_last_error().decode()
    items = make_items(rsaf_lib, [(2, 8)])
    for name, fn in both(rsaf_lib):
        assert fn(items, 1, 16, 32, 96, 2, 2, ACT_SILU, None) == RSAF_ERR_ARG          # hidden 96: refused as in the single entries
    # the messages of the single entries carry no item
    rc = rsaf_lib.rsaf_cnnlstm_train_forward(FAKE, 2, 1, *DIMS, ACT_SILU, FAKE, None, None, None, None, FAKE, 1, FAKE, 1, FAKE, None, None)
    assert rc == RSAF_ERR_ARG
    msg = rsaf_lib.rsaf_last_error().decode()
    assert "rsaf_cnnlstm_train_forward:" in msg and "item" not in msg and "sequence length" in msg


def test_train_item_matches_the_header_layout():
    """``_lib.TrainItem`` mirrors rsaf_cnnlstm_train_item field by field (LP64: 14 pointers/int64 + 2 ints = 120 bytes)."""
    from robust_speech_analysis_framework_amd import _lib
    names = [n for n, _ in _lib.TrainItem._fields_]
    assert names == ["x", "B", "T", "params", "mask_block1", "mask_block2", "mask_lstm_host", "mask_fc", "saved", "saved_floats",
                     "scratch", "scratch_floats", "logits", "bn_stats_out", "dlogits", "grads"]
    assert C.sizeof(_lib.TrainItem) == 120 and _lib.TrainItem.params.offset == 16


# ---- Python layer ---------------------------------------------------------------------------------------------------------
def model(D=16, Cc=32, H=64, act="silu"):
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM
    return CNNLSTM(input_dim=D, cnn_out_channels=Cc, lstm_hidden_dim=H, activation_fn=act).train()


def x(B=2, T=8, D=16):
    import torch
    return torch.zeros((B, T, D))


def test_python_refusals_come_before_any_launch(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_group
    with pytest.raises(ValueError, match="at least one"):
        cnnlstm_train_group([], [])
    with pytest.raises(ValueError, match="2 models but 1 inputs"):
        cnnlstm_train_group([model(), model()], [x()])
    with pytest.raises(ValueError, match=r"'hidden': 128.*'hidden': 64"):
        cnnlstm_train_group([model(), model(H=128)], [x(), x()])
    with pytest.raises(ValueError, match="'gelu'.*'silu'"):
        cnnlstm_train_group([model(), model(act="gelu")], [x(), x()])
    with pytest.raises(ValueError, match="replica 1 is in eval mode"):
        cnnlstm_train_group([model(), model().eval()], [x(), x()])
    m = model()
    with pytest.raises(ValueError, match="same module"):
        cnnlstm_train_group([m, m], [x(), x()])
    a, b = model(), model()
    b.fc.weight = a.fc.weight
    with pytest.raises(ValueError, match="share the parameter fc.weight"):
        cnnlstm_train_group([a, b], [x(), x()])
    with pytest.raises(ValueError, match=r"replica 1: expected input \[B, T, 16\]"):
        cnnlstm_train_group([model(), model()], [x(), torch.zeros((2, 8))])
    with pytest.raises(ValueError, match=r"replica 0: expected input \[B, T, 16\]"):
        cnnlstm_train_group([model(), model()], [x(D=24), x()])
    with pytest.raises(ValueError, match="replica 1: Expected more than 1 value per channel when training"):
        cnnlstm_train_group([model(), model()], [x(), x(B=1, T=3)])
    with pytest.raises(ValueError, match="mask sets"):
        cnnlstm_train_group([model(), model()], [x(), x()], masks=[None])
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        cnnlstm_train_group([model(), model()], [x(), x(B=3, T=11)])


def test_group_module_keys_and_refusals(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, CNNLSTMGroup
    import src.models as sm
    assert sm.CNNLSTMGroup is CNNLSTMGroup and sm.cnnlstm_train_group and sm.train_replicas_lockstep
    g = CNNLSTMGroup([model(), model(), model()])
    single = set(model().state_dict())
    assert set(g.state_dict()) == {f"models.{k}.{key}" for k in range(3) for key in single}
    fresh = CNNLSTM(input_dim=16, cnn_out_channels=32, lstm_hidden_dim=64)
    fresh.load_state_dict({k[len("models.1."):]: v for k, v in g.state_dict().items() if k.startswith("models.1.")})
    with pytest.raises(ValueError, match="3 replicas but 2 inputs"):
        g([x(), x()])
    with pytest.raises(ValueError):
        CNNLSTMGroup([])
    with pytest.raises(TypeError):
        CNNLSTMGroup([model(), model().fc])
    assert g([None, None, None]) == [None, None, None]
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        g.train()([x(), None, x()])
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        g.eval()([x(), None, None])


def test_lockstep_refuses_lists_of_different_length(rsaf_lib):
    from robust_speech_analysis_framework_amd.cnnlstm import train_replicas_lockstep
    with pytest.raises(ValueError, match="2 models, 1 optimizers and 2 loaders"):
        train_replicas_lockstep([model(), model()], [None], [[], []], None, 1, "cpu")
