"""Group eval forward of the CNN-LSTM (K eval-mode forwards in one call), the part that needs no GPU: the argument checks of
rsaf_cnnlstm_forward_group, which all run before the first HIP call, and the refusals of the Python layer, which come
before its device check."""
import ctypes as C

import pytest

DIMS = (16, 32, 64, 2, 2)            # input_dim, channels, hidden, num_classes, lstm_layers
ACT_SILU = 2
RSAF_ERR_ARG = 1
RSAF_ERR_WORKSPACE = 3
FAKE = 0x10000                       # never dereferenced: every call below returns from the checks
NAME = "rsaf_cnnlstm_forward_group"


def make_items(lib, shapes, dims=DIMS):
    from robust_speech_analysis_framework_amd import _lib
    D, Cc, H, NC, L = dims
    items = (_lib.ForwardItem * len(shapes))()
    base = FAKE
    for it, (B, T) in zip(items, shapes):
        it.B, it.T = B, T
        it.workspace_bytes = max(int(lib.rsaf_cnnlstm_workspace_bytes(B, T, D, Cc, H, L)), 0)
        for name in ("x", "weights", "workspace", "logits"):
            setattr(it, name, base)
            base += 1 << 32          # far apart: nothing overlaps unless a test makes it
    return items


def call(lib, items, K, dims=DIMS):
    rc = lib.rsaf_cnnlstm_forward_group(items, K, *dims, ACT_SILU, None)
    return rc, lib.rsaf_last_error().decode()


@pytest.mark.parametrize("K", [0, 17, -1])
def test_group_size_out_of_range_is_refused(rsaf_lib, K):
    rc, msg = call(rsaf_lib, make_items(rsaf_lib, [(2, 8)] * 17), K)
    assert rc == RSAF_ERR_ARG
    assert NAME in msg and "K must be in [1, 16]" in msg


def test_null_item_array_is_refused(rsaf_lib):
    rc, msg = call(rsaf_lib, None, 2)
    assert rc == RSAF_ERR_ARG and "items_host is NULL" in msg


def test_item_with_one_frame_is_refused_and_named(rsaf_lib):
    rc, msg = call(rsaf_lib, make_items(rsaf_lib, [(2, 8), (3, 12), (2, 1)]), 3)
    assert rc == RSAF_ERR_ARG
    assert NAME + ": item 2: " in msg and "sequence length must be >= 2" in msg


def test_item_with_an_empty_batch_is_refused_and_named(rsaf_lib):
    rc, msg = call(rsaf_lib, make_items(rsaf_lib, [(2, 8), (0, 12), (2, 8)]), 3)
    assert rc == RSAF_ERR_ARG
    assert NAME + ": item 1: " in msg and "batch must be in [1, 65535]" in msg


def test_null_weights_in_item_one_are_refused(rsaf_lib):
    items = make_items(rsaf_lib, [(2, 8), (2, 8)])
    items[1].weights = None
    rc, msg = call(rsaf_lib, items, 2)
    assert rc == RSAF_ERR_ARG and "item 1: NULL pointer" in msg


def test_workspace_one_byte_short_in_item_zero(rsaf_lib):
    items = make_items(rsaf_lib, [(2, 8), (2, 8)])
    items[0].workspace_bytes -= 1
    rc, msg = call(rsaf_lib, items, 2)
    assert rc == RSAF_ERR_WORKSPACE and "item 0" in msg and "workspace" in msg


@pytest.mark.parametrize("field", ["workspace", "logits"])
def test_items_sharing_workspace_or_logits_are_refused_and_named(rsaf_lib, field):
    items = make_items(rsaf_lib, [(2, 8), (3, 12), (2, 8)])
    setattr(items[2], field, getattr(items[0], field))
    rc, msg = call(rsaf_lib, items, 3)
    assert rc == RSAF_ERR_ARG
    assert "item 2" in msg and field in msg and "item 0" in msg
    # a partial overlap counts as well: item 1 starts inside item 0's range
    items = make_items(rsaf_lib, [(2, 8), (3, 12)])
    setattr(items[1], field, getattr(items[0], field) + 4)
    rc, msg = call(rsaf_lib, items, 2)
    assert rc == RSAF_ERR_ARG and "item 1" in msg and field in msg and "item 0" in msg


def test_items_sharing_weights_pass_the_checks(rsaf_lib):
    """Several batches of one model carry the same blob.  The dims are checked after the items and their overlaps, so a
    call that is refused for hidden = 96 has passed them, and nothing launches."""
    hidden96 = (16, 32, 96, 2, 2)
    items = make_items(rsaf_lib, [(2, 8), (3, 12), (2, 8)], hidden96)
    items[1].weights = items[2].weights = items[0].weights
    rc, msg = call(rsaf_lib, items, 3, hidden96)
    assert rc == RSAF_ERR_ARG
    assert "lstm_hidden_dim must be 64 or 128" in msg and "item" not in msg and "shares" not in msg
    # the same call with a shared workspace stops at the overlap: the order of the checks is what the first half relies on
    items[2].workspace = items[0].workspace
    rc, msg = call(rsaf_lib, items, 3, hidden96)
    assert rc == RSAF_ERR_ARG and "item 2" in msg and "workspace" in msg and "item 0" in msg


def test_the_single_entry_names_no_item(rsaf_lib):
    rc = rsaf_lib.rsaf_cnnlstm_forward(FAKE, 2, 1, *DIMS, ACT_SILU, FAKE, FAKE, 1 << 30, FAKE, None)
    msg = rsaf_lib.rsaf_last_error().decode()
    assert rc == RSAF_ERR_ARG and "rsaf_cnnlstm_forward:" in msg and "item" not in msg and "sequence length" in msg
    assert rsaf_lib.rsaf_cnnlstm_forward(FAKE, 2, 8, *DIMS, ACT_SILU, FAKE, FAKE, 16, FAKE, None) == RSAF_ERR_WORKSPACE
    assert rsaf_lib.rsaf_cnnlstm_forward(None, 0, 8, *DIMS, ACT_SILU, None, None, 0, None, None) == 0      # an empty batch is no work


def test_forward_item_matches_the_header_layout():
    """``_lib.ForwardItem`` mirrors rsaf_cnnlstm_forward_item field by field (LP64: 5 pointers/int64 + 2 ints = 48 bytes)."""
    from robust_speech_analysis_framework_amd import _lib
    names = [n for n, _ in _lib.ForwardItem._fields_]
    assert names == ["x", "B", "T", "weights", "workspace", "workspace_bytes", "logits"]
    assert C.sizeof(_lib.ForwardItem) == 48 and _lib.ForwardItem.weights.offset == 16


# ---- Python layer ---------------------------------------------------------------------------------------------------------
def model(D=16, Cc=32, H=64, act="silu"):
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM
    return CNNLSTM(input_dim=D, cnn_out_channels=Cc, lstm_hidden_dim=H, activation_fn=act).eval()


def x(B=2, T=8, D=16):
    import torch
    return torch.zeros((B, T, D))


def test_python_refusals_come_before_any_device_use(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group
    with pytest.raises(ValueError, match="at least one"):
        cnnlstm_forward_group([], [])
    with pytest.raises(ValueError, match="2 models but 1 inputs"):
        cnnlstm_forward_group([model(), model()], [x()])
    with pytest.raises(ValueError, match=r"'hidden': 128.*'hidden': 64"):
        cnnlstm_forward_group([model(), model(H=128)], [x(), x()])
    with pytest.raises(ValueError, match="'gelu'.*'silu'"):
        cnnlstm_forward_group([model(), model(act="gelu")], [x(), x()])
    with pytest.raises(ValueError, match="replica 1 is in training mode: "):
        cnnlstm_forward_group([model(), model().train()], [x(), x()])
    with pytest.raises(ValueError, match=r"replica 1: expected input \[B, T, 16\]"):
        cnnlstm_forward_group([model(), model()], [x(), torch.zeros((2, 8))])
    with pytest.raises(ValueError, match=r"replica 0: expected input \[B, T, 16\]"):
        cnnlstm_forward_group([model(), model()], [x(D=24), x()])
    with pytest.raises(ValueError, match="replica 1: sequence length must be >= 2"):
        cnnlstm_forward_group([model(), model()], [x(), x(T=1)])
    m = model()
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):          # one module twice is what a validation loader gives
        cnnlstm_forward_group([m, m], [x(), x(B=3, T=11)])


def test_group_module_and_loops_refuse_before_any_device_use(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import (CNNLSTMGroup, eval_replicas_lockstep,
                                                              train_eval_replicas_lockstep)
    import src.models as sm
    assert sm.cnnlstm_forward_group and sm.eval_model_grouped and sm.eval_replicas_lockstep is eval_replicas_lockstep
    assert sm.train_eval_replicas_lockstep is train_eval_replicas_lockstep
    g = CNNLSTMGroup([model(), model(), model()]).eval()
    assert g([None, None, None]) == [None, None, None]
    with pytest.raises(_lib.RsafError, match="cnnlstm_forward_group needs HIP"):
        g([x(), None, x()])
    g.models[1].train()
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):          # the group's own mode decides the path
        g([x(), None, x()])
    with pytest.raises(ValueError, match="2 models but 1 loaders"):
        eval_replicas_lockstep([model(), model()], [[]], "cpu")
    with pytest.raises(ValueError, match="2 models, 1 optimizers"):
        train_eval_replicas_lockstep([model(), model()], [None], [None, None], [[], []], [[], []], None, 1, 1, "cpu")
