"""Mixed groups of the CNN-LSTM (K replicas of different architecture in one call), the part that needs no GPU: the
argument checks of rsaf_cnnlstm_train_forward_group_mixed / _backward_group_mixed / rsaf_cnnlstm_forward_group_mixed, which
all run before the first HIP call, and the refusals of the Python layer, which come before its device check."""
import ctypes as C

import pytest

D, NC, L = 16, 2, 2                  # what a mixed group shares: input_dim, num_classes, lstm_layers
GELU, SILU = 1, 2
ARCHS = [(32, 64, SILU), (64, 128, GELU)]                     # channels, hidden, act
RSAF_ERR_ARG = 1
FAKE = 0x10000                       # never dereferenced: every call below returns from the checks
TRAIN = ("rsaf_cnnlstm_train_forward_group_mixed", "rsaf_cnnlstm_train_backward_group_mixed")
EVAL = "rsaf_cnnlstm_forward_group_mixed"


def archs(lib_mod, seq):
    return (lib_mod.Arch * len(seq))(*[lib_mod.Arch(*a) for a in seq])


def train_items(lib, shapes, arch_seq):
    from robust_speech_analysis_framework_amd import _lib
    items = (_lib.TrainItem * len(shapes))()
    base = FAKE
    for it, (B, T), (Cc, H, _) in zip(items, shapes, arch_seq):
        it.B, it.T = B, T
        it.saved_floats = max(int(lib.rsaf_cnnlstm_train_saved_floats(B, T, D, Cc, H, L)), 0)
        it.scratch_floats = max(int(lib.rsaf_cnnlstm_train_scratch_floats(B, T, D, Cc, H, L)), 0)
        for name in ("x", "params", "saved", "scratch", "logits", "dlogits", "grads"):
            setattr(it, name, base)
            base += 1 << 32          # far apart: nothing overlaps unless a test makes it
    return items


def eval_items(lib, shapes, arch_seq):
    from robust_speech_analysis_framework_amd import _lib
    items = (_lib.ForwardItem * len(shapes))()
    base = FAKE
    for it, (B, T), (Cc, H, _) in zip(items, shapes, arch_seq):
        it.B, it.T = B, T
        it.workspace_bytes = max(int(lib.rsaf_cnnlstm_workspace_bytes(B, T, D, Cc, H, L)), 0)
        for name in ("x", "weights", "workspace", "logits"):
            setattr(it, name, base)
            base += 1 << 32
    return items


def entries(lib, arch_seq, shapes):
    """(name, call(items, archs, K)) of the three mixed entries with well-formed items for ``arch_seq``."""
    out = [(name, getattr(lib, name), train_items(lib, shapes, arch_seq)) for name in TRAIN]
    out.append((EVAL, getattr(lib, EVAL), eval_items(lib, shapes, arch_seq)))
    return out


def refused(lib, rc, name, *words):
    msg = lib.rsaf_last_error().decode()
    assert rc == RSAF_ERR_ARG, (name, rc, msg)
    assert name in msg, msg
    for w in words:
        assert w in msg, (name, w, msg)


def test_arch_matches_the_header_layout():
    from robust_speech_analysis_framework_amd import _lib
    assert [n for n, _ in _lib.Arch._fields_] == ["channels", "hidden", "act"]
    assert C.sizeof(_lib.Arch) == 12


def test_null_arch_array_is_refused(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    for name, fn, items in entries(rsaf_lib, ARCHS, [(2, 8), (3, 12)]):
        refused(rsaf_lib, fn(items, None, 2, D, NC, L, None), name, "arch_host is NULL")
        refused(rsaf_lib, fn(None, archs(_lib, ARCHS), 2, D, NC, L, None), name, "items_host is NULL")


@pytest.mark.parametrize("K", [0, 17])
def test_group_size_out_of_range_is_refused(rsaf_lib, K):
    from robust_speech_analysis_framework_amd import _lib
    seq = (ARCHS * 9)[:17]
    for name, fn, items in entries(rsaf_lib, seq, [(2, 8)] * 17):
        refused(rsaf_lib, fn(items, archs(_lib, seq), K, D, NC, L, None), name, "K must be in [1, 16]")


def test_item_with_hidden_96_is_refused_and_named(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    seq = [ARCHS[0], ARCHS[1], (32, 96, SILU)]
    for name, fn, items in entries(rsaf_lib, seq, [(2, 8), (3, 12), (2, 8)]):
        refused(rsaf_lib, fn(items, archs(_lib, seq), 3, D, NC, L, None), name, ": item 2: ", "lstm_hidden_dim must be 64 or 128")


def test_item_with_an_unknown_activation_is_refused_and_named(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    seq = [ARCHS[0], (32, 64, 3)]
    for name, fn, items in entries(rsaf_lib, seq, [(2, 8), (3, 12)]):
        refused(rsaf_lib, fn(items, archs(_lib, seq), 2, D, NC, L, None), name, ": item 1: ", "activation")


def test_buffers_sized_for_another_architecture_are_refused_and_named(rsaf_lib):
    """The items are sized for (32, 64), (64, 128); calling them as (64, 128), (64, 128) leaves item 0 too small, and as
    (32, 64), (64, 128) with item 1's sizes taken from item 0 leaves item 1 too small."""
    from robust_speech_analysis_framework_amd import _lib
    shapes = [(2, 8), (2, 8)]
    for name, fn, items in entries(rsaf_lib, ARCHS, shapes):
        refused(rsaf_lib, fn(items, archs(_lib, [ARCHS[1], ARCHS[1]]), 2, D, NC, L, None), name, ": item 0: ", "too small", "architecture")
    for name, fn, items in entries(rsaf_lib, ARCHS, shapes):
        if name == EVAL:
            items[1].workspace_bytes = items[0].workspace_bytes
        else:
            items[1].saved_floats = items[0].saved_floats
        refused(rsaf_lib, fn(items, archs(_lib, ARCHS), 2, D, NC, L, None), name, ": item 1: ", "too small", "architecture")
    # the scratch buffer alone, one float short
    for name, fn, items in entries(rsaf_lib, ARCHS, shapes)[:2]:
        items[1].scratch_floats -= 1
        refused(rsaf_lib, fn(items, archs(_lib, ARCHS), 2, D, NC, L, None), name, ": item 1: ", "too small")


def test_per_item_checks_of_the_group_entries_apply(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    a = archs(_lib, ARCHS + ARCHS[:1])
    seq = ARCHS + ARCHS[:1]
    for name, fn, items in entries(rsaf_lib, seq, [(2, 8), (3, 12), (2, 1)]):
        refused(rsaf_lib, fn(items, a, 3, D, NC, L, None), name, ": item 2: ", "sequence length must be >= 2")
    for name, fn, items in entries(rsaf_lib, seq, [(2, 8), (3, 12), (2, 8)]):
        items[1].x = None
        refused(rsaf_lib, fn(items, a, 3, D, NC, L, None), name, ": item 1: NULL pointer")
    # overlaps are found with every item's own sizes: item 1 (the larger architecture) starts inside item 0's range
    for name, fn, items in entries(rsaf_lib, seq, [(2, 8), (3, 12), (2, 8)]):
        if name == EVAL:
            items[1].workspace = items[0].workspace + 16
            what = "workspace"
        else:
            items[1].saved = items[0].saved + 16
            what = "saved"
        refused(rsaf_lib, fn(items, a, 3, D, NC, L, None), name, ": item 1: ", what, "item 0")
    # the gradient blobs have the length of their own architecture: item 0's (the smaller) ends before item 1's begins
    n0 = int(rsaf_lib.rsaf_cnnlstm_train_param_floats(D, ARCHS[0][0], ARCHS[0][1], NC, L))
    n1 = int(rsaf_lib.rsaf_cnnlstm_train_param_floats(D, ARCHS[1][0], ARCHS[1][1], NC, L))
    assert 0 < n0 < n1
    name, fn, items = entries(rsaf_lib, ARCHS, [(2, 8), (2, 8)])[1]
    items[0].grads = items[1].grads + 4 * (n1 - 1)            # the last float of item 1's blob
    refused(rsaf_lib, fn(items, archs(_lib, ARCHS), 2, D, NC, L, None), name, ": item 1: ", "grads", "item 0")
    # shared dims out of range name the item they are first met in
    for name, fn, items in entries(rsaf_lib, ARCHS, [(2, 8), (2, 8)]):
        refused(rsaf_lib, fn(items, archs(_lib, ARCHS), 2, D, NC, 5, None), name, ": item 0: ", "lstm_layers must be in [1, 4]")


def test_eval_items_sharing_weights_must_share_an_architecture(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    fn = getattr(rsaf_lib, EVAL)
    seq = [ARCHS[0], ARCHS[1], (32, 64, GELU)]
    items = eval_items(rsaf_lib, [(2, 8), (3, 12), (2, 8)], seq)
    items[2].weights = items[0].weights                       # (32, 64, silu) and (32, 64, gelu): the activation differs
    refused(rsaf_lib, fn(items, archs(_lib, seq), 3, D, NC, L, None), EVAL, ": item 2: ", "weights", "item 0", "architecture")
    items = eval_items(rsaf_lib, [(2, 8), (3, 12)], ARCHS)
    items[1].weights = items[0].weights
    refused(rsaf_lib, fn(items, archs(_lib, ARCHS), 2, D, NC, L, None), EVAL, ": item 1: ", "weights", "item 0")


# ---- Python layer ---------------------------------------------------------------------------------------------------------
def model(Dm=16, Cc=32, H=64, act="silu", nc=2, layers=2):
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM
    return CNNLSTM(input_dim=Dm, num_classes=nc, cnn_out_channels=Cc, lstm_hidden_dim=H, lstm_layers=layers, activation_fn=act)


def x(B=2, T=8, Dm=16):
    import torch
    return torch.zeros((B, T, Dm))


CASES = [("input_dim", dict(Dm=24)), ("num_classes", dict(nc=3)), ("layers", dict(layers=1))]


@pytest.mark.parametrize("field,kw", CASES)
def test_mixed_groups_refuse_what_they_must_share(rsaf_lib, field, kw):
    from robust_speech_analysis_framework_amd.cnnlstm import (FusedAdam, cnnlstm_forward_group, cnnlstm_train_group,
                                                              cnnlstm_train_step_group)
    pat = rf"replica 2 differs from replica 0 in {field}: "
    xs = [x(), x(), x(Dm=kw.get("Dm", 16))]
    ms = [model(), model(Cc=64, H=128, act="gelu"), model(**kw)]
    with pytest.raises(ValueError, match=pat):
        cnnlstm_train_group([m.train() for m in ms], xs, mixed=True)
    with pytest.raises(ValueError, match=pat):
        cnnlstm_forward_group([m.eval() for m in ms], xs, mixed=True)
    with pytest.raises(ValueError, match=pat):
        cnnlstm_train_step_group([m.train() for m in ms], [None] * 3, xs, [None] * 3, mixed=True)
    assert FusedAdam is not None


def test_mixed_groups_need_hip_tensors(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import (CNNLSTMGroup, cnnlstm_forward_group, cnnlstm_train_group,
                                                              eval_replicas_lockstep, train_eval_replicas_lockstep,
                                                              train_replicas_lockstep)
    ms = [model(), model(Cc=64, H=128, act="gelu")]
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        cnnlstm_train_group([m.train() for m in ms], [x(), x(B=3, T=11)], mixed=True)
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        cnnlstm_forward_group([m.eval() for m in ms], [x(), x(B=3, T=11)], mixed=True)
    # without the keyword the same lists are refused as before: the default does not change
    with pytest.raises(ValueError, match="replica 1 differs from replica 0: dims"):
        cnnlstm_forward_group(ms, [x(), x()])
    g = CNNLSTMGroup(ms, mixed=True)
    assert g.mixed and not CNNLSTMGroup(ms).mixed
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        g.train()([x(), x()])
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        g.eval()([x(), x()])
    loaders = [[(x(), torch.zeros(2, dtype=torch.int64))]] * 2
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        eval_replicas_lockstep(ms, loaders, "cpu", mixed=True)
    opts = [torch.optim.Adam(m.parameters()) for m in ms]
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        train_replicas_lockstep(ms, opts, loaders, torch.nn.CrossEntropyLoss(), 1, "cpu", mixed=True)
    with pytest.raises(_lib.RsafError, match="no CPU fallback"):
        train_eval_replicas_lockstep(ms, opts, [None, None], loaders, loaders, torch.nn.CrossEntropyLoss(), 1, 1, "cpu", mixed=True)
