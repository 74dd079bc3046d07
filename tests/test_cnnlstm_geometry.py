"""Host side of the CNN-LSTM geometry table (no GPU): the two blob layouts over every case of tests/cnnlstm_geometry.py,
and the geometries just outside the domain, which every entry refuses by name before it launches anything."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cnnlstm_geometry as geo  # noqa: E402

ALL = list(range(len(geo.CASES) + 1))             # the table and the one-class case


def cpu_model(i):
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM
    D, Cc, H, act, NC, L = geo.geometry(i)
    return CNNLSTM(input_dim=D, num_classes=NC, cnn_out_channels=Cc, lstm_hidden_dim=H, lstm_layers=L, activation_fn=act)


def tiles(offsets, sizes, total):
    """Segments of ``sizes`` floats at ``offsets`` (-1 with size None: absent) increase, do not overlap, start on the
    16-byte grid and fill ``total`` up to that padding."""
    assert len(offsets) == len(sizes), (len(offsets), len(sizes))
    end = 0
    for k, (o, n) in enumerate(zip(offsets, sizes)):
        if n is None:
            assert o == -1, (k, o)
            continue
        assert o >= end and o % 4 == 0, (k, o, end)
        end = o + n
    assert end <= total
    assert total == sum((n + 3) // 4 * 4 for n in sizes if n is not None)


def lstm_sizes(m):
    out = []
    for l in range(m.dims["layers"]):
        g = lambda n: getattr(m.lstm, n).numel()                                         # noqa: E731
        out += [g(f"weight_ih_l{l}") + g(f"weight_ih_l{l}_reverse"), g(f"bias_ih_l{l}") + g(f"bias_ih_l{l}_reverse"),
                g(f"weight_hh_l{l}") + g(f"weight_hh_l{l}_reverse")]
    aw = m.attention_pooling.attention_weights
    return out + [aw.weight.numel(), aw.bias.numel(), m.fc.weight.numel(), m.fc.bias.numel()]


@pytest.mark.parametrize("i", ALL, ids=geo.case_id)
def test_blob_layouts_tile_the_tensors_of_the_module(rsaf_lib, i):
    from robust_speech_analysis_framework_amd.cnnlstm import pack_weights, train_param_offsets, weight_offsets, _train_segments
    D, Cc, H, act, NC, L = geo.geometry(i)
    m = cpu_model(i).eval()
    r1, r2 = m.res_block1, m.res_block2
    has_sc = len(r1.shortcut) > 0
    assert has_sc == (D != Cc)
    convs = [r1.conv1, r1.shortcut[0] if has_sc else None, r1.conv2, r2.conv1, r2.conv2]
    bns = [r1.bn1, r1.shortcut[1] if has_sc else None, r1.bn2, r2.bn1, r2.bn2]
    # folded inference blob: (weight, bias) per convolution
    sizes = []
    for cv in convs:
        sizes += [None, None] if cv is None else [cv.weight.numel(), cv.bias.numel()]
    offs, total = weight_offsets(D, Cc, H, NC, L)
    tiles(offs, sizes + lstm_sizes(m), total)
    assert (offs[2] == -1 and offs[3] == -1) == (D == Cc)
    assert pack_weights(m).shape == (total,)
    # training blob: (weight, bias, gamma, beta) per convolution
    sizes = []
    for cv, bn in zip(convs, bns):
        sizes += [None] * 4 if cv is None else [cv.weight.numel(), cv.bias.numel(), bn.weight.numel(), bn.bias.numel()]
    offs, total = train_param_offsets(m.dims)
    tiles(offs, sizes + lstm_sizes(m), total)
    assert all(o == -1 for o in offs[4:8]) == (D == Cc)
    segs, total2 = _train_segments(m)
    assert total2 == total and [s.offset for s in segs] == [o for o in offs if o >= 0]
    assert [s.n for s in segs] == [n for n in sizes + lstm_sizes(m) if n is not None]
    n = rsaf_lib.rsaf_cnnlstm_adam_param_count(D, Cc, H, NC, L)
    assert n == len(list(m.parameters()))


OUTSIDE = [
    # D, C, H, NC, L, what the message names
    (16, 32, 32, 2, 2, "lstm_hidden_dim"),
    (16, 6, 64, 2, 2, "cnn_out_channels"),
    (10, 32, 64, 2, 2, "input_dim"),
    (16, 32, 64, 0, 2, "num_classes"),
    (16, 32, 64, 17, 2, "num_classes"),
    (16, 32, 64, 2, 0, "lstm_layers"),
    (16, 32, 64, 2, 5, "lstm_layers"),
]


def refused(rc, lib, word):
    assert rc != 0
    assert word.encode() in lib.rsaf_last_error(), (word, lib.rsaf_last_error())


@pytest.mark.parametrize("D,Cc,H,NC,L,word", OUTSIDE, ids=[f"d{c[0]}_c{c[1]}_h{c[2]}_nc{c[3]}_l{c[4]}" for c in OUTSIDE])
def test_geometries_outside_the_domain_are_refused_by_name(rsaf_lib, D, Cc, H, NC, L, word):
    """Every entry checks the dimensions first: with NULL operands and no device the calls below can only come back
    with the message of ``check_dims``."""
    from robust_speech_analysis_framework_amd import _lib
    lib = rsaf_lib
    buf, n = (C.c_int64 * 48)(), C.c_int(0)
    refused(lib.rsaf_cnnlstm_weight_offsets(D, Cc, H, NC, L, buf, 48, C.byref(n)), lib, word)
    refused(lib.rsaf_cnnlstm_train_param_offsets(D, Cc, H, NC, L, buf, 48, C.byref(n)), lib, word)
    assert lib.rsaf_cnnlstm_weight_floats(D, Cc, H, NC, L) == -1 and lib.rsaf_cnnlstm_train_param_floats(D, Cc, H, NC, L) == -1
    assert lib.rsaf_cnnlstm_adam_param_count(D, Cc, H, NC, L) == -1
    act = 2
    refused(lib.rsaf_cnnlstm_forward(None, 1, 4, D, Cc, H, NC, L, act, None, None, 0, None, None), lib, word)
    refused(lib.rsaf_cnnlstm_forward_stages(None, 1, 4, D, Cc, H, NC, L, act, None, None, 0, None, None, None, None, None, None),
            lib, word)
    refused(lib.rsaf_cnnlstm_train_forward(None, 2, 4, D, Cc, H, NC, L, act, None, None, None, None, None, None, 0, None, 0, None,
                                           None, None), lib, word)
    refused(lib.rsaf_cnnlstm_train_backward(None, 2, 4, D, Cc, H, NC, L, act, None, None, None, None, None, None, 0, None, 0, None,
                                            None, None), lib, word)
    refused(lib.rsaf_cnnlstm_train_forward_group((_lib.TrainItem * 1)(), 1, D, Cc, H, NC, L, act, None), lib, word)
    refused(lib.rsaf_cnnlstm_train_backward_group((_lib.TrainItem * 1)(), 1, D, Cc, H, NC, L, act, None), lib, word)
    refused(lib.rsaf_cnnlstm_adam_group((_lib.AdamItem * 1)(), 1, D, Cc, H, NC, L, None), lib, word)
    refused(lib.rsaf_cnnlstm_pack_params_group((_lib.PackItem * 1)(), 1, D, Cc, H, NC, L, None), lib, word)
    # the sizes of the training buffers depend on D, C, H and L only
    if word not in ("num_classes",):
        assert lib.rsaf_cnnlstm_train_saved_floats(2, 4, D, Cc, H, L) == -1
        assert lib.rsaf_cnnlstm_train_scratch_floats(2, 4, D, Cc, H, L) == -1


def test_group_forward_refuses_a_geometry_outside_the_domain_behind_its_item_checks(rsaf_lib):
    """rsaf_cnnlstm_forward_group names a bad item first (its message carries the item); with well-formed items the
    dimensions are refused by name, still in front of every launch.  The operands are host memory: whoever moves
    ``check_dims`` behind the first launch of rsaf_cnnlstm_forward_group turns this test, on a machine with a GPU, from a
    failing assertion into kernels started on host addresses.  Keep the check in front."""
    from robust_speech_analysis_framework_amd import _lib
    lib = rsaf_lib
    for D, Cc, H, NC, L, word in OUTSIDE:
        if word == "lstm_layers":                                  # the layouts cannot be computed: refused at once
            refused(lib.rsaf_cnnlstm_forward_group((_lib.ForwardItem * 1)(), 1, D, Cc, H, NC, L, 2, None), lib, word)
            continue
        need = lib.rsaf_cnnlstm_workspace_bytes(1, 4, D, Cc, H, L)
        assert need > 0
        bufs = [np.zeros(max(need // 4, 64), np.float32) for _ in range(4)]         # host memory: nothing may touch it
        it = (_lib.ForwardItem * 1)()
        it[0].x, it[0].weights, it[0].workspace, it[0].logits = [b.ctypes.data for b in bufs]
        it[0].B, it[0].T, it[0].workspace_bytes = 1, 4, need
        refused(lib.rsaf_cnnlstm_forward_group(it, 1, D, Cc, H, NC, L, 2, None), lib, word)
        assert all(not b.any() for b in bufs)


@pytest.mark.parametrize("i", range(len(geo.CASES)), ids=geo.case_id)
def test_buffers_one_float_short_are_refused_before_any_launch(rsaf_lib, i):
    """The entries accept exactly the sizes of their size queries: one float less is refused by name, in front of every
    launch (the operands are host memory that must stay untouched; see the remark on check order above)."""
    from robust_speech_analysis_framework_amd import _lib
    lib = rsaf_lib
    D, Cc, H, act, NC, L, B, T = geo.CASES[i]
    need = lib.rsaf_cnnlstm_workspace_bytes(B, T, D, Cc, H, L)
    n_saved, n_scr = lib.rsaf_cnnlstm_train_saved_floats(B, T, D, Cc, H, L), lib.rsaf_cnnlstm_train_scratch_floats(B, T, D, Cc, H, L)
    assert need > 0 and need % 4 == 0 and n_saved > 0 and n_scr > 0
    host = np.zeros(64, np.float32)
    hp = C.c_void_p(host.ctypes.data)
    refused(lib.rsaf_cnnlstm_forward(hp, B, T, D, Cc, H, NC, L, 2, hp, hp, need - 4, hp, None), lib, "workspace too small")
    it = (_lib.ForwardItem * 1)()
    it[0].x = it[0].weights = it[0].workspace = it[0].logits = host.ctypes.data
    it[0].B, it[0].T, it[0].workspace_bytes = B, T, need - 4
    refused(lib.rsaf_cnnlstm_forward_group(it, 1, D, Cc, H, NC, L, 2, None), lib, "workspace too small")
    for saved, scr in ((n_saved - 1, n_scr), (n_saved, n_scr - 1)):
        refused(lib.rsaf_cnnlstm_train_forward(hp, B, T, D, Cc, H, NC, L, 2, hp, None, None, None, None, hp, saved, hp, scr, hp,
                                               None, None), lib, "too small")
        refused(lib.rsaf_cnnlstm_train_backward(hp, B, T, D, Cc, H, NC, L, 2, hp, None, None, None, None, hp, saved, hp, scr, hp,
                                                hp, None), lib, "too small")
    assert not host.any()


def test_training_refuses_more_than_1024_channels_and_the_loss_one_class(rsaf_lib):
    from robust_speech_analysis_framework_amd import _lib
    lib = rsaf_lib
    buf, n = (C.c_int64 * 48)(), C.c_int(0)
    word = "cnn_out_channels"
    assert lib.rsaf_cnnlstm_weight_offsets(16, 1028, 64, 2, 2, buf, 48, C.byref(n)) == 0         # inference takes it
    refused(lib.rsaf_cnnlstm_train_param_offsets(16, 1028, 64, 2, 2, buf, 48, C.byref(n)), lib, word)
    assert b"1024" in lib.rsaf_last_error()
    assert lib.rsaf_cnnlstm_train_saved_floats(2, 4, 16, 1028, 64, 2) == -1
    assert lib.rsaf_cnnlstm_train_scratch_floats(2, 4, 16, 1028, 64, 2) == -1
    refused(lib.rsaf_cnnlstm_train_forward(None, 2, 4, 16, 1028, 64, 2, 2, 2, None, None, None, None, None, None, 0, None, 0, None,
                                           None, None), lib, word)
    refused(lib.rsaf_cnnlstm_train_forward_group((_lib.TrainItem * 1)(), 1, 16, 1028, 64, 2, 2, 2, None), lib, word)
    refused(lib.rsaf_cnnlstm_adam_group((_lib.AdamItem * 1)(), 1, 16, 1028, 64, 2, 2, None), lib, word)
    assert lib.rsaf_cnnlstm_train_param_offsets(16, 1024, 64, 2, 2, buf, 48, C.byref(n)) == 0    # the last width inside
    refused(lib.rsaf_ce_loss_group((_lib.CeLossItem * 1)(), 1, 1, None), lib, "num_classes")
    refused(lib.rsaf_bn_running_stats_group((_lib.BnRunningItem * 1)(), 1, 1028, None), lib, "channels")


def test_the_table_holds_what_it_promises():
    """The properties the table is there for, stated on its numbers: a later edit cannot drop a branch unnoticed."""
    cases = geo.CASES
    f16 = lambda c: c[0] % 16 == 0 and c[1] % 16 == 0                                    # noqa: E731  use_f16x3
    assert {(c[0] % 16 == 0, c[1] % 16 == 0) for c in cases} == {(True, True), (True, False), (False, True), (False, False)}
    n_f16 = sorted({c[1] for c in cases if f16(c)})
    assert any(n < 64 for n in n_f16) and any(64 < n < 128 for n in n_f16) and any(n > 128 and n % 256 == 16 for n in n_f16)
    assert any(f16(c) and c[0] % 64 == 0 and c[0] == c[1] for c in cases)                # panel image + identity shortcut
    assert any(f16(c) and c[0] == 64 and c[0] != c[1] for c in cases)
    assert any(c[0] == c[1] and not f16(c) for c in cases)
    assert any(c[1] % 8 for c in cases) and any(c[1] % 32 for c in cases) and any(c[1] > 256 and c[1] % 256 for c in cases)
    assert any(c[1] > 8 * c[2] for c in cases) and any(2 * c[2] < c[1] <= 8 * c[2] for c in cases)
    assert {c[5] for c in cases} == {1, 2, 3, 4} and {c[2] for c in cases} == {64, 128}
    assert {1, 16} <= {c[4] for c in cases} | {geo.geometry(geo.NC1)[4]}
    assert any(c[6] > 16 for c in cases) and any(c[7] % 2 for c in cases) and any(c[7] // 2 == 2 for c in cases)
    assert all(c[6] * c[7] <= 17 * 13 for c in cases)
