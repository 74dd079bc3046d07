"""Host side of the fused CNN-LSTM training step (no GPU): what FusedAdam refuses, and the parameter numbering that
rsaf_cnnlstm_adam_group / rsaf_cnnlstm_pack_params_group share with the Python side."""
import pytest
import torch

from robust_speech_analysis_framework_amd import cnnlstm
from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, FusedAdam, cnnlstm_train_step_group  # noqa: F401


def small(**kw):
    return CNNLSTM(**dict(dict(input_dim=16, cnn_out_channels=32, lstm_hidden_dim=64), **kw))


@pytest.mark.parametrize("kw, word", [({"weight_decay": 0.01}, "weight_decay"), ({"amsgrad": True}, "amsgrad"),
                                      ({"maximize": True}, "maximize")])
def test_unsupported_adam_options_are_refused_by_name(rsaf_lib, kw, word):
    with pytest.raises(ValueError, match=word):
        FusedAdam(small(), **kw)


def test_other_modules_and_cpu_models_are_refused(rsaf_lib):
    with pytest.raises(ValueError, match="CNNLSTM"):
        FusedAdam(torch.nn.Linear(4, 2))
    with pytest.raises(ValueError, match="CNNLSTM"):
        FusedAdam(small().parameters())
    with pytest.raises(ValueError, match="HIP device"):
        FusedAdam(small())
    for bad in ({"lr": -1.0}, {"eps": -1e-8}, {"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)}):
        with pytest.raises(ValueError):
            FusedAdam(small(), **bad)


@pytest.mark.parametrize("dims", [dict(input_dim=16, cnn_out_channels=32), dict(input_dim=32, cnn_out_channels=32),
                                  dict(input_dim=16, cnn_out_channels=32, lstm_layers=1),
                                  dict(input_dim=768, cnn_out_channels=128, lstm_hidden_dim=128, lstm_layers=3, num_classes=3)])
def test_kernel_numbering_covers_every_parameter_once(rsaf_lib, dims):
    """The kernels number the parameters in blob order; the Python side hands them their pointers in that order.  The
    order is a bijection onto model.parameters(), and the segments that carry two parameters for one run of the blob
    are exactly the bias pairs (both directions of every layer) and the two directions of weight_ih / weight_hh."""
    m = small(**dims)
    d = m.dims
    n = rsaf_lib.rsaf_cnnlstm_adam_param_count(d["input_dim"], d["channels"], d["hidden"], d["num_classes"], d["layers"])
    order = cnnlstm._adam_order(m)
    assert n == len(order) == len(list(m.parameters()))
    assert sorted(id(p) for p in order) == sorted(id(p) for p in m.parameters())
    names = {id(p): k for k, p in m.named_parameters()}
    segs, total = cnnlstm._train_segments(m)
    shared = [[names[id(p)] for p, _ in outs] for _, _, _, outs in segs if len(outs) > 1]
    assert len(shared) == 3 * d["layers"]
    assert sum(len(s) == 4 and all("bias" in k for k in s) for s in shared) == d["layers"]
    # the segments tile the blob without overlap, each as large as what it packs (the pair of a bias segment: one image)
    end = 0
    for off, nfl, pack, outs in segs:
        assert off >= end and off % 4 == 0 and pack().numel() == nfl
        end = off + nfl
    assert end <= total
    assert rsaf_lib.rsaf_cnnlstm_adam_param_count(16, 32, 65, 2, 2) == -1          # unsupported hidden size


def test_group_calls_check_their_arguments_before_any_launch(rsaf_lib):
    import ctypes as C
    from robust_speech_analysis_framework_amd import _lib
    items = (_lib.AdamItem * 1)()
    assert rsaf_lib.rsaf_cnnlstm_adam_group(items, 0, 16, 32, 64, 2, 2, None) != 0
    assert rsaf_lib.rsaf_cnnlstm_adam_group(items, 17, 16, 32, 64, 2, 2, None) != 0
    assert rsaf_lib.rsaf_cnnlstm_adam_group(items, 1, 16, 32, 64, 2, 2, None) != 0      # NULL table
    assert b"NULL" in rsaf_lib.rsaf_last_error()
    assert rsaf_lib.rsaf_ce_loss_group((_lib.CeLossItem * 1)(), 1, 1, None) != 0        # one class
    assert rsaf_lib.rsaf_cnnlstm_pack_params_group((_lib.PackItem * 1)(), 1, 16, 32, 64, 2, 2, None) != 0
    assert rsaf_lib.rsaf_bn_running_stats_group((_lib.BnRunningItem * 1)(), 1, 32, None) != 0
    assert C.sizeof(_lib.AdamItem) == 64 and C.sizeof(_lib.BnRunningItem) == 168 and C.sizeof(_lib.CeLossItem) == 40
