"""Fused CNN-LSTM training step on the MI355X: rsaf_ce_loss_group, rsaf_cnnlstm_adam_group, rsaf_cnnlstm_pack_params_group
and rsaf_bn_running_stats_group through FusedAdam / cnnlstm_train_step_group / the lockstep loops.

Bars.  Cross-entropy against float64 numpy: 4 * 2^-23 * max(1, max|logit|) for the loss (a difference of two numbers of
that size, each a few ulp off) and 4 * 2^-23 / B for the gradient of the logits.  Adam on prescribed gradients: the
deviation from the float64 oracle may be twice torch.optim.Adam's own largest deviation on the same tensor plus one ulp
of the parameter; the bar is computed in the test from the behaviour being replaced.  The whole step against the
oracle's loop: the bars of tests/test_cnnlstm_train_gpu.py::test_adam_loop_follows_oracle."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from weights import synth_input  # noqa: E402
from cnnlstm_support import (  # noqa: E402
    GEOMETRIES, RAGGED, ULP, ZERO_GRAD, adam_bar, bits, build,
    device_masks, freeze_zero_grad, gradient_blob, launches, lockstep_setup, same, unpacked)

from oracle import cnnlstm_train_oracle as to

pytestmark = pytest.mark.gpu

P_BLOCK, P_RATE = 0.2, 0.5


# ---- 1. cross-entropy kernel -------------------------------------------------------------------------------------------
def ce_reference(x, y):
    x = x.astype(np.float64)
    mx = x.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
    loss = (lse - x[np.arange(len(y)), y]).mean()
    sm = np.exp(x - lse[:, None])
    sm[np.arange(len(y)), y] -= 1.0
    return loss, sm / len(y)


@pytest.mark.parametrize("nc", [2, 3])
def test_cross_entropy_kernel_against_float64(nc):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import ce_loss_group
    rng = np.random.Generator(np.random.PCG64(100 + nc))
    items = []
    for B, scale in ((1, 1.0), (4, 30.0), (7, 80.0)):                       # K = 3 items of different batch
        x = (rng.uniform(-1, 1, (B, nc)) * scale).astype(np.float32)
        if B == 7:
            x[0, 0], x[0, -1] = 80.0, -80.0                                 # the extremes in one row
            x[3, :] = 12.5                                                  # a row of equal logits
        items.append((x, rng.integers(0, nc, B)))
    logits = [torch.from_numpy(x).cuda() for x, _ in items]
    labels = [torch.from_numpy(y).cuda() for _, y in items]
    losses, dl = ce_loss_group(logits, labels)
    losses_only, none = ce_loss_group(logits, labels, with_grad=False)
    torch.cuda.synchronize()
    assert none is None
    same(bits(losses_only), bits(losses), "loss without dlogits")
    for k, (x, y) in enumerate(items):
        want_loss, want_dl = ce_reference(x, y)
        err = abs(float(losses[k]) - want_loss)
        derr = np.abs(dl[k].cpu().numpy().astype(np.float64) - want_dl).max()
        print(f"nc={nc} item {k} B={len(y)}: loss err {err:.3e}, dlogits err {derr:.3e}")
        assert err <= 4 * ULP * max(1.0, np.abs(x).max()), (k, err)
        assert derr <= 4 * ULP / len(y), (k, derr)


def test_cross_entropy_group_longer_than_the_chunk():
    """K = train_group_max() + 1 items of batch 1, 2, 3, 1, ...: item k of the second call writes ``losses[k]`` and its
    own ``dlogits``, not those of its position in the call.  Bars of test_cross_entropy_kernel_against_float64."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import ce_loss_group, train_group_max
    nc, K = 2, train_group_max() + 1
    rng = np.random.Generator(np.random.PCG64(120))
    items = []
    for k in range(K):
        B = 1 + k % 3
        items.append(((rng.uniform(-1, 1, (B, nc)) * (1.0 + 3.0 * k)).astype(np.float32), rng.integers(0, nc, B)))
    logits = [torch.from_numpy(x).cuda() for x, _ in items]
    labels = [torch.from_numpy(y).cuda() for _, y in items]
    losses, dl = ce_loss_group(logits, labels)
    losses_only, none = ce_loss_group(logits, labels, with_grad=False)
    last_loss, last_dl = ce_loss_group(logits[K - 1:], labels[K - 1:])
    torch.cuda.synchronize()
    assert losses.shape == (K,) and len(dl) == K and none is None
    same(bits(losses_only), bits(losses), "loss without dlogits")
    same(bits(losses[K - 1:]), bits(last_loss), f"loss of item {K - 1} against a call of its own")
    same(bits(dl[K - 1]), bits(last_dl[0]), f"dlogits of item {K - 1} against a call of its own")
    for k, (x, y) in enumerate(items):
        want_loss, want_dl = ce_reference(x, y)
        err = abs(float(losses[k]) - want_loss)
        derr = np.abs(dl[k].cpu().numpy().astype(np.float64) - want_dl).max()
        print(f"item {k} B={len(y)}: loss err {err:.3e}, dlogits err {derr:.3e}")
        assert err <= 4 * ULP * max(1.0, np.abs(x).max()), (k, err)
        assert derr <= 4 * ULP / len(y), (k, derr)


# ---- 2. / 3. Adam kernel on prescribed gradients --------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_adam_kernel_on_prescribed_gradients(geom):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, _pack_train_blob, train_param_offsets
    D, C, H, act, NC, L = GEOMETRIES[geom]
    lr = 1e-3
    m, sd = build(D, C, H, 801, act, num_classes=NC, layers=L)
    ref = copy.deepcopy(m)
    opt, topt = FusedAdam(m, lr=lr), torch.optim.Adam(ref.parameters(), lr=lr)
    total = train_param_offsets(m.dims)[1]
    rng = np.random.Generator(np.random.PCG64(802))
    zero = rng.random(total) < 0.1                              # the same elements see a zero gradient at every step
    before = {k: bits(p) for k, p in m.named_parameters()}
    oracle = {k: np.asarray(v, np.float64) for k, v in sd.items() if k in before}
    state = {}
    for it in range(5):
        gb = torch.from_numpy(gradient_blob(rng, total, zero)).cuda()
        opt.step_blob(gb)
        grads = unpacked(ref, gb)
        for k, p in ref.named_parameters():
            p.grad = grads[k].clone()
        topt.step()
        to.adam_step(oracle, {k: g.cpu().numpy().astype(np.float64) for k, g in grads.items()}, state, lr)
        torch.cuda.synchronize()
        same(bits(opt.packed_blob()), bits(_pack_train_blob(m, "cuda")[1]), f"{geom} step {it}: packed blob")
        rp = dict(ref.named_parameters())
        for k, p in m.named_parameters():
            adam_bar(p.detach().cpu().numpy(), rp[k].detach().cpu().numpy(), oracle[k], f"{geom} step {it} {k}")
        assert all(int(opt.state[p]["step"]) == it + 1 for p in m.parameters())
    # zero gradient from a zero state: the bits of the parameter stay
    zg = unpacked(m, torch.from_numpy(zero.astype(np.float32)).cuda())
    n_zero = 0
    for k, p in m.named_parameters():
        z = zg[k].cpu().numpy() != 0
        n_zero += int(z.sum())
        same(bits(p)[z], before[k][z], f"{geom} {k}: elements with zero gradients")
        assert (bits(p)[~z] != before[k][~z]).any() or (~z).sum() == 0, k
    assert n_zero > 100
    # both biases of a direction took the same gradient from the same state: identical moments
    assert m.dims["layers"] == L and m.dims["num_classes"] == NC
    for l in range(m.dims["layers"]):
        for sfx in ("", "_reverse"):
            a, b = getattr(m.lstm, f"bias_ih_l{l}{sfx}"), getattr(m.lstm, f"bias_hh_l{l}{sfx}")
            same(bits(opt.state[a]["exp_avg"]), bits(opt.state[b]["exp_avg"]), f"exp_avg of the bias pair l{l}{sfx}")
            same(bits(opt.state[a]["exp_avg_sq"]), bits(opt.state[b]["exp_avg_sq"]), f"exp_avg_sq of the bias pair l{l}{sfx}")
            da = a.detach().cpu().numpy().astype(np.float64) - sd[f"lstm.bias_ih_l{l}{sfx}"]
            db = b.detach().cpu().numpy().astype(np.float64) - sd[f"lstm.bias_hh_l{l}{sfx}"]
            # equal updates, each parameter rounded to float32 once per step
            room = 5 * ULP * (np.abs(a.detach().cpu().numpy()) + np.abs(b.detach().cpu().numpy()) + 5 * lr)
            assert (np.abs(da - db) <= room).all(), (l, sfx, np.abs(da - db).max())


def test_frozen_parameters_keep_their_bits():
    """requires_grad_(False) on a conv kernel, on one bias of a pair and on fc.bias: value and moments stay, the partner
    moves, the packed blob follows the module; after thawing, the kernel honours torch's per-parameter step counts
    (bar against torch.optim.Adam fed the same gradients: both round the same real update of at most lr per step to
    float32, a few ulp of the parameter per step on either side plus 1e-5 of the moves made)."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, _pack_train_blob, train_param_offsets
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    lr = 1e-3
    m, _ = build(D, C, H, 811, act)
    ref = copy.deepcopy(m)
    opt, topt = FusedAdam(m, lr=lr), torch.optim.Adam(ref.parameters(), lr=lr)
    total = train_param_offsets(m.dims)[1]
    rng = np.random.Generator(np.random.PCG64(812))
    frozen = ["res_block1.conv1.weight", "lstm.bias_hh_l0", "fc.bias"]
    named = dict(m.named_parameters())

    def one(skip_names):
        gb = torch.from_numpy(gradient_blob(rng, total, np.zeros(total, bool))).cuda()
        opt.step_blob(gb)
        grads = unpacked(ref, gb)
        for k, p in ref.named_parameters():
            p.grad = None if k in skip_names else grads[k].clone()
        topt.step()
        torch.cuda.synchronize()
        same(bits(opt.packed_blob()), bits(_pack_train_blob(m, "cuda")[1]), "packed blob")

    one([])
    for k in frozen:
        named[k].requires_grad_(False)
    keep = {k: (bits(named[k]), bits(opt.state[named[k]]["exp_avg"]), bits(opt.state[named[k]]["exp_avg_sq"])) for k in frozen}
    partner = bits(named["lstm.bias_ih_l0"])
    one(frozen)
    one(frozen)
    for k in frozen:
        same(bits(named[k]), keep[k][0], f"frozen {k}")
        same(bits(opt.state[named[k]]["exp_avg"]), keep[k][1], f"exp_avg of frozen {k}")
        same(bits(opt.state[named[k]]["exp_avg_sq"]), keep[k][2], f"exp_avg_sq of frozen {k}")
        assert int(opt.state[named[k]]["step"]) == 1
    assert (bits(named["lstm.bias_ih_l0"]) != partner).any()
    for k in frozen:
        named[k].requires_grad_(True)
    one([])                                                     # step 2 for the thawed parameters, step 4 for the others
    for k, p in ref.named_parameters():
        assert int(opt.state[named[k]]["step"]) == int(topt.state[p]["step"]) == (2 if k in frozen else 4), k
        a, b = named[k].detach().cpu().numpy().astype(np.float64), p.detach().cpu().numpy().astype(np.float64)
        assert (np.abs(a - b) <= 4 * 4 * ULP * np.abs(b) + 1e-5 * 4 * lr).all(), (k, np.abs(a - b).max())


# ---- 4. the whole step against the oracle's loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_fused_group_step_follows_the_oracle_loop(geom):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, cnnlstm_train_group, cnnlstm_train_step_group
    D, C, H, act, NC, L = GEOMETRIES[geom]
    lr, steps = 1e-3, 3
    models, sds = zip(*[build(D, C, H, 901 + 10 * k, act, P_RATE, P_BLOCK, NC, L) for k in range(len(RAGGED))])
    for m in models:
        freeze_zero_grad(m)
    opts = [FusedAdam(m, lr=lr) for m in models]
    params = [{k: np.asarray(v, np.float64) for k, v in sd.items()} for sd in sds]
    states = [{} for _ in models]
    losses_o, losses_g = [], []
    for it in range(steps):
        xs = [synth_input(B, T, D, 950 + 10 * k + it) for k, (B, T) in enumerate(RAGGED)]
        labels = [np.random.Generator(np.random.PCG64(960 + 10 * k + it)).integers(0, NC, B) for k, (B, _) in enumerate(RAGGED)]
        mks = [to.make_masks(B, T, C, H, P_BLOCK, P_RATE, 970 + 10 * k + it, layers=L) for k, (B, T) in enumerate(RAGGED)]
        row = []
        for k in range(len(RAGGED)):
            r = to.forward_backward(params[k], xs[k], labels[k], act, masks=mks[k])
            g = {key: (np.zeros_like(v) if key.endswith(ZERO_GRAD) else v) for key, v in r["grads"].items()}
            params[k].update(to.adam_step({key: params[k][key] for key in g}, g, states[k], lr))
            params[k].update(to.updated_bn_buffers(params[k], r["bn_stats"]))
            row.append(r["loss"])
        losses_o.append(row)
        dx = [torch.from_numpy(x).cuda() for x in xs]
        dmk = [device_masks(mk) for mk in mks]
        if it == 0:                                             # the same kernels on the same blob: the same logits
            with torch.no_grad():
                want = [o.cpu().numpy() for o in cnnlstm_train_group([copy.deepcopy(m) for m in models], dx, masks=dmk)]
        ls, logits = cnnlstm_train_step_group(models, opts, dx, [torch.from_numpy(y).cuda() for y in labels], masks=dmk)
        assert ls.shape == (len(RAGGED),) and ls.is_cuda and all(p.grad is None for m in models for p in m.parameters())
        if it == 0:
            for k in range(len(RAGGED)):
                same(logits[k].cpu().numpy(), want[k], f"{geom} replica {k}: first-step logits against cnnlstm_train_group")
        losses_g.append(ls.tolist())
    print(f"{geom}: losses fused {losses_g} oracle {losses_o}")
    assert np.allclose(losses_g, losses_o, rtol=2e-4, atol=2e-5), (losses_g, losses_o)
    for k, m in enumerate(models):
        st = m.state_dict()
        for key in sds[k]:
            if key.endswith("num_batches_tracked"):
                assert int(st[key]) == steps
                continue
            a, b = st[key].cpu().numpy().astype(np.float64), params[k][key]
            if key.endswith(("running_mean", "running_var")):
                assert np.abs(a - b).max() < 1e-4 * max(np.abs(b).max(), 1e-3), (k, key, np.abs(a - b).max())
            else:
                assert np.abs(a - b).max() < 0.05 * lr + 1e-4 * np.abs(b).max(), (k, key, np.abs(a - b).max())


def test_group_longer_than_the_chunk():
    """K = train_group_max() + 1: the second chunk computes what a group of its own computes."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, cnnlstm_train_step_group, train_group_max
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    K = train_group_max() + 1
    models = [build(D, C, H, 1001 + (k % 3), act)[0] for k in range(K)]
    twins = [copy.deepcopy(models[0]), copy.deepcopy(models[K - 1])]
    xs = [torch.from_numpy(synth_input(2, 12, D, 1010 + k)).cuda() for k in range(K)]
    ys = [torch.tensor([k % 2, 1 - k % 2]).cuda() for k in range(K)]
    ls, logits = cnnlstm_train_step_group(models, [FusedAdam(m) for m in models], xs, ys)
    ls2, logits2 = cnnlstm_train_step_group(twins, [FusedAdam(m) for m in twins], [xs[0], xs[K - 1]], [ys[0], ys[K - 1]])
    assert ls.shape == (K,) and len(logits) == K
    for a, b in ((0, 0), (K - 1, 1)):
        same(logits[a].cpu().numpy(), logits2[b].cpu().numpy(), f"replica {a} logits")
        same(bits(ls[a]), bits(ls2[b]), f"replica {a} loss")
        for (k, p), q in zip(models[a].named_parameters(), twins[b].parameters()):
            same(bits(p), bits(q), f"replica {a} {k}")


# ---- 5. staleness -------------------------------------------------------------------------------------------------------------
def fused_steps(m, opt, n, seed, D):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_step_group
    logits = None
    for it in range(n):
        x = torch.from_numpy(synth_input(4, 24, D, seed + it)).cuda()
        y = torch.tensor([0, 1, 1, 0]).cuda()
        logits = cnnlstm_train_step_group([m], [opt], [x], [y])[1][0]
    return logits.cpu().numpy()


def test_eval_after_fused_steps_sees_the_new_weights():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, FusedAdam
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    m, _ = build(D, C, H, 1101, act)
    x = torch.from_numpy(synth_input(3, 20, D, 1102)).cuda()
    m.eval()
    before = m(x).cpu().numpy()                                   # fills the eval blob cache
    m.train()
    fused_steps(m, FusedAdam(m), 2, 1110, D)
    got = m.eval()(x).cpu().numpy()
    fresh = CNNLSTM(input_dim=D, cnn_out_channels=C, lstm_hidden_dim=H, activation_fn=act).cuda().eval()
    fresh.load_state_dict(m.state_dict())
    same(got, fresh(x).cpu().numpy(), "eval logits after two fused steps")
    assert np.abs(got - before).max() > 1e-5


@pytest.mark.parametrize("edit", ["load_state_dict", "data_mul"])
def test_fused_step_after_somebody_else_wrote_the_parameters(edit):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, FusedAdam
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    m, _ = build(D, C, H, 1201, act)
    opt = FusedAdam(m)
    fused_steps(m, opt, 2, 1210, D)
    if edit == "load_state_dict":
        m.load_state_dict(build(D, C, H, 1202, act)[0].state_dict())
    else:
        for p in m.parameters():
            p.data.mul_(2)
    fresh = CNNLSTM(input_dim=D, cnn_out_channels=C, lstm_hidden_dim=H, activation_fn=act).cuda().train()
    fresh.load_state_dict(m.state_dict())
    fresh.res_block1.dropout.p = fresh.res_block2.dropout.p = 0.0
    fresh.dropout.p = fresh.lstm.dropout = 0.0
    got = fused_steps(m, opt, 1, 1220, D)
    same(got, fused_steps(fresh, FusedAdam(fresh), 1, 1220, D), f"logits of the step after {edit}")


# ---- 6. optimizer interchange and schedulers ----------------------------------------------------------------------------------
def test_state_dict_interchange_with_torch_adam():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_param_offsets
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    lr = 1e-3
    total = train_param_offsets(build(D, C, H, 1301, act)[0].dims)[1]
    rng = np.random.Generator(np.random.PCG64(1302))
    blobs = [torch.from_numpy(gradient_blob(rng, total, np.zeros(total, bool))).cuda() for _ in range(3)]

    def torch_steps(model, topt, gbs):
        for gb in gbs:
            grads = unpacked(model, gb)
            for k, p in model.named_parameters():
                p.grad = grads[k].clone()
            topt.step()

    def oracle_after(sd, model):
        prm = {k: np.asarray(sd[k], np.float64) for k, _ in model.named_parameters()}
        st = {}
        for gb in blobs:
            to.adam_step(prm, {k: g.cpu().numpy().astype(np.float64) for k, g in unpacked(model, gb).items()}, st, lr)
        return prm

    for direction in ("fused_to_torch", "torch_to_fused"):
        (a, sd), (b, _), (ref, _) = build(D, C, H, 1301, act), build(D, C, H, 1301, act), build(D, C, H, 1301, act)
        fa, tb, tref = FusedAdam(a, lr=lr), torch.optim.Adam(b.parameters(), lr=lr), torch.optim.Adam(ref.parameters(), lr=lr)
        torch_steps(ref, tref, blobs)                             # torch alone, all three steps
        if direction == "fused_to_torch":
            for gb in blobs[:2]:
                fa.step_blob(gb)
            b.load_state_dict(a.state_dict())
            tb.load_state_dict(fa.state_dict())
            torch_steps(b, tb, blobs[2:])
            got = b
        else:
            torch_steps(b, tb, blobs[:2])
            a.load_state_dict(b.state_dict())
            fa.load_state_dict(tb.state_dict())
            fa.step_blob(blobs[2])
            got = a
        torch.cuda.synchronize()
        want = oracle_after(sd, ref)
        rp = dict(ref.named_parameters())
        for k, p in got.named_parameters():
            adam_bar(p.detach().cpu().numpy(), rp[k].detach().cpu().numpy(), want[k], f"{direction} {k}")
        assert sorted(fa.state_dict()["param_groups"][0]) == sorted(tb.state_dict()["param_groups"][0])
        assert all(sorted(v) == ["exp_avg", "exp_avg_sq", "step"] for v in fa.state_dict()["state"].values())


def test_reduce_lr_on_plateau_drives_the_fused_step():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_param_offsets
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    total = train_param_offsets(build(D, C, H, 1401, act)[0].dims)[1]
    gb = torch.full((total,), 0.25, device="cuda")
    moves = []
    for lr_steps in (0, 1):                                       # fresh state both times: the first update is lr * sign(g)
        m, _ = build(D, C, H, 1401, act)
        opt = FusedAdam(m, lr=1e-2)
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.1, patience=0)
        for _ in range(2 * lr_steps):
            sched.step(1.0)                                       # the second equal metric is a non-improving one
        before = m.fc.weight.detach().clone()
        opt.step_blob(gb)
        moves.append((m.fc.weight.detach() - before).abs().max().item())
    print("update sizes", moves)
    assert abs(moves[0] - 1e-2) < 1e-6 and abs(moves[1] - 1e-3) < 1e-7, moves


# ---- 7. / 8. the lockstep loops -----------------------------------------------------------------------------------------------
def test_lockstep_takes_the_fused_step_and_agrees_with_torch_adam():
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_replicas_lockstep
    lr, epochs = 1e-3, 2
    models, opts, loaders = lockstep_setup(1500, lambda k, m: FusedAdam(m, lr=lr))
    assert [len(ld) for ld in loaders] == [5, 3, 4]
    _lib.prof_begin()
    hist = train_replicas_lockstep(models, opts, loaders, torch.nn.CrossEntropyLoss(), epochs, "cuda")
    prof = _lib.prof_end()
    group_steps = epochs * max(len(ld) for ld in loaders)
    for family in ("train_adam", "train_ce", "train_pack", "train_bn_running"):
        assert launches(prof, family) == group_steps, (family, prof.get(family))
    models_t, opts_t, loaders_t = lockstep_setup(1500, lambda k, m: torch.optim.Adam(m.parameters(), lr=lr))
    _lib.prof_begin()
    want = train_replicas_lockstep(models_t, opts_t, loaders_t, torch.nn.CrossEntropyLoss(), epochs, "cuda")
    assert launches(_lib.prof_end(), "train_adam") == 0
    print("lockstep histories fused", hist, "torch", want)
    assert np.allclose(hist, want, rtol=2e-4, atol=2e-5), (hist, want)


@pytest.mark.parametrize("case", ["label_smoothing", "one_torch_optimizer"])
def test_lockstep_keeps_the_autograd_loop_for_anything_else(case):
    """Another loss, or one torch optimizer among the K: no launch of the group step; every FusedAdam steps on its own
    (one launch per model and step).  The replica that holds a torch.optim.Adam ends where it ends in a run with three of
    them, bit for bit (the replicas share nothing); the others follow that run under the loss bar."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_replicas_lockstep
    lr, epochs = 1e-3, 1
    loss_fn = torch.nn.CrossEntropyLoss(label_smoothing=0.1) if case == "label_smoothing" else torch.nn.CrossEntropyLoss()
    fused = (lambda k: True) if case == "label_smoothing" else (lambda k: k != 1)
    mk = lambda k, m: FusedAdam(m, lr=lr) if fused(k) else torch.optim.Adam(m.parameters(), lr=lr)     # noqa: E731
    models, opts, loaders = lockstep_setup(1600, mk)
    _lib.prof_begin()
    hist = train_replicas_lockstep(models, opts, loaders, loss_fn, epochs, "cuda")
    prof = _lib.prof_end()
    assert launches(prof, "train_ce") == 0 and launches(prof, "train_pack") == 0 and launches(prof, "train_bn_running") == 0
    assert launches(prof, "train_adam") == sum(len(ld) for k, ld in enumerate(loaders) if fused(k))
    models_t, opts_t, loaders_t = lockstep_setup(1600, lambda k, m: torch.optim.Adam(m.parameters(), lr=lr))
    want = train_replicas_lockstep(models_t, opts_t, loaders_t, loss_fn, epochs, "cuda")
    print(case, "histories", hist, "torch", want)
    assert np.allclose(hist, want, rtol=2e-4, atol=2e-5), (hist, want)
    for k in range(3):
        if fused(k):
            continue
        assert hist[k] == want[k], (k, hist[k], want[k])
        for (name, p), q in zip(models[k].state_dict().items(), models_t[k].state_dict().values()):
            same(p.cpu().numpy(), q.cpu().numpy(), f"replica {k} {name}")


def test_reference_loop_with_only_the_optimizer_swapped():
    """zero_grad / model(x) / loss / backward / FusedAdam.step() on ordinary .grad tensors against the same loop with
    torch.optim.Adam, under the bar of the prescribed-gradient test (float64 oracle fed torch's gradients); a parameter
    without a gradient is skipped."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam
    D, C, H, act = GEOMETRIES["identity_shortcut_gelu"][:4]
    lr = 1e-3
    (a, sd), (b, _) = build(D, C, H, 1701, act), build(D, C, H, 1701, act)
    fa, tb = FusedAdam(a, lr=lr), torch.optim.Adam(b.parameters(), lr=lr)
    x = torch.from_numpy(synth_input(4, 24, D, 1702)).cuda()
    y = torch.tensor([0, 1, 1, 0]).cuda()
    outs = []
    for m, opt in ((a, fa), (b, tb)):
        opt.zero_grad()
        out = m(x)
        torch.nn.CrossEntropyLoss()(out, y).backward()
        m.fc.bias.grad = None
        outs.append(out.detach().cpu().numpy())
    same(outs[0], outs[1], "logits")
    grads = {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in b.named_parameters() if p.grad is not None}
    fa.step()
    tb.step()
    torch.cuda.synchronize()
    oracle = to.adam_step({k: np.asarray(sd[k], np.float64) for k in grads}, grads, {}, lr)
    pb = dict(b.named_parameters())
    for k, p in a.named_parameters():
        if k == "fc.bias":
            same(bits(p), bits(pb[k]), "fc.bias without a gradient")
            assert "exp_avg" not in fa.state[p]
            continue
        adam_bar(p.detach().cpu().numpy(), pb[k].detach().cpu().numpy(), oracle[k], k)
    fa.zero_grad()
    assert all(p.grad is None for p in a.parameters())


def test_train_eval_lockstep_with_fused_adam_and_schedulers():
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_eval_replicas_lockstep
    epochs, patience = 3, 1
    models, opts, loaders = lockstep_setup(1800, lambda k, m: FusedAdam(m, lr=1e-3), p=0.2)
    _, _, val_loaders = lockstep_setup(1850, lambda k, m: None, shuffle=False)
    scheds = [torch.optim.lr_scheduler.ReduceLROnPlateau(o, factor=0.5, patience=0) for o in opts]
    _lib.prof_begin()
    res = train_eval_replicas_lockstep(models, opts, scheds, loaders, val_loaders, torch.nn.CrossEntropyLoss(), epochs, patience, "cuda")
    prof = _lib.prof_end()
    assert launches(prof, "train_adam") > 0 and launches(prof, "train_ce") > launches(prof, "train_adam")     # + the validation passes
    assert len(res) == 3
    for k, (m, th, vh) in enumerate(res):
        assert m is models[k] and len(th) == len(vh) and 1 <= len(vh) <= epochs
        assert np.isfinite(th).all() and np.isfinite(vh).all()
        stopped = len(vh) < epochs
        assert not stopped or vh[-1] >= min(vh[:-1])
        # the model holds its best weights: its validation loss is the best of the history
        m.eval()
        tot, n, big = 0.0, 0, 1.0
        with torch.no_grad():
            for seq, lab in val_loaders[k]:
                out = m(seq.cuda())
                tot += torch.nn.CrossEntropyLoss()(out, lab.cuda()).item()
                big = max(big, out.abs().max().item())
                n += 1
        # torch's float32 loss here, the kernel's in the history: the cross-entropy bar once for either side
        assert abs(tot / n - min(vh)) <= 2 * 4 * ULP * big, (k, tot / n, vh)
