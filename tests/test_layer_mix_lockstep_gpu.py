"""The learned layer mix in the training paths on the MI355X: ``collate_mix_batches`` in front of ``cnnlstm_train_group``, the
fused ``cnnlstm_mix_train_step_group``, and the three lock-step loops with ``mixes=``.

One ragged step (tests/collate_mix_cases.py: three layers in front of geometry row 2) is held to the float64 restatement of
``input_grad_restatement.forward_backward`` at the float64 mix of the zero-padded stack, under ``cnnlstm_support.RTOL`` and
``check_grads`` as tests/test_layer_mix_gpu.py holds the dense path.  Everything else is bit equality: the resident path
against ``LayerMix`` on the loader's padded stack, lock step against sequential runs, one group launch against K."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cnnlstm_geometry as geo  # noqa: E402
import collate_mix_cases as cmc  # noqa: E402
import input_grad_cases as igc  # noqa: E402
from cnnlstm_support import (GEOMETRIES, RTOL, bits, build, check_grads, device_masks, freeze_zero_grad, launches,  # noqa: E402
                             same)

pytestmark = pytest.mark.gpu

L = 3


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def step_setup():
    """(model with the case's masks, mix at the case's weights, plan of the one batch, h_padded, labels) of the ragged step."""
    import torch
    from src.models import LayerMix
    from robust_speech_analysis_framework_amd.cnnlstm import DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore
    e = cmc.step_case()
    store = DeviceSequenceStore(e["seqs"], layers=cmc.STEP_L)
    loader = DeviceBatchLoader(DeviceSequenceDataset(store, e["labels"]), batch_size=len(e["seqs"]))
    (h, lab), = list(loader)
    same(bits(h), e["h"].view(np.uint32), "the loader's padded stack")
    m = geo.model_of(cmc.STEP_ROW, e["sd"], train=True)
    m.forced_masks = device_masks(e["masks"])
    mix = LayerMix(cmc.STEP_L).cuda()
    with torch.no_grad():
        mix.weights.copy_(dev(np.asarray(cmc.STEP_WEIGHTS, np.float32)))
    return e, m, mix, next(loader.plans()), h, lab


def test_one_ragged_step_against_the_float64_restatement(rsaf_lib):
    import torch
    from src.models import cnnlstm_train_group, collate_mix_batches
    e, m, mix, plan, h, lab = step_setup()
    want = e["want"]
    assert len(set(e["lengths"])) > 1 and max(e["lengths"]) == geo.CASES[cmc.STEP_ROW][7]
    gap = geo.pool_gap(want["stages"]["res1"])
    assert gap >= igc.POOL_GAP, gap
    (x, labels), = collate_mix_batches([plan], [mix])
    out, = cnnlstm_train_group([m], [x])
    loss = torch.nn.CrossEntropyLoss()(out, labels)
    loss.backward()
    torch.cuda.synchronize()
    dw = mix.weights.grad.cpu().numpy().astype(np.float64)
    err = np.abs(dw - e["dw64"]).max() / np.abs(e["dw64"]).max()
    worst = check_grads({k: v.grad.detach().cpu().numpy() for k, v in m.named_parameters()}, want["grads"])
    print(f"ragged mix step: dL/dw {err:.2e} of max|dw64| = {np.abs(e['dw64']).max():.2e}, worst gradient {worst[1]:.2e} ({worst[0]}), "
          f"loss {abs(loss.item() - want['loss']):.2e}, pool gap {gap:.2e}")
    assert err < RTOL, err
    assert abs(loss.item() - want["loss"]) < RTOL
    # the same step through LayerMix on the padded stack: the same bits everywhere
    _, m2, mix2, _, _, _ = step_setup()
    out2, = cnnlstm_train_group([m2], [mix2(h)])
    loss2 = torch.nn.CrossEntropyLoss()(out2, lab)
    loss2.backward()
    same(bits(out), bits(out2), "logits")
    same(bits(loss), bits(loss2), "loss")
    same(bits(mix.weights.grad), bits(mix2.weights.grad), "weights.grad")
    for (k, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        same(bits(a.grad), bits(b.grad), k + ".grad")
    for (k, a), (_, b) in zip(m.named_buffers(), m2.named_buffers()):
        assert torch.equal(a, b), k


def test_fused_mix_step_against_the_float64_restatement(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from src.models import FusedAdam, cnnlstm_mix_train_step_group
    e, m, mix, plan, h, lab = step_setup()
    want = e["want"]
    opt = FusedAdam(m, lr=1e-3, layer_mix=mix, layer_mix_lr=1e-2)
    w0 = mix.weights.detach().clone()
    _lib.prof_begin()
    losses, logits = cnnlstm_mix_train_step_group([m], [mix], [opt], [plan])
    prof = _lib.prof_end()
    torch.cuda.synchronize()
    assert losses.shape == (1,) and abs(losses[0].item() - want["loss"]) < RTOL
    lerr = np.abs(logits[0].cpu().numpy() - want["logits"]).max() / np.abs(want["logits"]).max()
    dp = opt.last_mix_dp.cpu().numpy().astype(np.float64)
    derr = np.abs(dp - e["dp64"]).max() / np.abs(e["dp64"]).max()
    print(f"fused mix step: logits {lerr:.2e}, dL/dp {derr:.2e} of max|dp64| = {np.abs(e['dp64']).max():.2e}")
    assert lerr < RTOL and derr < RTOL, (lerr, derr)
    # launch census of the step: p costs one softmax-only launch here (the weights were set from outside), then the step's own
    assert launches(prof, "train_collate_mix") == 1 and launches(prof, "train_collate_mix_backward") == 2
    assert launches(prof, "layer_mix_adam") == 2 and launches(prof, "layer_mix_forward") == 0 == launches(prof, "layer_mix_backward")
    # Adam's first step moves every weight by lr * g / (|g| + eps): lr against the sign of dw where |dw| >> eps = 1e-8, which
    # holds for this case (asserted), so that the RTOL of dw does not show in the update
    assert np.abs(e["dw64"]).min() > 1e-5, e["dw64"]
    moved = (mix.weights.detach() - w0).cpu().numpy()
    assert (np.abs(np.abs(moved) - 1e-2) < 1e-4).all() and (np.sign(moved) == -np.sign(e["dw64"])).all(), (moved, e["dw64"])
    assert int(opt.state[mix.weights]["step"]) == 1 and mix.weights.grad is None


# ---- the lock-step loops ---------------------------------------------------------------------------------------------------
def layered_setup(seed, p=0.2, shuffle=True, with_opt=True):
    """Three replicas as ``cnnlstm_support.lockstep_setup`` sizes them (19, 12 and 14 sequences in batches of 4: 5, 3 and 4
    ragged batches), every sequence a stack of L layers in a store of its own, every model with a ``DropoutStream``."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import (DeviceBatchLoader, DeviceSequenceDataset, DeviceSequenceStore, DropoutStream,
                                                               FusedAdam)
    from src.models import LayerMix
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    models, mixes, opts, loaders = [], [], [], []
    for k, n_seq in enumerate((19, 12, 14)):
        m, _ = build(D, C, H, seed + k, act, p_rate=p, p_block=p)
        freeze_zero_grad(m)
        m.dropout_stream = DropoutStream(seed + 300 + k)
        rng = np.random.Generator(np.random.PCG64(seed + 100 + k))
        seqs = [rng.standard_normal((L, int(rng.integers(10, 31)), D)).astype(np.float32) for _ in range(n_seq)]
        labels = rng.integers(0, 2, n_seq)
        mix = LayerMix(L).cuda()
        with torch.no_grad():
            mix.weights.copy_(dev(rng.uniform(-0.5, 0.5, L).astype(np.float32)))
        store = DeviceSequenceStore(seqs, layers=L)
        loaders.append(DeviceBatchLoader(DeviceSequenceDataset(store, labels), batch_size=4, shuffle=shuffle,
                                         generator=torch.Generator().manual_seed(seed + k) if shuffle else None))
        models.append(m)
        mixes.append(mix)
        opts.append(FusedAdam(m, lr=2e-3, layer_mix=mix, layer_mix_lr=2e-2) if with_opt else None)
    return models, mixes, opts, loaders


def state_of(models, mixes, opts):
    out = []
    for m, mix, opt in zip(models, mixes, opts):
        st = {"param." + k: v for k, v in m.named_parameters()}
        st.update({"buffer." + k: v for k, v in m.named_buffers()})
        st["mix.weights"] = mix.weights
        if opt is not None:
            names = {id(p): k for k, p in list(m.named_parameters()) + [("mix.weights", mix.weights)]}
            for p, s in opt.state.items():
                for key in ("step", "exp_avg", "exp_avg_sq"):
                    st[f"adam.{names[id(p)]}.{key}"] = s[key]
        out.append({k: v.detach().cpu().numpy().copy() for k, v in st.items()})
    return out


def same_state(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), (what, k)
        for name in w:
            assert g[name].dtype == w[name].dtype and g[name].tobytes() == w[name].tobytes(), f"{what}: replica {k}: {name} differs"


def test_lock_step_equals_sequential_runs(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from src.models import train_replicas_lockstep
    seed, epochs = 29200, 2
    loss_fn = torch.nn.CrossEntropyLoss()
    models, mixes, opts, loaders = layered_setup(seed)
    before = state_of(models, mixes, [None] * 3)
    _lib.prof_begin()
    got = train_replicas_lockstep(models, opts, loaders, loss_fn, epochs, "cuda", mixes=mixes)
    prof = _lib.prof_end()
    steps = epochs * 5
    # per group step: one collate-mix launch, two launches of its backward, one step of the mix weights; the first step adds
    # one softmax-only launch (the weights were set from outside)
    assert launches(prof, "train_collate_mix") == steps and launches(prof, "train_collate_mix_backward") == 2 * steps
    assert launches(prof, "layer_mix_adam") == steps + 1 and launches(prof, "train_collate") == 0
    assert launches(prof, "layer_mix_forward") == 0 == launches(prof, "layer_mix_backward")
    state = state_of(models, mixes, opts)
    for k in range(3):
        assert state[k]["mix.weights"].tobytes() != before[k]["mix.weights"].tobytes(), k
        assert int(state[k]["adam.mix.weights.step"]) == epochs * len(loaders[k])
    models, mixes, opts, loaders = layered_setup(seed)
    want, census = [], []
    for k in range(3):
        _lib.prof_begin()
        want += train_replicas_lockstep([models[k]], [opts[k]], [loaders[k]], loss_fn, epochs, "cuda", mixes=[mixes[k]])
        census.append(_lib.prof_end())
    assert got == want, (got, want)
    same_state(state, state_of(models, mixes, opts), "K = 3 in lock step against three K = 1 runs")
    # the same number of launches per group step at K = 1
    for k, prof in enumerate(census):
        n = epochs * len(loaders[k])
        assert (launches(prof, "train_collate_mix"), launches(prof, "train_collate_mix_backward"), launches(prof, "layer_mix_adam")) \
            == (n, 2 * n, n + 1), k


def test_autograd_loop_when_the_optimizer_does_not_own_the_mix(rsaf_lib):
    """torch.optim.Adam over both parameter sets: the loop runs over ``collate_mix_batches`` and learns the mix too; K = 3
    equals three K = 1 runs."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from src.models import train_replicas_lockstep
    seed = 29250
    loss_fn = torch.nn.CrossEntropyLoss()

    def setup():
        models, mixes, _, loaders = layered_setup(seed, with_opt=False)
        return models, mixes, [torch.optim.Adam(list(m.parameters()) + [x.weights], lr=2e-3) for m, x in zip(models, mixes)], loaders

    models, mixes, opts, loaders = setup()
    before = state_of(models, mixes, [None] * 3)
    _lib.prof_begin()
    got = train_replicas_lockstep(models, opts, loaders, loss_fn, 1, "cuda", mixes=mixes)
    prof = _lib.prof_end()
    assert launches(prof, "train_collate_mix") == 5 and launches(prof, "train_collate_mix_backward") == 10
    assert launches(prof, "layer_mix_adam") == 0
    state = state_of(models, mixes, [None] * 3)
    assert all(state[k]["mix.weights"].tobytes() != before[k]["mix.weights"].tobytes() for k in range(3))
    models, mixes, opts, loaders = setup()
    want = []
    for k in range(3):
        want += train_replicas_lockstep([models[k]], [opts[k]], [loaders[k]], loss_fn, 1, "cuda", mixes=[mixes[k]])
    assert got == want
    same_state(state, state_of(models, mixes, [None] * 3), "autograd loop, K = 3 against three K = 1 runs")


def test_a_mixed_and_an_unmixed_replica_share_a_call(rsaf_lib):
    import torch
    from cnnlstm_support import lockstep_setup
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam
    from src.models import train_replicas_lockstep
    seed = 29300
    loss_fn = torch.nn.CrossEntropyLoss()

    def setup():
        models, mixes, opts, loaders = layered_setup(seed)
        pm, po, pl = lockstep_setup(seed + 50, lambda k, m: FusedAdam(m, lr=2e-3), p=0.0)
        return [models[0], pm[1]], [mixes[0], None], [opts[0], po[1]], [loaders[0], pl[1]]

    models, mixes, opts, loaders = setup()
    got = train_replicas_lockstep(models, opts, loaders, loss_fn, 1, "cuda", mixes=mixes)
    a = [{k: v.detach().cpu().numpy().copy() for k, v in m.named_parameters()} for m in models] + [mixes[0].weights.detach().cpu().numpy().copy()]
    models, mixes, opts, loaders = setup()
    want = [train_replicas_lockstep([models[k]], [opts[k]], [loaders[k]], loss_fn, 1, "cuda", mixes=[mixes[k]])[0] for k in range(2)]
    assert got == want
    for k in range(2):
        for name, p in models[k].named_parameters():
            assert a[k][name].tobytes() == p.detach().cpu().numpy().tobytes(), (k, name)
    assert a[2].tobytes() == mixes[0].weights.detach().cpu().numpy().tobytes()


def test_train_eval_lockstep_restores_the_best_mix(rsaf_lib):
    import torch
    from src.models import train_eval_replicas_lockstep
    seed, epochs, patience = 29350, 3, 1
    loss_fn = torch.nn.CrossEntropyLoss()

    def run(ks):
        models, mixes, opts, loaders = layered_setup(seed)
        _, _, _, val_loaders = layered_setup(seed + 50, shuffle=False, with_opt=False)
        pick = lambda xs: [xs[k] for k in ks]                                      # noqa: E731
        res = train_eval_replicas_lockstep(pick(models), pick(opts), [None] * len(ks), pick(loaders), pick(val_loaders), loss_fn, epochs,
                                           patience, "cuda", mixes=pick(mixes))
        return res, pick(models), pick(mixes), pick(loaders), pick(val_loaders)

    res, models, mixes, loaders, val_loaders = run([0, 1, 2])
    state = state_of(models, mixes, [None] * 3)
    for k in range(3):
        one, m1, x1, _, _ = run([k])
        assert res[k][1] == one[0][1] and res[k][2] == one[0][2], (k, res[k][1:], one[0][1:])
        same_state([state[k]], state_of(m1, x1, [None]), f"best weights of replica {k}")
    # the restored mix is the best epoch's: replay the training to that epoch without validation
    from src.models import train_replicas_lockstep
    replayed = 0
    for k in range(3):
        best = int(np.argmin(res[k][2]))
        if best == len(res[k][2]) - 1:
            continue                                          # the last epoch was the best: nothing was rolled back
        m2, x2, o2, l2 = layered_setup(seed)
        train_replicas_lockstep([m2[k]], [o2[k]], [l2[k]], loss_fn, best + 1, "cuda", mixes=[x2[k]])
        same_state([state[k]], state_of([m2[k]], [x2[k]], [None]), f"replica {k} at its best epoch {best}")
        replayed += 1
    print(f"validation histories {[r[2] for r in res]}: {replayed} replicas rolled back to an earlier epoch")


def test_eval_lockstep_equals_the_forward_on_layer_mix(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group, eval_outputs
    from robust_speech_analysis_framework_amd.cnnlstm_loops import _eval_pairs, _grouped_eval_batches
    from src.models import eval_replicas_lockstep
    models, mixes, _, loaders = layered_setup(29400, shuffle=False, with_opt=False)
    _lib.prof_begin()
    got = eval_replicas_lockstep(models, loaders, "cuda", mixes=mixes)
    prof = _lib.prof_end()
    assert launches(prof, "train_collate_mix") == 1 and launches(prof, "train_collate") == 0       # 12 batches: one group call
    assert launches(prof, "layer_mix_forward") == 0 == launches(prof, "train_collate_mix_backward")
    with torch.no_grad():
        for k, (m, mix, ld) in enumerate(zip(models, mixes, loaders)):
            stacks = list(ld)                                 # the zero-padded stacks
            logits = cnnlstm_forward_group([m] * len(stacks), [mix(h) for h, _ in stacks])
            mine = [o for _, o, _ in _grouped_eval_batches(_eval_pairs([(k, m, ld, mix)]), "cuda")]
            for i, (a, b) in enumerate(zip(mine, logits)):
                same(bits(a), bits(b), f"replica {k} batch {i}: logits")
            prob, pred = eval_outputs(torch.cat(logits))
            labels = torch.cat([lab for _, lab in stacks])
            for name, a, b in zip(("labels", "predictions", "probabilities"), got[k], (labels, pred, prob)):
                b = b.cpu().numpy()
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (k, name)


def test_refusals_come_before_any_launch(rsaf_lib):
    import torch
    from cnnlstm_support import lockstep_setup
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import AugmentStream, DeviceSequenceDataset, FusedAdam, Scale
    from src.models import LayerMix, eval_replicas_lockstep, train_eval_replicas_lockstep, train_replicas_lockstep
    loss_fn = torch.nn.CrossEntropyLoss()
    models, mixes, opts, loaders = layered_setup(29450)
    pm, po, pl = lockstep_setup(29460, lambda k, m: FusedAdam(m, lr=2e-3))
    from src.models import cnnlstm_mix_train_step_group
    plans = [next(ld.plans()) for ld in loaders]              # uploads an epoch's order: ahead of the profiled window
    other = LayerMix(L).cuda()
    torch.cuda.synchronize()
    _lib.prof_begin()
    with pytest.raises(ValueError, match=r"optimizers\[1\].layer_mix is not mixes\[1\]"):
        cnnlstm_mix_train_step_group(models, [mixes[0], other, mixes[2]], opts, plans)
    with pytest.raises(ValueError, match=r"optimizers\[2\] is a FusedAdam that does not own mixes\[2\]"):
        train_replicas_lockstep(models, opts[:2] + [FusedAdam(models[2], lr=2e-3)], loaders, loss_fn, 1, "cuda", mixes=mixes)
    with pytest.raises(ValueError, match="loader 1 is a DeviceBatchLoader over a store of layer stacks.*mixes\\[1\\] is None"):
        train_replicas_lockstep(models, opts, loaders, loss_fn, 1, "cuda", mixes=[mixes[0], None, mixes[2]])
    with pytest.raises(ValueError, match="loader 0 is a DeviceBatchLoader over a store of layer stacks"):
        train_replicas_lockstep(models, opts, loaders, loss_fn, 1, "cuda")
    with pytest.raises(ValueError, match="loader 0 is a DeviceBatchLoader over a store of layer stacks"):
        eval_replicas_lockstep(models, loaders, "cuda")
    with pytest.raises(ValueError, match="mixes\\[1\\] is a LayerMix, but loader 1 is not"):
        train_replicas_lockstep(pm, po, pl, loss_fn, 1, "cuda", mixes=[None, LayerMix(L).cuda(), None])
    with pytest.raises(ValueError, match="mixes\\[2\\] has num_layers=4.*layers=3"):
        train_replicas_lockstep(models, opts, loaders, loss_fn, 1, "cuda", mixes=[mixes[0], mixes[1], LayerMix(4).cuda()])
    with pytest.raises(ValueError, match="val_loaders.*loader 0 is not a DeviceBatchLoader over a store of layer"):
        train_eval_replicas_lockstep(models, opts, [None] * 3, loaders, pl, loss_fn, 1, 1, "cuda", mixes=mixes)
    with pytest.raises(ValueError, match="transform is not supported over a store of layer stacks"):
        DeviceSequenceDataset(loaders[0].dataset.store, np.zeros(19, np.int64), transform=Scale(0.9, 1.1), augment_stream=AugmentStream(1))
    prof = _lib.prof_end()
    assert not prof, prof                                     # nothing was launched
    assert all(m.dropout_stream.step == 0 for m in models)
