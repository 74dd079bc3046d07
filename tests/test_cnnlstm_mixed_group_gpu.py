"""Mixed groups of the CNN-LSTM on the MI355X: replicas of different architecture (channels, hidden size, activation) through
``mixed=True`` of the group calls against the same replicas through the existing paths, single calls or one group call per
architecture.

Exact equality (``np.array_equal``) is the only bar.  Per item a mixed call runs the kernels of the single call with the same
launch parameters in the same order, and the mixed recurrence and head kernels share their bodies with the single and the
group kernels, so a difference is a bug, not rounding.  The existing paths are held to the reference's goldens and to float64
by their own tests.

Run as a script (``python tests/test_cnnlstm_mixed_group_gpu.py train_vs_singles``) the file runs the comparison of the
training step once: the child process of the test that lowers RSAF_LSTM_SMALL_MAX, which the library reads once."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from weights import synth_input, synth_state_dict  # noqa: E402
from cnnlstm_support import same  # noqa: E402

pytestmark = pytest.mark.gpu

D, NC = 16, 2
A = (16, 64, "silu")                 # identity shortcut: C == D
B_ = (32, 64, "gelu")
C_ = (32, 128, "silu")
D_ = (64, 128, "gelu")
ARCHS = [A, B_, C_, D_]
SHAPES = [(2, 6), (5, 7), (3, 9), (1, 12)]       # odd T, a partly filled second 4-row tile, a loop length per item


def build(arch, seed, layers=2, train=True):
    """A seeded CNNLSTM of ``arch`` on the device with a DropoutStream of its own (so a deep copy draws the same masks)."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, DropoutStream
    Cc, H, act = arch
    m = CNNLSTM(input_dim=D, num_classes=NC, cnn_out_channels=Cc, lstm_hidden_dim=H, lstm_layers=layers, activation_fn=act,
                dropout_rate=0.5)
    full = m.state_dict()
    for k, v in synth_state_dict(D, Cc, H, seed, num_classes=NC, layers=layers).items():
        full[k] = torch.from_numpy(v)
    m.load_state_dict(full)
    m.res_block1.dropout.p = m.res_block2.dropout.p = 0.2
    m.dropout_stream = DropoutStream(seed)
    m = m.to("cuda")
    return m.train() if train else m.eval()


def inputs(shapes, seed):
    import torch
    return [torch.from_numpy(synth_input(B, T, D, seed + k)).to("cuda") for k, (B, T) in enumerate(shapes)]


def labels(shapes, seed):
    import torch
    return [torch.from_numpy(np.random.Generator(np.random.PCG64(seed + k)).integers(0, NC, B)).to("cuda")
            for k, (B, _) in enumerate(shapes)]


def host(t):
    return t.detach().cpu().numpy()


def same_model(got, want, what, grads=False):
    """Parameters (``grads``: their gradients as well) and buffers, running statistics and num_batches_tracked included."""
    for (k, p), q in zip(got.named_parameters(), want.parameters()):
        same(host(p), host(q), f"{what} parameter {k}")
        if grads:
            assert p.grad is not None and q.grad is not None, (what, k)
            same(host(p.grad), host(q.grad), f"{what} grad {k}")
    for (k, p), q in zip(got.named_buffers(), want.buffers()):
        same(host(p), host(q), f"{what} buffer {k}")


# ---- 1. training forward + backward -------------------------------------------------------------------------------------------
def train_vs_singles(archs, shapes, seed, layers):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_group
    models = [build(a, seed + 10 * k, layers) for k, a in enumerate(archs)]
    refs = [copy.deepcopy(m) for m in models]
    xs, labs = inputs(shapes, seed + 500), labels(shapes, seed + 600)
    ce = torch.nn.CrossEntropyLoss()
    outs = cnnlstm_train_group(models, xs, mixed=True)
    assert isinstance(outs, list) and len(outs) == len(models)
    torch.stack([ce(o, lab) for o, lab in zip(outs, labs)]).sum().backward()
    for k, (m, x, lab) in enumerate(zip(refs, xs, labs)):
        out = m(x)
        ce(out, lab).backward()
        what = f"replica {k} {archs[k]} {shapes[k]}"
        same(host(outs[k]), host(out), f"{what} logits")
        same_model(models[k], m, what, grads=True)
        assert models[k].dropout_stream.step == m.dropout_stream.step == 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("layers,reverse", [(2, False), (2, True), (1, False)], ids=["l2", "l2_reversed", "l1"])
def test_mixed_training_step_equals_single_steps(layers, reverse):
    archs, shapes = (ARCHS[::-1], SHAPES[::-1]) if reverse else (ARCHS, SHAPES)      # reversed: an H = 128 item comes first
    train_vs_singles(archs, shapes, 100 + 1000 * layers, layers)


# ---- 2. eval forward ------------------------------------------------------------------------------------------------------------
def eval_singles(models, xs):
    copies = {}
    for m in models:
        if id(m) not in copies:
            copies[id(m)] = copy.deepcopy(m)
    return [host(copies[id(m)](x)) for m, x in zip(models, xs)]


@pytest.mark.parametrize("layers", [2, 1])
def test_mixed_eval_forward_equals_model_calls(layers):
    """a, b, a, c, d: model a twice, so its weight planes are prepared once and read by item 2."""
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group
    a, b, c, d = [build(arch, 3000 + 10 * k, layers, train=False) for k, arch in enumerate(ARCHS)]
    models = [a, b, a, c, d]
    xs = inputs(SHAPES[:3] + [SHAPES[3], SHAPES[1]], 3500)
    want = eval_singles(models, xs)
    outs = cnnlstm_forward_group(models, xs, mixed=True)
    assert isinstance(outs, list) and len(outs) == 5
    for k, (o, w) in enumerate(zip(outs, want)):
        assert not o.requires_grad
        same(host(o), w, f"item {k} {tuple(xs[k].shape)}")


# ---- 3. fused step --------------------------------------------------------------------------------------------------------------
def optimizer_state(opt, model):
    return [(k, host(opt.state[p]["exp_avg"]), host(opt.state[p]["exp_avg_sq"]), int(opt.state[p]["step"]))
            for k, p in model.named_parameters()]


def test_mixed_fused_step_equals_group_steps_per_architecture():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, cnnlstm_train_step_group
    archs = [B_, C_, B_, C_]                                     # two replicas of each of two architectures, interleaved
    shapes = [(2, 6), (5, 7), (3, 9), (1, 12)]
    models = [build(a, 4000 + 10 * k) for k, a in enumerate(archs)]
    refs = [copy.deepcopy(m) for m in models]
    lrs = [1e-3, 3e-3, 2e-3, 5e-4]
    opts = [FusedAdam(m, lr=lr) for m, lr in zip(models, lrs)]
    ropts = [FusedAdam(m, lr=lr) for m, lr in zip(refs, lrs)]
    for step in range(2):
        xs, labs = inputs(shapes, 4500 + 10 * step), labels(shapes, 4600 + 10 * step)
        losses, logits = cnnlstm_train_step_group(models, opts, xs, labs, mixed=True)
        assert losses.shape == (4,) and len(logits) == 4
        for part in ((0, 2), (1, 3)):                               # the same replicas, one group call per architecture
            pl, plog = cnnlstm_train_step_group([refs[k] for k in part], [ropts[k] for k in part], [xs[k] for k in part],
                                                [labs[k] for k in part])
            for j, k in enumerate(part):
                same(host(losses[k]), host(pl[j]), f"step {step} replica {k} loss")
                same(host(logits[k]), host(plog[j]), f"step {step} replica {k} logits")
        for k in range(4):
            what = f"step {step} replica {k} {archs[k]}"
            same_model(models[k], refs[k], what)
            for (name, m1, v1, t1), (_, m2, v2, t2) in zip(optimizer_state(opts[k], models[k]), optimizer_state(ropts[k], refs[k])):
                same(m1, m2, f"{what} exp_avg {name}")
                same(v1, v2, f"{what} exp_avg_sq {name}")
                assert t1 == t2 == step + 1, (what, name)
            assert int(models[k].res_block1.bn1.num_batches_tracked) == step + 1
    torch.cuda.synchronize()


# ---- 4. lock-step loop ----------------------------------------------------------------------------------------------------------
def test_mixed_lockstep_training_equals_lockstep_per_architecture():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_eval_replicas_lockstep
    archs = [A, D_, A, D_]
    models = [build(a, 5000 + 10 * k) for k, a in enumerate(archs)]
    refs = [copy.deepcopy(m) for m in models]

    def loader(n, seed):
        shapes = [SHAPES[(seed + i) % 4] for i in range(n)]
        return [(x.cpu(), lab.cpu()) for x, lab in zip(inputs(shapes, seed), labels(shapes, seed + 50))]

    train_loaders = [loader(3, 5100 + 10 * k) for k in range(4)]
    val_loaders = [loader(2, 5200 + 10 * k) for k in range(4)]
    ce = torch.nn.CrossEntropyLoss()
    got = train_eval_replicas_lockstep(models, [FusedAdam(m, lr=2e-3) for m in models], [None] * 4, train_loaders, val_loaders, ce,
                                       2, 2, "cuda", mixed=True)
    want = [None] * 4
    for part in ((0, 2), (1, 3)):
        res = train_eval_replicas_lockstep([refs[k] for k in part], [FusedAdam(refs[k], lr=2e-3) for k in part], [None] * 2,
                                           [train_loaders[k] for k in part], [val_loaders[k] for k in part], ce, 2, 2, "cuda")
        for k, r in zip(part, res):
            want[k] = r
    for k in range(4):
        (m, th, vh), (rm, rth, rvh) = got[k], want[k]
        assert m is models[k] and len(th) == len(vh) == 2
        assert th == rth and vh == rvh, (k, th, rth, vh, rvh)
        sd, rsd = m.state_dict(), rm.state_dict()
        assert list(sd) == list(rsd)
        for key in sd:
            same(host(sd[key]), host(rsd[key]), f"replica {k} {archs[k]} state_dict {key}")


# ---- 5. chunking ----------------------------------------------------------------------------------------------------------------
def test_seventeen_items_of_alternating_architecture_are_chunked():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group, cnnlstm_train_group, train_group_max
    assert train_group_max() == 16
    archs = [A if k % 2 == 0 else C_ for k in range(17)]
    shapes = [(2, 4)] * 17
    # eval group: two modules, 17 batches
    ea, ec = build(A, 6000, train=False), build(C_, 6010, train=False)
    emodels = [ea if k % 2 == 0 else ec for k in range(17)]
    xs = inputs(shapes, 6100)
    want = eval_singles(emodels, xs)
    for k, o in enumerate(cnnlstm_forward_group(emodels, xs, mixed=True)):
        same(host(o), want[k], f"eval item {k}")
    # training group: 17 replicas
    models = [build(a, 6200 + 10 * k) for k, a in enumerate(archs)]
    refs = [copy.deepcopy(m) for m in models]
    outs = cnnlstm_train_group(models, xs, mixed=True)
    torch.stack([o.square().sum() for o in outs]).sum().backward()
    for k, (m, x) in enumerate(zip(refs, xs)):
        out = m(x)
        out.square().sum().backward()
        same(host(outs[k]), host(out), f"training replica {k} logits")
        same_model(models[k], m, f"training replica {k}", grads=True)


# ---- 6. the grouping happens ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 1])
def test_one_recurrence_launch_per_layer_and_pass_and_one_head_launch(layers):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group, cnnlstm_train_group
    models = [build(a, 7000 + 10 * k, layers) for k, a in enumerate(ARCHS)]          # H = 64, 64, 128, 128
    xs = inputs(SHAPES, 7100)
    _lib.prof_begin()
    outs = cnnlstm_train_group(models, xs, mixed=True)
    torch.stack([o.sum() for o in outs]).sum().backward()
    torch.cuda.synchronize()
    pr = _lib.prof_end()
    print({k: v["launches"] for k, v in pr.items()})
    assert pr["lstm_recurrent"]["launches"] == layers
    assert pr["lstm_bwd_recurrent"]["launches"] == layers
    for m in models:
        m.eval()
    _lib.prof_begin()
    cnnlstm_forward_group(models, xs, mixed=True)
    torch.cuda.synchronize()
    pr = _lib.prof_end()
    print({k: v["launches"] for k, v in pr.items()})
    assert pr["lstm_recurrent"]["launches"] == layers
    assert pr["attnpool_fc"]["launches"] == 1


# ---- 7. a batch above the 4-row threshold ---------------------------------------------------------------------------------------
def test_items_above_the_small_batch_threshold_run_on_their_own():
    """RSAF_LSTM_SMALL_MAX = 2 (read once per process, hence the child): the B = 3 and B = 5 items take the stand-alone
    16-row recurrence, in the mixed call as in the single calls, while B = 2 and B = 1 stay grouped."""
    env = dict(os.environ, RSAF_LSTM_SMALL_MAX="2")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "train_vs_singles"], env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "train_vs_singles ok" in r.stdout
    assert "lstm_recurrent launches 6" in r.stdout and "lstm_bwd_recurrent launches 6" in r.stdout


if __name__ == "__main__":
    assert sys.argv[1:] == ["train_vs_singles"], sys.argv
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_group
    train_vs_singles(ARCHS, SHAPES, 8000, 2)
    # per layer and pass: one grouped launch (B = 2 and B = 1) and one launch each for B = 5 and B = 3
    models = [build(a, 8100 + 10 * k) for k, a in enumerate(ARCHS)]
    _lib.prof_begin()
    outs = cnnlstm_train_group(models, inputs(SHAPES, 8200), mixed=True)
    torch.stack([o.sum() for o in outs]).sum().backward()
    torch.cuda.synchronize()
    pr = _lib.prof_end()
    for fam in ("lstm_recurrent", "lstm_bwd_recurrent"):
        print(f"{fam} launches {pr[fam]['launches']}")
    print("train_vs_singles ok")
