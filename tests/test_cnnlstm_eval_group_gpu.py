"""Group eval forward of the CNN-LSTM on the MI355X: K eval-mode forwards through cnnlstm_forward_group / CNNLSTMGroup /
eval_model_grouped / eval_replicas_lockstep / train_eval_replicas_lockstep against the same forwards through
CNNLSTM.forward (bit for bit), against the reference's golden vectors, and against the reference's loops written out.

Exact equality is the bar between the group and the single path: per item both run the same kernels with the same launch
parameters in the same order (the recurrence and the head kernels share one body each; the fp16 planes of the weights are a
pure function of the blob), so a difference is a bug, not rounding.  Against the golden vectors the bar is the project's
1e-4 relative to the largest logit (tests/test_cnnlstm_gpu.py)."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from weights import synth_input, synth_state_dict  # noqa: E402
from cnnlstm_support import same  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4                             # tests/test_cnnlstm_gpu.py


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


GROUPS = {
    # D, C, H, act, [(B_k, T_k)]: one model per item
    "odd_t_tprime1_b1_empty_tiles": (16, 32, 64, "silu", [(3, 21), (4, 40), (1, 9), (1, 2), (2, 3)]),
    "fp32_path_two_and_three_row_tiles": (24, 64, 128, "gelu", [(2, 40), (5, 18), (9, 12)]),
    "identity_shortcut": (32, 32, 64, "gelu", [(2, 18), (2, 18)]),
    "reference_defaults_k5": (768, 128, 128, "silu", [(4, 64), (4, 300), (3, 64), (5, 128), (4, 200)]),
    "k16": (16, 32, 64, "silu", [(2, 12)] * 16),
    "k17_chunked": (16, 32, 64, "silu", [(2, 12)] * 17),
}
ONE_MODEL_SHAPES = [(4, 30), (4, 17), (2, 30), (1, 5), (4, 8), (3, 2)]


def build(D, C, H, seed, act, p_rate=0.5, p_block=0.2, layers=2, num_classes=2):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM
    m = CNNLSTM(input_dim=D, num_classes=num_classes, cnn_out_channels=C, lstm_hidden_dim=H, lstm_layers=layers, activation_fn=act,
                dropout_rate=p_rate)
    full = m.state_dict()
    for k, v in synth_state_dict(D, C, H, seed, num_classes=num_classes, layers=layers).items():
        full[k] = torch.from_numpy(v)
    m.load_state_dict(full)
    m.res_block1.dropout.p = p_block
    m.res_block2.dropout.p = p_block
    return m.to("cuda").eval()


def inputs(D, shapes, seed):
    import torch
    return [torch.from_numpy(synth_input(B, T, D, seed + k)).to("cuda") for k, (B, T) in enumerate(shapes)]


def singles(models, xs):
    """``model(x)`` of every pair on deep copies (one copy per distinct module)."""
    import torch
    copies = {}
    for m in models:
        if id(m) not in copies:
            copies[id(m)] = copy.deepcopy(m)
    want = [copies[id(m)](x).cpu().numpy() for m, x in zip(models, xs)]
    torch.cuda.synchronize()
    return want


def group_equals_singles(models, xs, what=""):
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group
    want = singles(models, xs)
    outs = cnnlstm_forward_group(models, xs)
    assert isinstance(outs, list) and len(outs) == len(xs)
    got = [o.cpu().numpy() for o in outs]
    for k, (g, w, x) in enumerate(zip(got, want, xs)):
        assert not outs[k].requires_grad
        same(g, w, f"{what} item {k} {tuple(x.shape)}")
    return got


def distinct_group_equals_singles(D, C, H, act, shapes, seed, layers=2, num_classes=2):
    models = [build(D, C, H, seed + 10 * k, act, layers=layers, num_classes=num_classes) for k in range(len(shapes))]
    xs = inputs(D, shapes, seed + 5000)
    group_equals_singles(models, xs)
    return models, xs


# ---- 1. bit for bit against model(x) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GROUPS))
def test_group_forward_equals_model_calls_bit_for_bit(name):
    D, C, H, act, shapes = GROUPS[name]
    distinct_group_equals_singles(D, C, H, act, shapes, 1100 + 100 * list(GROUPS).index(name))


def test_one_model_six_batches():
    m = build(16, 32, 64, 7100, "silu")
    group_equals_singles([m] * 6, inputs(16, ONE_MODEL_SHAPES, 7200))


def test_shared_weights_mixed_with_distinct_ones_and_weights_changed_in_place():
    """a, b, a, b, a: the planes of a are split once, in item 0's workspace, and read by items 2 and 4.  The second call, after
    fc.bias of b moved in place, must show the move (the packed-weights cache and the shared planes follow the parameters)."""
    import torch
    a, b = build(16, 32, 64, 7300, "silu"), build(16, 32, 64, 7310, "silu")
    models = [a, b, a, b, a]
    xs = inputs(16, [(3, 21), (2, 30), (4, 16), (1, 9), (2, 12)], 7400)
    first = group_equals_singles(models, xs, "first call")
    with torch.no_grad():
        b.fc.bias.add_(1.0)
    second = group_equals_singles(models, xs, "second call")
    for k in (0, 2, 4):
        same(second[k], first[k], f"item {k} (model a, untouched)")
    for k in (1, 3):
        assert np.allclose(second[k] - first[k], 1.0, atol=1e-5), (k, second[k] - first[k])


# ---- 2. against the reference's own vectors -----------------------------------------------------------------------------------
def golden_model(D, C, H, act, sd):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM
    m = CNNLSTM(input_dim=D, cnn_out_channels=C, lstm_hidden_dim=H, activation_fn=act)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    return m.cuda().eval()


def golden_case(name):
    import torch
    z = np.load(os.path.join(HERE, "golden", name))
    D, C, H, B, T, seed = [int(v) for v in z["meta"]]
    m = golden_model(D, C, H, str(z["act"]), synth_state_dict(D, C, H, seed))
    return m, torch.from_numpy(synth_input(B, T, D, seed + 1000)).cuda(), z["logits"]


@pytest.mark.parametrize("names", [("cnnlstm_d16_c32_h64_silu.npz", "cnnlstm_d16_c32_h64_silu_odd.npz"),
                                   ("cnnlstm_d768_c128_h128_silu.npz",)], ids=["d16_pair", "d768_k1"])
def test_group_forward_matches_reference_golden(names):
    """Guards against the group path and the single path being equally wrong."""
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group
    cases = [golden_case(n) for n in names]
    outs = cnnlstm_forward_group([c[0] for c in cases], [c[1] for c in cases])
    for n, o, (_, x, want) in zip(names, outs, cases):
        err = _rel(o.cpu().numpy(), want)
        print(f"{n}: rel err {err:.2e}")
        assert o.shape == (x.shape[0], 2) and err < TOL, (n, err)


def test_ragged_zero_padded_pair_and_clip_alone_through_one_model():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group, collate_zero_pad
    z = np.load(os.path.join(HERE, "golden", "cnnlstm_ragged_pad.npz"))
    D, C, H, B, T, seed = [int(v) for v in z["meta"]]
    m = golden_model(D, C, H, "silu", synth_state_dict(D, C, H, seed))
    a, b = synth_input(1, 37, D, 2001)[0], synth_input(1, 64, D, 2002)[0]
    padded, alone = cnnlstm_forward_group([m, m], [collate_zero_pad([a, b]), torch.from_numpy(a[None]).cuda()])
    e1, e2 = _rel(padded.cpu().numpy(), z["logits_padded"]), _rel(alone.cpu().numpy(), z["logits_alone"])
    print(f"padded pair {e1:.2e}, clip alone {e2:.2e}")
    assert e1 < TOL and e2 < TOL


# ---- 3. the grouping happens ----------------------------------------------------------------------------------------------
def profiled(fn):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    fn()                                                          # workspace, packed weights
    torch.cuda.synchronize()
    _lib.prof_begin()
    fn()
    torch.cuda.synchronize()
    return _lib.prof_end()


def test_one_recurrence_launch_per_layer_and_one_head_launch():
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group
    D, C, H, act, shapes = GROUPS["reference_defaults_k5"]
    models = [build(D, C, H, 8100 + 10 * k, act) for k in range(len(shapes))]
    assert models[0].dims["layers"] == 2
    xs = inputs(D, shapes, 8200)
    pr = profiled(lambda: cnnlstm_forward_group(models, xs))
    print({k: v["launches"] for k, v in pr.items()})
    assert pr["lstm_recurrent"]["launches"] == 2
    assert pr["attnpool_fc"]["launches"] == 1


@pytest.mark.parametrize("layers", [1, 2])
def test_weights_of_one_model_are_split_once(layers):
    """launch_split_f16x2 reports under `split_f16x2`.  With one LSTM layer that family holds the weight matrices only (five
    convolution matrices less the absent ones, one W_ih), and six batches of one model show the count of one batch.  From the
    second layer on every item also splits its own previous layer's output under the same tag: one more per item and layer,
    which is per-item data and stays per item."""
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_forward_group
    m = build(16, 32, 64, 8300, "silu", layers=layers)
    xs = inputs(16, ONE_MODEL_SHAPES, 8400)
    one = profiled(lambda: m(xs[0]))["split_f16x2"]["launches"]
    assert one == 5 + layers + (layers - 1)
    six = profiled(lambda: cnnlstm_forward_group([m] * 6, xs))["split_f16x2"]["launches"]
    print(f"layers {layers}: one item {one} launches, six items of one model {six}")
    assert six == one + 5 * (layers - 1)
    other = build(16, 32, 64, 8310, "silu", layers=layers)           # distinct weights are split per model
    two = profiled(lambda: cnnlstm_forward_group([m, other, m], xs[:3]))["split_f16x2"]["launches"]
    assert two == 2 * (5 + layers) + 3 * (layers - 1)


# ---- 4. CNNLSTMGroup(...).eval() --------------------------------------------------------------------------------------------
def test_group_module_in_eval_mode_with_a_replica_sitting_out():
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTMGroup, cnnlstm_forward_group
    shapes = [(3, 21), (2, 30), (4, 16)]
    models = [build(16, 32, 64, 8500 + 10 * k, "silu") for k in range(3)]
    xs = inputs(16, shapes, 8600)
    want = singles(models, xs)
    g = CNNLSTMGroup(models).eval()
    outs = g([xs[0], None, xs[2]])
    assert outs[1] is None
    same(outs[0].cpu().numpy(), want[0], "replica 0")
    same(outs[2].cpu().numpy(), want[2], "replica 2")
    for k, o in enumerate(g(xs)):
        same(o.cpu().numpy(), want[k], f"replica {k}")
    models[1].train()
    with pytest.raises(ValueError, match="replica 1 is in training mode: "):
        cnnlstm_forward_group(models, xs)


# ---- 5. above the 4-row threshold ----------------------------------------------------------------------------------------
def test_group_above_the_four_row_threshold_in_a_subprocess():
    """With RSAF_LSTM_SMALL_MAX=0 (read once per process) every batch is above the 4-row threshold: the group entry launches
    every recurrence on its own through the 16-row kernel, and the logits still equal the single forwards bit for bit."""
    import subprocess
    code = r'''
import sys
sys.path.insert(0, "tests")
import test_cnnlstm_eval_group_gpu as t
t.distinct_group_equals_singles(24, 64, 128, "gelu", [(2, 40), (19, 12)], 5100)
t.distinct_group_equals_singles(16, 48, 64, "silu", [(5, 13), (2, 9)], 5200, layers=3, num_classes=5)    # row 2 of tests/cnnlstm_geometry.py
print("EVAL_GROUP_SIXTEEN_ROW_OK")
'''
    env = dict(os.environ, RSAF_LSTM_SMALL_MAX="0")
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "EVAL_GROUP_SIXTEEN_ROW_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 6. / 7. the reference's loops ------------------------------------------------------------------------------------------
def make_loader(n_seq, seed, D=16):
    import torch
    from torch.utils.data import DataLoader
    from robust_speech_analysis_framework_amd.cnnlstm import collate_zero_pad

    def collate(batch):
        return collate_zero_pad([b[0] for b in batch], device="cpu"), torch.tensor([b[1] for b in batch], dtype=torch.long)

    rng = np.random.Generator(np.random.PCG64(seed))
    data = [(synth_input(1, int(rng.integers(10, 31)), D, seed + 1 + i)[0], int(rng.integers(0, 2))) for i in range(n_seq)]
    return DataLoader(data, batch_size=4, shuffle=False, collate_fn=collate)


def reference_eval_model(model, data_loader, device):
    """src/dl_cv_strategies.py:183-194"""
    import torch
    model.eval()
    preds, probs, labels = [], [], []
    with torch.no_grad():
        for seq, lab in data_loader:
            seq, lab = seq.to(device), lab.to(device)
            out = model(seq)
            prob = torch.softmax(out, dim=1)[:, 1]
            pred = torch.argmax(out, dim=1)
            preds.extend(pred.cpu().numpy())
            probs.extend(prob.cpu().numpy())
            labels.extend(lab.cpu().numpy())
    return np.array(labels), np.array(preds), np.array(probs)


def test_grouped_eval_equals_the_reference_eval_loop():
    from robust_speech_analysis_framework_amd.cnnlstm import eval_model_grouped, eval_replicas_lockstep
    models = [build(16, 32, 64, 9100 + 10 * k, "silu") for k in range(3)]
    loaders = [make_loader(n, 9200 + 100 * k) for k, n in enumerate((19, 12, 14))]      # batch 4 -> 5, 3 and 4 batches
    assert [len(ld) for ld in loaders] == [5, 3, 4]
    want = [reference_eval_model(copy.deepcopy(m), ld, "cuda") for m, ld in zip(models, loaders)]
    got = eval_replicas_lockstep(models, loaders, "cuda")
    assert len(got) == 3
    for k in range(3):
        for name, g, w in zip(("labels", "preds", "probs"), got[k], want[k]):
            assert g.dtype == w.dtype, (k, name, g.dtype, w.dtype)
            same(g, w, f"replica {k} {name}")
    one = eval_model_grouped(models[1], loaders[1], "cuda")
    for name, g, w in zip(("labels", "preds", "probs"), one, want[1]):
        same(g, w, f"eval_model_grouped {name}")
    assert len(want[0][0]) == 19 and want[0][2].dtype == np.float32


def reference_train_eval_loop(model, train_loader, val_loader, loss_fn, optimizer, scheduler, device, epochs, patience):
    """src/dl_cv_strategies.py:112-165"""
    import torch
    histories = {'train_loss': [], 'val_loss': []}
    best_val_loss = float('inf')
    epochs_no_improve = 0
    best_model_weights = None
    for epoch in range(epochs):
        model.train()
        train_loss = 0
        for seq, lab in train_loader:
            seq, lab = seq.to(device), lab.to(device)
            optimizer.zero_grad()
            out = model(seq)
            loss = loss_fn(out, lab)
            loss.backward()
            optimizer.step()
            train_loss += loss.item()
        histories['train_loss'].append(train_loss / len(train_loader))
        model.eval()
        val_loss = 0
        with torch.no_grad():
            for seq, lab in val_loader:
                seq, lab = seq.to(device), lab.to(device)
                out = model(seq)
                loss = loss_fn(out, lab)
                val_loss += loss.item()
        avg_val_loss = val_loss / len(val_loader)
        histories['val_loss'].append(avg_val_loss)
        scheduler.step(avg_val_loss)
        if avg_val_loss < best_val_loss:
            best_val_loss = avg_val_loss
            best_model_weights = copy.deepcopy(model.state_dict())
            epochs_no_improve = 0
        else:
            epochs_no_improve += 1
        if epochs_no_improve >= patience:
            break
    if best_model_weights:
        model.load_state_dict(best_model_weights)
    return model, histories['train_loss'], histories['val_loss']


TRAIN_EVAL_LRS = (1e-3, 1e-2, 5e-2)      # chosen on the sequential reference loop alone, see the test
EPOCHS, PATIENCE = 6, 2


def train_eval_setup():
    import torch
    models = [build(16, 32, 64, 9500 + 10 * k, "silu", p_rate=0.0, p_block=0.0) for k in range(3)]
    train_loaders = [make_loader(n, 9600 + 100 * k) for k, n in enumerate((19, 12, 14))]
    val_loaders = [make_loader(n, 9700 + 100 * k) for k, n in enumerate((7, 9, 6))]       # 2, 3 and 2 batches
    opts = [torch.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(models, TRAIN_EVAL_LRS)]
    scheds = [torch.optim.lr_scheduler.ReduceLROnPlateau(o, factor=0.1, patience=1) for o in opts]
    return models, opts, scheds, train_loaders, val_loaders


def test_train_eval_lockstep_equals_sequential_train_eval_loops():
    """_train_eval_loop for three replicas (no dropout: no RNG involved), each with its own Adam and ReduceLROnPlateau,
    against three sequential runs of that loop on copies.  The learning rates were picked by running the sequential loop
    alone until its runs stop at different epochs, one of them early; that is asserted on the sequential histories."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import train_eval_replicas_lockstep
    loss_fn = torch.nn.CrossEntropyLoss()
    models, opts, scheds, train_loaders, val_loaders = train_eval_setup()
    seq_models, seq_opts, seq_scheds, _, _ = train_eval_setup()                          # the same seeds: equal copies
    for a, b in zip(models, seq_models):
        for (k, v), (_, w) in zip(a.state_dict().items(), b.state_dict().items()):
            same(v.cpu().numpy(), w.cpu().numpy(), f"initial {k}")

    want = [reference_train_eval_loop(m, tl, vl, loss_fn, o, s, "cuda", EPOCHS, PATIENCE)
            for m, o, s, tl, vl in zip(seq_models, seq_opts, seq_scheds, train_loaders, val_loaders)]
    stops = [len(w[2]) for w in want]
    print("sequential runs stop after epochs", stops, "val", [w[2] for w in want])
    assert len(set(stops)) == 3 and min(stops) < EPOCHS, stops

    got = train_eval_replicas_lockstep(models, opts, scheds, train_loaders, val_loaders, loss_fn, EPOCHS, PATIENCE, "cuda")
    assert len(got) == 3
    for k, ((gm, gt, gv), (wm, wt, wv)) in enumerate(zip(got, want)):
        assert gm is models[k]
        assert gt == wt, (k, gt, wt)
        assert gv == wv, (k, gv, wv)
        got_sd, want_sd = gm.state_dict(), wm.state_dict()
        assert list(got_sd) == list(want_sd)
        for key, v in want_sd.items():
            same(got_sd[key].cpu().numpy(), v.cpu().numpy(), f"replica {k} {key}")
        assert opts[k].param_groups[0]["lr"] == seq_opts[k].param_groups[0]["lr"], k
