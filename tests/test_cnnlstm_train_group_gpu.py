"""Group training step of the CNN-LSTM on the MI355X: K replicas through cnnlstm_train_group / CNNLSTMGroup /
train_replicas_lockstep against K single steps through CNNLSTM.forward (bit for bit) and against the training oracle.

Exact equality is the bar between the group and the single path: both run the same device code in the same order per
replica (the recurrence kernels of cnnlstm_lstm.hip share one body) and every reduction of the step has a fixed partition (header
comment of cnnlstm_train.hip; the sums of the loss and the gradient norm: the fixed tree of cnnlstm_optim.hip), so a difference is a bug, not rounding.  Against the float64 oracle the bar is the project's 1e-4
relative to each tensor's largest magnitude (tests/test_cnnlstm_train_gpu.py)."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from weights import synth_input  # noqa: E402
from cnnlstm_support import RTOL, build, check_grads, device_masks, same  # noqa: E402

from oracle import cnnlstm_train_oracle as to

pytestmark = pytest.mark.gpu

P_BLOCK, P_RATE = 0.2, 0.5

GROUPS = {
    # D, C, H, act, [(B_k, T_k)]
    "odd_t_b1_tiny": (16, 32, 64, "silu", [(3, 21), (4, 40), (1, 9), (2, 4)]),
    "two_row_tiles": (24, 64, 128, "gelu", [(2, 40), (5, 18), (4, 40)]),
    "identity_shortcut_equal_shapes": (32, 32, 64, "gelu", [(2, 18), (2, 18)]),
    "reference_defaults_k5": (768, 128, 128, "silu", [(4, 64), (4, 300), (4, 128), (3, 64), (4, 200)]),
    "k16": (16, 32, 64, "silu", [(2, 12)] * 16),
    "k17_chunked": (16, 32, 64, "silu", [(2, 12)] * 17),
}


def make_replica(D, C, H, act, B, T, s, num_classes=2, layers=2):
    m, sd = build(D, C, H, s, act, p_rate=P_RATE, p_block=P_BLOCK, num_classes=num_classes, layers=layers)
    return {"model": m, "sd": sd, "x": synth_input(B, T, D, s + 1),
            "labels": np.random.Generator(np.random.PCG64(s + 2)).integers(0, num_classes, B),
            "masks": to.make_masks(B, T, C, H, P_BLOCK, P_RATE, s + 3, layers=layers)}


def make_group(D, C, H, act, shapes, seed, num_classes=2, layers=2):
    """K replicas with own weights, data, labels and dropout masks."""
    return [make_replica(D, C, H, act, B, T, seed + 10 * k, num_classes, layers) for k, (B, T) in enumerate(shapes)]


def state_of(m):
    return {"grads": {k: (None if p.grad is None else p.grad.detach().cpu().numpy()) for k, p in m.named_parameters()},
            "buffers": {k: v.detach().cpu().numpy() for k, v in m.named_buffers()}}


def single_step(m, rep):
    import torch
    m.forced_masks = device_masks(rep["masks"])
    m.zero_grad()
    out = m(torch.from_numpy(rep["x"]).to("cuda"))
    loss = torch.nn.CrossEntropyLoss()(out, torch.from_numpy(rep["labels"]).to("cuda"))
    loss.backward()
    torch.cuda.synchronize()
    return dict(state_of(m), logits=out.detach().cpu().numpy(), loss=loss.item())


def group_step(reps, in_loss=None):
    """One group step; only the outputs listed in `in_loss` (default: all) enter the summed loss."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_group
    models = [r["model"] for r in reps]
    for m in models:
        m.zero_grad()
    outs = cnnlstm_train_group(models, [torch.from_numpy(r["x"]).to("cuda") for r in reps],
                               masks=[device_masks(r["masks"]) for r in reps])
    assert isinstance(outs, list) and len(outs) == len(reps)
    ce = torch.nn.CrossEntropyLoss()
    losses = [ce(o, torch.from_numpy(r["labels"]).to("cuda")) for o, r in zip(outs, reps)]
    keep = range(len(reps)) if in_loss is None else in_loss
    torch.stack([losses[k] for k in keep]).sum().backward()
    torch.cuda.synchronize()
    return [dict(state_of(m), logits=o.detach().cpu().numpy(), loss=ls.item()) for m, o, ls in zip(models, outs, losses)], outs


def same_step(got, want, what):
    same(got["logits"], want["logits"], f"{what} logits")
    same(got["loss"], want["loss"], f"{what} loss")
    assert set(got["grads"]) == set(want["grads"])
    for k, g in want["grads"].items():
        assert g is not None and got["grads"][k] is not None, (what, k)
        same(got["grads"][k], g, f"{what} grad {k}")
    for k, v in want["buffers"].items():
        same(got["buffers"][k], v, f"{what} buffer {k}")


def group_equals_singles(D, C, H, act, shapes, seed, num_classes=2, layers=2):
    reps = make_group(D, C, H, act, shapes, seed, num_classes, layers)
    singles = [copy.deepcopy(r["model"]) for r in reps]
    got, _ = group_step(reps)
    for k, (m, r) in enumerate(zip(singles, reps)):
        same_step(got[k], single_step(m, r), f"replica {k} {shapes[k]}")
    return reps, got


@pytest.mark.parametrize("name", list(GROUPS))
def test_group_step_equals_single_steps_bit_for_bit(name):
    D, C, H, act, shapes = GROUPS[name]
    group_equals_singles(D, C, H, act, shapes, 1100 + 100 * list(GROUPS).index(name))


# max_pool1d(2) hands the gradient of a pair of frames to the larger one: the step is discontinuous where the two are
# equal.  A float32 path and the float64 oracle may then legitimately pick different frames of a pair that lies closer
# together than the float32 rounding error of the values compared (BatchNorm-ed dot products of up to K = 3 * 768
# terms: sqrt(K) * 2^-24 = 2.9e-6), and every gradient of res_block1 moves by 1e-3 .. 1e-2 of its scale: the single step
# shows exactly that, on the parent commit too, for inputs whose closest pair is 3.0e-7 apart.  Such an input cannot be
# compared with an oracle at 1e-4, so a replica's data are drawn again (next seed) until the ORACLE's own forward has no
# pool pair closer than POOL_GAP; the code under test has no part in that choice.
POOL_GAP = 4e-6


def oracle_step(r, act):
    want = to.forward_backward(r["sd"], r["x"], r["labels"], act, masks=r["masks"], return_stages=True)
    h = want["stages"]["res1"]                                      # [B, T, C], what the pool compares
    Tp = h.shape[1] // 2
    return want, float(np.abs(h[:, 0:2 * Tp:2] - h[:, 1:2 * Tp:2]).min())


def make_well_posed_group(D, C, H, act, shapes, seed):
    reps, wants = [], []
    for k, (B, T) in enumerate(shapes):
        for attempt in range(40):
            r = make_replica(D, C, H, act, B, T, seed + 10 * k + 1000 * attempt)
            want, gap = oracle_step(r, act)
            print(f"replica {k} {(B, T)} seed {seed + 10 * k + 1000 * attempt}: closest pool pair of the oracle {gap:.2e}")
            if gap >= POOL_GAP:
                break
        else:
            raise AssertionError(f"no well-posed input for replica {k} in 40 draws")
        reps.append(r)
        wants.append(want)
    return reps, wants


@pytest.mark.parametrize("name", ["odd_t_b1_tiny", "two_row_tiles", "reference_defaults_k5"])
def test_group_step_matches_oracle(name):
    """Guards against the bit-identity test comparing two equally wrong paths."""
    D, C, H, act, shapes = GROUPS[name]
    reps, wants = make_well_posed_group(D, C, H, act, shapes, 2100 + 100 * list(GROUPS).index(name))
    got, _ = group_step(reps)
    for k, (r, want) in enumerate(zip(reps, wants)):
        err = np.abs(got[k]["logits"] - want["logits"]).max() / max(np.abs(want["logits"]).max(), 1.0)
        print(f"{name} replica {k} {shapes[k]}: logits err {err:.2e}, loss diff {abs(got[k]['loss'] - want['loss']):.2e}")
        assert err < RTOL, (k, err)
        assert abs(got[k]["loss"] - want["loss"]) < RTOL, k
        check_grads(got[k]["grads"], want["grads"])
        new = to.updated_bn_buffers(r["sd"], want["bn_stats"])
        for key, v in new.items():
            assert np.abs(got[k]["buffers"][key] - v).max() < RTOL * max(np.abs(v).max(), 1e-3), (k, key)


def test_output_outside_the_loss_gets_no_gradient():
    D, C, H, act, shapes = 16, 32, 64, "silu", [(3, 21), (2, 30), (4, 16)]
    reps = make_group(D, C, H, act, shapes, 3100)
    singles = [copy.deepcopy(r["model"]) for r in reps]
    before = state_of(reps[1]["model"])["buffers"]
    got, _ = group_step(reps, in_loss=[0, 2])
    assert all(g is None for g in got[1]["grads"].values())
    after = got[1]["buffers"]
    for k, v in after.items():                        # its forward ran: the BatchNorm buffers advanced
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1, k
        elif k.endswith("running_mean"):
            assert not np.array_equal(v, before[k]), k
    want1 = single_step(singles[1], reps[1])
    same(got[1]["logits"], want1["logits"], "replica 1 logits")
    for k, v in want1["buffers"].items():
        same(after[k], v, f"replica 1 buffer {k}")
    for k in (0, 2):
        same_step(got[k], single_step(singles[k], reps[k]), f"replica {k}")


def test_group_module_lets_a_replica_sit_out():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTMGroup
    D, C, H, act, shapes = 16, 32, 64, "silu", [(3, 21), (2, 30), (4, 16)]
    reps = make_group(D, C, H, act, shapes, 3200)
    singles = [copy.deepcopy(r["model"]) for r in reps]
    g = CNNLSTMGroup([r["model"] for r in reps]).train()
    for r in reps:
        r["model"].forced_masks = device_masks(r["masks"])
    before = state_of(reps[1]["model"])["buffers"]
    xs = [torch.from_numpy(r["x"]).to("cuda") for r in reps]
    outs = g([xs[0], None, xs[2]])
    assert outs[1] is None
    ce = torch.nn.CrossEntropyLoss()
    (ce(outs[0], torch.from_numpy(reps[0]["labels"]).cuda()) + ce(outs[2], torch.from_numpy(reps[2]["labels"]).cuda())).backward()
    torch.cuda.synchronize()
    st1 = state_of(reps[1]["model"])
    for k, v in before.items():
        same(st1["buffers"][k], v, f"replica 1 buffer {k} (sat out)")
    assert all(v is None for v in st1["grads"].values())
    for k in (0, 2):
        want = single_step(singles[k], reps[k])
        st = state_of(reps[k]["model"])
        same(outs[k].detach().cpu().numpy(), want["logits"], f"replica {k} logits")
        for key, v in want["grads"].items():
            same(st["grads"][key], v, f"replica {k} grad {key}")
        for key, v in want["buffers"].items():
            same(st["buffers"][key], v, f"replica {k} buffer {key}")


def test_second_backward_is_refused():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_group
    reps = make_group(16, 32, 64, "silu", [(2, 8), (3, 10)], 3300)
    outs = cnnlstm_train_group([r["model"] for r in reps], [torch.from_numpy(r["x"]).cuda() for r in reps])
    (outs[0].sum() + outs[1].sum()).backward(retain_graph=True)
    with pytest.raises(RuntimeError):
        (outs[0].sum() + outs[1].sum()).backward()


def test_lockstep_training_equals_sequential_trainings():
    """The reference's inner loop for three replicas over loaders of 5, 3 and 4 batches, 2 epochs, one Adam each, with
    every dropout probability 0 (no RNG involved), against three sequential runs of that loop on copies."""
    import torch
    from torch.utils.data import DataLoader
    from robust_speech_analysis_framework_amd.cnnlstm import collate_zero_pad, train_replicas_lockstep
    D, C, H, act, lr, epochs = 16, 32, 64, "silu", 1e-3, 2

    def collate(batch):
        return collate_zero_pad([b[0] for b in batch], device="cpu"), torch.tensor([b[1] for b in batch], dtype=torch.long)

    models, loaders = [], []
    for k, n_seq in enumerate((19, 12, 14)):                        # batch 4 -> 5, 3 and 4 batches (two of them ragged)
        m, _ = build(D, C, H, 4100 + k, act, p_rate=0.0, p_block=0.0)
        models.append(m)
        rng = np.random.Generator(np.random.PCG64(4200 + k))
        data = [(synth_input(1, int(rng.integers(10, 31)), D, 4300 + 100 * k + i)[0], int(rng.integers(0, 2))) for i in range(n_seq)]
        loaders.append(DataLoader(data, batch_size=4, shuffle=False, collate_fn=collate))
    assert [len(ld) for ld in loaders] == [5, 3, 4]
    copies = [copy.deepcopy(m) for m in models]
    loss_fn = torch.nn.CrossEntropyLoss()

    hist = train_replicas_lockstep(models, [torch.optim.Adam(m.parameters(), lr=lr) for m in models], loaders, loss_fn, epochs, "cuda")

    for k, (m, ld) in enumerate(zip(copies, loaders)):
        opt = torch.optim.Adam(m.parameters(), lr=lr)
        want = []
        for _ in range(epochs):                                      # src/dl_cv_strategies.py:117-129,244-248
            m.train()
            train_loss = 0
            for seq, lab in ld:
                seq, lab = seq.to("cuda"), lab.to("cuda")
                opt.zero_grad()
                out = m(seq)
                loss = loss_fn(out, lab)
                loss.backward()
                opt.step()
                train_loss += loss.item()
            want.append(train_loss / len(ld))
        assert hist[k] == want, (k, hist[k], want)
        got_sd, want_sd = models[k].state_dict(), m.state_dict()
        assert list(got_sd) == list(want_sd)
        for key, v in want_sd.items():
            same(got_sd[key].cpu().numpy(), v.cpu().numpy(), f"replica {k} {key}")


def test_group_above_the_four_row_threshold_in_a_subprocess():
    """With RSAF_LSTM_SMALL_MAX=0 (read once per process) every batch is above the 4-row threshold: the group entries run
    the recurrences per replica through the 16-row kernels, and the step still equals the single steps bit for bit."""
    import subprocess
    code = r'''
import sys
sys.path.insert(0, "tests")
import test_cnnlstm_train_group_gpu as t
t.group_equals_singles(24, 64, 128, "gelu", [(2, 40), (19, 12)], 5100)
t.group_equals_singles(16, 48, 64, "silu", [(5, 13), (2, 9)], 5200, num_classes=5, layers=3)    # row 2 of tests/cnnlstm_geometry.py
print("GROUP_SIXTEEN_ROW_OK")
'''
    env = dict(os.environ, RSAF_LSTM_SMALL_MAX="0")
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GROUP_SIXTEEN_ROW_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_group_module_in_eval_mode_and_state_dict_slices():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import CNNLSTM, CNNLSTMGroup
    D, C, H, act, shapes = 16, 32, 64, "silu", [(3, 21), (2, 30), (4, 16)]
    reps = make_group(D, C, H, act, shapes, 6100)
    g = CNNLSTMGroup([r["model"] for r in reps]).eval()
    xs = [torch.from_numpy(r["x"]).to("cuda") for r in reps]
    outs = g(xs)
    for k, r in enumerate(reps):
        same(outs[k].cpu().numpy(), r["model"](xs[k]).cpu().numpy(), f"replica {k} eval logits")
    assert g([xs[0], None, None])[1:] == [None, None]
    sd = g.state_dict()
    fresh = CNNLSTM(input_dim=D, cnn_out_channels=C, lstm_hidden_dim=H, activation_fn=act).to("cuda").eval()
    fresh.load_state_dict({k[len("models.1."):]: v for k, v in sd.items() if k.startswith("models.1.")})
    same(fresh(xs[1]).cpu().numpy(), outs[1].cpu().numpy(), "replica 1 through its state_dict slice")
