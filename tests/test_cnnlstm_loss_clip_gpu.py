"""Class weights and gradient-norm clipping in the fused CNN-LSTM step on the MI355X: rsaf_ce_loss_weighted_group,
rsaf_cnnlstm_grad_norm_group and rsaf_cnnlstm_adam_scaled_group through ce_loss_group(weights=), FusedAdam(max_grad_norm=),
cnnlstm_train_step_group(class_weights=) and the lockstep loops.

Bars.  Weighted cross-entropy against float64 (tests/loss_clip_restatement.py): the loss within 4 * 2^-23 * max(1, max|logit|),
as the unweighted kernel (a weighted mean of the same terms); the gradient of the logits within 4 * 2^-23 * max(w) / sum_b w[y_b],
the size of its largest possible entry.  Norm and scale: summed in double and rounded once, so within 2^-23 of themselves.
Clipped Adam on prescribed gradients: twice the largest deviation of clip_grad_norm_ + torch.optim.Adam on the same tensor plus
one ulp (the behaviour being replaced sets the bar).  Whole steps and loops against that path: rtol 2e-4, atol 2e-5 on the
losses, the bar of tests/test_cnnlstm_fused_step_gpu.py.  Everything that compares the kernels with themselves (group against
single, NULL weights, no clipping) is bit for bit."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from weights import synth_input  # noqa: E402
from cnnlstm_support import (  # noqa: E402
    GEOMETRIES, RAGGED, ULP, ZERO_GRAD, adam_bar, bits,
    build, freeze_zero_grad, gradient_blob, launches, lockstep_setup, same, unpacked)
from loss_clip_restatement import clip_scale, clipped_adam_step, grad_norm, weighted_cross_entropy  # noqa: E402

pytestmark = pytest.mark.gpu


def state_bits(model, opt):
    """Parameters and moments of a replica, for bit-for-bit comparisons."""
    out = {}
    for k, p in model.named_parameters():
        out[k] = bits(p)
        st = opt.state.get(p) or {}
        for key in ("exp_avg", "exp_avg_sq"):
            if key in st:
                out[f"{k}.{key}"] = bits(st[key])
    return out


def same_state(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        same(a[k], b[k], f"{what}: {k}")


# ---- 1. weighted cross-entropy against float64 ---------------------------------------------------------------------------------
def ce_items(nc, seed):
    """(logits, labels, weights): B = 1, 4, 7, 300, the last class at weight 0 and carried by some rows of every item of
    B > 1; the 7-row item holds +80 and -80 in one row and a row of equal logits."""
    rng = np.random.Generator(np.random.PCG64(seed))
    items = []
    for B, scale in ((1, 1.0), (4, 30.0), (7, 80.0), (300, 30.0)):
        x = (rng.uniform(-1, 1, (B, nc)) * scale).astype(np.float32)
        if B == 7:
            x[0, 0], x[0, -1] = 80.0, -80.0
            x[3, :] = 12.5
        w = rng.uniform(0.1, 5.0, nc).astype(np.float32)
        w[nc - 1] = 0.0
        y = rng.integers(0, nc, B)
        y[0] = rng.integers(0, nc - 1)
        if B > 1:
            y[1] = nc - 1
        items.append((x, y, w))
    return items


@pytest.mark.parametrize("nc", [2, 3, 16])
def test_weighted_cross_entropy_against_float64(nc):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import ce_loss_group
    items = ce_items(nc, 2100 + nc)
    plain = np.random.Generator(np.random.PCG64(2150 + nc))
    items.append(((plain.uniform(-1, 1, (4, nc)) * 30).astype(np.float32), plain.integers(0, nc, 4), None))    # NULL weights
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()                 # noqa: E731
    logits, labels, weights = ([dev(it[j]) for it in items] for j in range(3))
    losses, dl = ce_loss_group(logits, labels, weights=weights)
    losses_only, none = ce_loss_group(logits, labels, with_grad=False, weights=weights)
    plain_loss, plain_dl = ce_loss_group(logits[-1:], labels[-1:])
    torch.cuda.synchronize()
    assert none is None and losses.shape == (len(items),)
    same(bits(losses_only), bits(losses), "loss without dlogits")
    same(bits(losses[-1:]), bits(plain_loss), "item without weights: loss against rsaf_ce_loss_group")
    same(bits(dl[-1]), bits(plain_dl[0]), "item without weights: dlogits against rsaf_ce_loss_group")
    for k, (x, y, w) in enumerate(items[:-1]):
        assert (y == nc - 1).any() or len(y) == 1
        assert (y != nc - 1).any()
        want_loss, want_dl = weighted_cross_entropy(x, y, w)
        err = abs(float(losses[k]) - want_loss)
        derr = np.abs(dl[k].cpu().numpy().astype(np.float64) - want_dl).max()
        wsum = float(w.astype(np.float64)[y].sum())
        print(f"nc={nc} item {k} B={len(y)}: loss err {err:.3e}, dlogits err {derr:.3e}, bar {4 * ULP * float(w.max()) / wsum:.3e}")
        assert err <= 4 * ULP * max(1.0, np.abs(x).max()), (k, err)
        assert derr <= 4 * ULP * float(w.max()) / wsum, (k, derr)


def test_weighted_cross_entropy_nan_cases():
    """A label outside [0, nc) and an item whose rows all carry the zero-weight class give a NaN loss; their neighbours in
    the call are untouched."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import ce_loss_group
    nc = 3
    rng = np.random.Generator(np.random.PCG64(2200))
    x = [torch.from_numpy(rng.uniform(-2, 2, (4, nc)).astype(np.float32)).cuda() for _ in range(4)]
    w = torch.tensor([0.5, 2.0, 0.0]).cuda()
    y = [torch.tensor(v).cuda() for v in ([0, 1, 3, 1], [0, -1, 1, 1], [2, 2, 2, 2], [0, 1, 2, 1])]
    losses, _ = ce_loss_group(x, y, weights=[w] * 4)
    got = losses.tolist()
    assert np.isnan(got[0]) and np.isnan(got[1]) and np.isnan(got[2]), got
    want = weighted_cross_entropy(x[3].cpu().numpy(), np.array([0, 1, 2, 1]), w.cpu().numpy())[0]
    assert abs(got[3] - want) <= 4 * ULP * 2.0, (got[3], want)


# ---- 2. chunking ------------------------------------------------------------------------------------------------------------------
def test_weighted_cross_entropy_group_longer_than_the_chunk():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import ce_loss_group, train_group_max
    nc, K = 3, train_group_max() + 1
    rng = np.random.Generator(np.random.PCG64(2300))
    logits = [torch.from_numpy((rng.uniform(-1, 1, (1 + k % 3, nc)) * (1.0 + 3.0 * k)).astype(np.float32)).cuda() for k in range(K)]
    labels = [torch.from_numpy(rng.integers(0, nc, 1 + k % 3)).cuda() for k in range(K)]
    weights = [torch.from_numpy(rng.uniform(0.1, 5.0, nc).astype(np.float32)).cuda() for _ in range(K)]
    losses, dl = ce_loss_group(logits, labels, weights=weights)
    assert losses.shape == (K,) and len(dl) == K
    for k in range(K):
        own_loss, own_dl = ce_loss_group(logits[k:k + 1], labels[k:k + 1], weights=weights[k:k + 1])
        same(bits(losses[k:k + 1]), bits(own_loss), f"loss of item {k} against a call of its own")
        same(bits(dl[k]), bits(own_dl[0]), f"dlogits of item {k} against a call of its own")


# ---- 3. the norm on prescribed gradient blobs ---------------------------------------------------------------------------------
def norm_of(opt, gb, skip=None, table=None):
    """(norm, scale) as float32 bit patterns, through rsaf_cnnlstm_grad_norm_group alone."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm_fused import _grad_norm_group
    skip = opt._frozen() if skip is None else skip
    _grad_norm_group([(opt, gb, table if table is not None else opt._cached_table(), skip)])
    torch.cuda.synchronize()
    return bits(opt.last_grad_norm), bits(opt.last_grad_scale)


def as_float(b):
    return float(np.asarray(b).view(np.float32))


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_grad_norm_on_prescribed_blobs(geom):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, _train_segments, train_param_offsets
    from robust_speech_analysis_framework_amd.cnnlstm_fused import _pointer_table
    D, C, H, act, NC, L = GEOMETRIES[geom]
    m, _ = build(D, C, H, 2401, act, num_classes=NC, layers=L)
    opt = FusedAdam(m, max_grad_norm=1.0)
    total = train_param_offsets(m.dims)[1]
    rng = np.random.Generator(np.random.PCG64(2402))
    gb = torch.from_numpy(gradient_blob(rng, total, rng.random(total) < 0.1)).cuda()
    grads = unpacked(m, gb)
    g64 = {k: g.cpu().numpy().astype(np.float64) for k, g in grads.items()}
    named = dict(m.named_parameters())

    def check(what):
        live = {k: g for k, g in g64.items() if named[k].requires_grad}
        want = grad_norm(live)
        opt.max_grad_norm = 1e-2 * want                           # the clipping regime
        norm, scale = norm_of(opt, gb)
        want_scale = clip_scale(want, opt.max_grad_norm)
        print(f"{geom} {what}: norm {as_float(norm)!r} float64 {want!r}, scale {as_float(scale)!r} float64 {want_scale!r}")
        assert abs(as_float(norm) - want) <= ULP * want, (what, as_float(norm), want)
        assert abs(as_float(scale) - want_scale) <= ULP * want_scale, (what, as_float(scale), want_scale)
        return norm, scale, want

    norm_all, scale_all, want_all = check("all parameters")
    same(np.r_[norm_of(opt, gb)], np.r_[norm_all, scale_all], "a second run of the same call")
    # the .grad source: the fourth table row on the same gradients
    names = {id(p): k for k, p in m.named_parameters()}
    keep = [grads[names[id(p)]].contiguous() for p in opt._order]              # in the kernels' parameter numbering
    table = _pointer_table(opt._rows() + [[g.data_ptr() for g in keep]], "cuda")
    same(np.r_[norm_of(opt, None, table=table)], np.r_[norm_all, scale_all], ".grad source against the blob source")
    # parameters without a gradient, as FusedAdam.step() skips them
    skip = sum(1 << i for i, p in enumerate(opt._order) if names[id(p)].endswith(ZERO_GRAD))
    rows = opt._rows() + [[0 if (skip >> i) & 1 else g.data_ptr() for i, g in enumerate(keep)]]
    n_skip, _ = norm_of(opt, None, skip=skip, table=_pointer_table(rows, "cuda"))
    # frozen parameters are left out of the norm
    freeze_zero_grad(m)
    norm_frozen, _, want_frozen = check("ZERO_GRAD frozen")
    assert want_frozen < want_all
    same(n_skip, norm_frozen, "skipped through the .grad source against frozen through the blob source")
    # one bias of a pair frozen: its segment counts once
    named["lstm.bias_hh_l0"].requires_grad_(False)
    _, _, want_one = check("bias_hh_l0 frozen too")
    assert want_one < want_frozen
    named["lstm.bias_ih_l0"].requires_grad_(False)
    check("both biases of l0 frozen")
    for p in m.parameters():
        p.requires_grad_(True)
    # known answer: 1.0 on every b_ih + b_hh segment of the blob, 0 elsewhere
    segs, _ = _train_segments(m)
    ones = np.zeros(total, np.float32)
    n_bias = 0
    for off, nfl, _, outs in segs:
        if len(outs) == 4:                                          # the bias segment of a layer: both directions, two parameters each
            ones[off:off + nfl] = 1.0
            n_bias += nfl
    assert n_bias == 8 * H * L
    opt.max_grad_norm = float("inf")
    norm, scale = norm_of(opt, torch.from_numpy(ones).cuda())
    same(norm, bits(torch.tensor(np.float32(np.sqrt(16.0 * H * L)))), "norm of the unit bias blob")
    assert as_float(scale) == 1.0


# ---- 4. clipped Adam on prescribed gradients ----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["shortcut_conv_silu", "geometry3_h128_l4_nc16"])
def test_clipped_adam_on_prescribed_gradients(geom):
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_param_offsets
    D, C, H, act, NC, L = GEOMETRIES[geom]
    lr = 1e-3
    m, sd = build(D, C, H, 2501, act, num_classes=NC, layers=L)
    ref, plain, big, inf = (copy.deepcopy(m) for _ in range(4))
    opt, topt = FusedAdam(m, lr=lr, max_grad_norm=1.0), torch.optim.Adam(ref.parameters(), lr=lr)
    others = [(plain, FusedAdam(plain, lr=lr)), (big, FusedAdam(big, lr=lr, max_grad_norm=1e9)),
              (inf, FusedAdam(inf, lr=lr, max_grad_norm=float("inf")))]
    total = train_param_offsets(m.dims)[1]
    rng = np.random.Generator(np.random.PCG64(2502))
    zero = rng.random(total) < 0.1
    oracle = {k: np.asarray(v, np.float64) for k, v in sd.items() if k in dict(m.named_parameters())}
    state = {}
    for it in range(3):
        gb = torch.from_numpy(gradient_blob(rng, total, zero)).cuda()
        grads = unpacked(ref, gb)
        g64 = {k: g.cpu().numpy().astype(np.float64) for k, g in grads.items()}
        max_norm = 1e-2 * grad_norm(g64)
        opt.max_grad_norm = max_norm
        opt.step_blob(gb)
        for k, p in ref.named_parameters():
            p.grad = grads[k].clone()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
        topt.step()
        norm, scale = clipped_adam_step(oracle, g64, state, lr, max_norm)
        for _, o in others:
            o.step_blob(gb)
        torch.cuda.synchronize()
        assert abs(float(opt.last_grad_norm) - norm) <= ULP * norm and abs(float(opt.last_grad_scale) - scale) <= ULP * scale
        assert scale < 0.011
        rp = dict(ref.named_parameters())
        for k, p in m.named_parameters():
            adam_bar(p.detach().cpu().numpy(), rp[k].detach().cpu().numpy(), oracle[k], f"{geom} step {it} {k}")
        assert abs(float(others[1][1].last_grad_norm) - norm) <= ULP * norm and float(others[1][1].last_grad_scale) == 1.0
        assert abs(float(others[2][1].last_grad_norm) - norm) <= ULP * norm and float(others[2][1].last_grad_scale) == 1.0
    want = state_bits(*others[0])
    same_state(state_bits(*others[1]), want, f"{geom}: max_grad_norm 1e9 against no clipping")
    same_state(state_bits(*others[2]), want, f"{geom}: max_grad_norm inf against no clipping")
    # an all-zero blob from a fresh state: every bit stays, nothing is NaN
    z, _ = build(D, C, H, 2503, act, num_classes=NC, layers=L)
    zopt = FusedAdam(z, lr=lr, max_grad_norm=0.5)
    before = {k: bits(p) for k, p in z.named_parameters()}
    zopt.step_blob(torch.zeros(total, device="cuda"))
    torch.cuda.synchronize()
    assert float(zopt.last_grad_norm) == 0.0 and float(zopt.last_grad_scale) == 1.0
    for k, p in z.named_parameters():
        same(bits(p), before[k], f"{geom} {k}: zero gradient")
        assert torch.isfinite(zopt.state[p]["exp_avg"]).all() and torch.isfinite(zopt.state[p]["exp_avg_sq"]).all()
        assert not zopt.state[p]["exp_avg"].any() and not zopt.state[p]["exp_avg_sq"].any()


# ---- 5. the whole step against the path it replaces ------------------------------------------------------------------------------
def torch_step(model, topt, x, y, weight, max_norm):
    """cnnlstm_train_group + CrossEntropyLoss(weight) + clip_grad_norm_ + torch.optim.Adam -> (loss, norm)."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import cnnlstm_train_group
    topt.zero_grad()
    loss = torch.nn.CrossEntropyLoss(weight=weight)(cnnlstm_train_group([model], [x])[0], y)
    loss.backward()
    norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
    topt.step()
    return loss.item(), norm.item()


def test_whole_step_against_the_autograd_path():
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, cnnlstm_train_step_group
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    lr, steps, K = 1e-3, 3, 2
    models = [build(D, C, H, 2601 + k, act)[0] for k in range(K)]
    for m in models:
        freeze_zero_grad(m)
    refs = [copy.deepcopy(m) for m in models]
    weights = [torch.tensor(w).cuda() for w in ([0.3, 2.5], [4.0, 0.7])]
    xs = [[torch.from_numpy(synth_input(4, 24, D, 2610 + 10 * k + it)).cuda() for k in range(K)] for it in range(steps)]
    ys = [[torch.tensor(v).cuda() for v in ([0, 1, 1, 0], [1, 1, 0, 1])] for _ in range(steps)]
    # half the norm of the first step's gradient: that step clips
    probe = [copy.deepcopy(m) for m in models]
    first = [torch_step(p, torch.optim.Adam(p.parameters(), lr=lr), xs[0][k], ys[0][k], weights[k], float("inf"))[1] for k, p in enumerate(probe)]
    max_norms = [0.5 * n for n in first]
    opts = [FusedAdam(m, lr=lr, max_grad_norm=mx) for m, mx in zip(models, max_norms)]
    topts = [torch.optim.Adam(r.parameters(), lr=lr) for r in refs]
    got, want, scales = [], [], []
    for it in range(steps):
        res = [torch_step(refs[k], topts[k], xs[it][k], ys[it][k], weights[k], max_norms[k]) for k in range(K)]
        want.append([r[0] for r in res])
        ls, _ = cnnlstm_train_step_group(models, opts, xs[it], ys[it], class_weights=weights)
        got.append(ls.tolist())
        print(f"step {it}: norms fused {[float(o.last_grad_norm) for o in opts]} torch {[r[1] for r in res]}")
        scales.append([float(o.last_grad_scale) for o in opts])
    print(f"losses fused {got} torch {want}; scales {scales}")
    assert all(s < 1.0 for s in scales[0]), scales                  # max_grad_norm is half the first step's norm
    assert np.allclose(got, want, rtol=2e-4, atol=2e-5), (got, want)
    assert all(p.grad is None for m in models for p in m.parameters())


# ---- 6. group against single, bit for bit -------------------------------------------------------------------------------------
def group_against_single(archs, mixed, seed):
    """K = 3 replicas on the RAGGED shapes with different class weights and one max_grad_norm that clips some replicas
    and not others: the group step against one call per replica (``mixed``: per architecture) on deep copies."""
    import torch
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, cnnlstm_train_step_group
    lr, steps = 1e-3, 2
    D = archs[0][0]
    models = [build(D, C, H, seed + k, act)[0] for k, (_, C, H, act) in enumerate(archs)]
    for m in models:
        freeze_zero_grad(m)
    weights = [torch.tensor(w).cuda() for w in ([0.3, 2.5], [4.0, 0.7], [1.0, 0.0])]
    xs = [[torch.from_numpy(synth_input(B, T, D, seed + 10 + 10 * k + it)).cuda() for k, (B, T) in enumerate(RAGGED)] for it in range(steps)]
    ys = [[(torch.arange(B) + k + it).cuda() % 2 for k, (B, _) in enumerate(RAGGED)] for it in range(steps)]
    # the norms of the first step, from a step on copies that clips nothing
    probe = [copy.deepcopy(m) for m in models]
    popts = [FusedAdam(p, lr=lr, max_grad_norm=float("inf")) for p in probe]
    cnnlstm_train_step_group(probe, popts, xs[0], ys[0], class_weights=weights, mixed=mixed)
    norms = sorted(float(o.last_grad_norm) for o in popts)
    max_norm = 0.5 * (norms[0] + norms[1])
    assert norms[0] < max_norm < norms[1], norms

    singles = [copy.deepcopy(m) for m in models]
    opts = [FusedAdam(m, lr=lr, max_grad_norm=max_norm) for m in models]
    sopts = [FusedAdam(m, lr=lr, max_grad_norm=max_norm) for m in singles]
    if mixed:                                                    # one call per architecture
        calls = {}
        for k, a in enumerate(archs):
            calls.setdefault(a, []).append(k)
        calls = list(calls.values())
        assert 1 < len(calls) < len(archs)
    else:
        calls = [[k] for k in range(len(archs))]
    for it in range(steps):
        ls, logits = cnnlstm_train_step_group(models, opts, xs[it], ys[it], class_weights=weights, mixed=mixed)
        group = (bits(ls), [bits(o.last_grad_norm) for o in opts], [bits(o.last_grad_scale) for o in opts])
        if it == 0:
            sc = [float(o.last_grad_scale) for o in opts]
            print(f"mixed={mixed}: first-step norms {norms}, max_grad_norm {max_norm}, scales {sc}")
            assert any(s < 1.0 for s in sc) and any(s == 1.0 for s in sc), sc
        for idx in calls:
            sl, slog = cnnlstm_train_step_group([singles[k] for k in idx], [sopts[k] for k in idx], [xs[it][k] for k in idx],
                                                [ys[it][k] for k in idx], class_weights=[weights[k] for k in idx])
            for j, k in enumerate(idx):
                same(group[0][k:k + 1], bits(sl[j:j + 1]), f"step {it} replica {k}: loss")
                same(bits(logits[k]), bits(slog[j]), f"step {it} replica {k}: logits")
                same(group[1][k], bits(sopts[k].last_grad_norm), f"step {it} replica {k}: norm")
                same(group[2][k], bits(sopts[k].last_grad_scale), f"step {it} replica {k}: scale")
    for k in range(len(archs)):
        same_state(state_bits(models[k], opts[k]), state_bits(singles[k], sopts[k]), f"replica {k}")


def test_group_step_equals_single_steps_bit_for_bit():
    group_against_single([GEOMETRIES["shortcut_conv_silu"][:4]] * 3, False, 2700)


def test_mixed_group_step_equals_one_step_per_architecture_bit_for_bit():
    a, b = (16, 32, 64, "silu"), (16, 48, 128, "gelu")
    group_against_single([a, b, a], True, 2800)


# ---- 7. the lockstep loops ------------------------------------------------------------------------------------------------------
FOLD_WEIGHTS = ([0.4, 2.2], [3.0, 0.8], [1.0, 1.7])
MAX_NORM = 1e-2


def clipped_torch_adam(params, lr, max_norm):
    """torch.optim.Adam whose step() is preceded by clip_grad_norm_, as the reference's loop would call the two."""
    import torch

    class ClippedAdam(torch.optim.Adam):
        def step(self, closure=None):
            torch.nn.utils.clip_grad_norm_([p for g in self.param_groups for p in g["params"]], max_norm)
            return super().step(closure)

    return ClippedAdam(params, lr=lr)


def test_lockstep_with_fold_weights_and_clipping_takes_the_fused_step():
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_replicas_lockstep
    lr, epochs = 1e-3, 2
    loss_fns = [torch.nn.CrossEntropyLoss(weight=torch.tensor(w).cuda()) for w in FOLD_WEIGHTS]
    models, opts, loaders = lockstep_setup(2900, lambda k, m: FusedAdam(m, lr=lr, max_grad_norm=MAX_NORM))
    _lib.prof_begin()
    hist = train_replicas_lockstep(models, opts, loaders, loss_fns, epochs, "cuda")
    prof = _lib.prof_end()
    group_steps = epochs * max(len(ld) for ld in loaders)
    for family in ("train_adam", "train_ce", "train_pack", "train_bn_running"):
        assert launches(prof, family) == group_steps, (family, prof.get(family))
    assert group_steps <= launches(prof, "train_grad_norm") <= 2 * group_steps, prof.get("train_grad_norm")
    scales = [float(o.last_grad_scale) for o in opts]
    assert all(s < 1.0 for s in scales), scales                     # the test clips
    models_t, opts_t, loaders_t = lockstep_setup(2900, lambda k, m: clipped_torch_adam(m.parameters(), lr, MAX_NORM))
    _lib.prof_begin()
    want = train_replicas_lockstep(models_t, opts_t, loaders_t, loss_fns, epochs, "cuda")
    prof_t = _lib.prof_end()
    assert launches(prof_t, "train_ce") == 0 and launches(prof_t, "train_grad_norm") == 0
    print("lockstep histories fused", hist, "torch", want, "last scales", scales)
    assert np.allclose(hist, want, rtol=2e-4, atol=2e-5), (hist, want)


def test_autograd_gradients_of_a_bias_pair_do_not_share_memory():
    """b_ih and b_hh of a direction receive the gradient of one run of the blob.  Through autograd each `.grad` must own its
    floats: clip_grad_norm_ multiplies `.grad` in place, and on shared floats the pair would be scaled twice (the comparisons
    against clip_grad_norm_ + torch.optim.Adam in this file lean on that)."""
    import torch
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    m, _ = build(D, C, H, 2950, act)
    x = torch.from_numpy(synth_input(4, 24, D, 2951)).cuda()
    torch.nn.CrossEntropyLoss()(m(x), torch.tensor([0, 1, 1, 0]).cuda()).backward()
    grads = [p.grad for p in m.parameters()]
    assert len({g.data_ptr() for g in grads}) == len(grads)
    a, b = m.lstm.bias_ih_l0.grad, m.lstm.bias_hh_l0.grad
    same(bits(a), bits(b), "the two biases of a direction hold the same gradient")
    before = a.clone()
    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), 0.25).item()
    scale = np.float32(0.25) / (np.float32(norm) + np.float32(1e-6))
    assert scale < 1.0
    for g in (a, b):                                                 # scaled once each (torch's float32 product, to an ulp of slack)
        assert np.abs(g.cpu().numpy() - before.cpu().numpy() * scale).max() <= 2 * ULP * float(before.abs().max()) * scale


def test_lockstep_autograd_loop_clips_in_fused_adam_step():
    """Label smoothing keeps the autograd loop; FusedAdam.step() does the clipping there and leaves .grad alone."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_replicas_lockstep
    lr = 1e-3
    loss_fns = [torch.nn.CrossEntropyLoss(weight=torch.tensor(w).cuda(), label_smoothing=0.1) for w in FOLD_WEIGHTS]
    models, opts, loaders = lockstep_setup(3000, lambda k, m: FusedAdam(m, lr=lr, max_grad_norm=MAX_NORM))
    _lib.prof_begin()
    hist = train_replicas_lockstep(models, opts, loaders, loss_fns, 1, "cuda")
    prof = _lib.prof_end()
    steps = sum(len(ld) for ld in loaders)
    assert launches(prof, "train_ce") == 0 and launches(prof, "train_adam") == launches(prof, "train_grad_norm") == steps
    for m, o in zip(models, opts):                                  # the norm of the .grad tensors, which nothing scaled
        n = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None)).item()
        assert abs(float(o.last_grad_norm) - n) <= 2 * ULP * n, (float(o.last_grad_norm), n)
        assert float(o.last_grad_scale) < 1.0
    models_t, opts_t, loaders_t = lockstep_setup(3000, lambda k, m: clipped_torch_adam(m.parameters(), lr, MAX_NORM))
    want = train_replicas_lockstep(models_t, opts_t, loaders_t, loss_fns, 1, "cuda")
    assert np.allclose(hist, want, rtol=2e-4, atol=2e-5), (hist, want)


@pytest.mark.parametrize("case", ["cpu_weight", "float64_weight"])
def test_lockstep_keeps_the_autograd_loop_for_a_weight_the_kernel_cannot_read(case):
    """A weight on the CPU or in float64 is not the fused step's: the decision says so, and the loop that runs is the
    autograd one with torch's own loss (which may refuse such a weight itself); no launch of the loss kernel either way."""
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_replicas_lockstep
    from robust_speech_analysis_framework_amd.cnnlstm_fused import _fused_step_applies
    w = torch.tensor(FOLD_WEIGHTS[0]) if case == "cpu_weight" else torch.tensor(FOLD_WEIGHTS[0], dtype=torch.float64).cuda()
    good = torch.nn.CrossEntropyLoss(weight=torch.tensor(FOLD_WEIGHTS[1]).cuda())
    loss_fns = [good, torch.nn.CrossEntropyLoss(weight=w), good]
    models, opts, loaders = lockstep_setup(3100, lambda k, m: FusedAdam(m, lr=1e-3))
    assert _fused_step_applies(opts, models, [good] * 3) and _fused_step_applies(opts, models, good)
    assert not _fused_step_applies(opts, models, loss_fns)
    _lib.prof_begin()
    try:
        train_replicas_lockstep(models, opts, loaders, loss_fns, 1, "cuda")
    except RuntimeError as e:                                        # torch's cross_entropy on logits of another device or dtype
        print(f"{case}: torch refused the weight: {e}")
    prof = _lib.prof_end()
    assert launches(prof, "train_ce") == 0 and launches(prof, "train_pack") == 0


def test_train_eval_lockstep_validates_with_the_replicas_weights():
    import torch
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm import FusedAdam, train_eval_replicas_lockstep
    epochs, patience = 2, 2
    loss_fns = [torch.nn.CrossEntropyLoss(weight=torch.tensor(w).cuda()) for w in FOLD_WEIGHTS]
    models, opts, loaders = lockstep_setup(3200, lambda k, m: FusedAdam(m, lr=1e-3, max_grad_norm=MAX_NORM))
    _, _, val_loaders = lockstep_setup(3250, lambda k, m: None, shuffle=False)
    _lib.prof_begin()
    res = train_eval_replicas_lockstep(models, opts, [None] * 3, loaders, val_loaders, loss_fns, epochs, patience, "cuda")
    prof = _lib.prof_end()
    assert launches(prof, "train_ce") > launches(prof, "train_adam") > 0            # + the validation passes
    for k, (m, th, vh) in enumerate(res):
        assert len(th) == len(vh) == epochs and np.isfinite(th).all() and np.isfinite(vh).all()
        # the model holds its best weights: its weighted validation loss, in float64 on the same logits, is the best of the history
        m.eval()
        tot, n, big = 0.0, 0, 1.0
        with torch.no_grad():
            for seq, lab in val_loaders[k]:
                out = m(seq.cuda()).cpu().numpy()
                tot += weighted_cross_entropy(out, lab.numpy(), np.asarray(FOLD_WEIGHTS[k], np.float32))[0]
                big = max(big, float(np.abs(out).max()))
                n += 1
        print(f"replica {k}: validation history {vh}, float64 weighted loss of the best weights {tot / n}")
        assert abs(tot / n - min(vh)) <= 4 * ULP * big, (k, tot / n, vh)
