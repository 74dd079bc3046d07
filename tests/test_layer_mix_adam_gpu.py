"""``rsaf_layer_mix_adam_group`` on the MI355X: the step of a mix's L weights (softmax Jacobian in double, published Adam, the
softmax of the new weights), and ``FusedAdam(layer_mix=...)`` on top of it.

Bars.  Weights and moments against a float64 restatement (Jacobian p (dp - p . dp) and ``cnnlstm_train_oracle.adam_step`` in
float64 from the float32 p and dp) under ``cnnlstm_support.adam_bar``, whose yardstick is ``torch.optim.Adam`` fed torch's own
softmax-Jacobian gradient of the same p and dp.  ``p_next`` within 2^-23 relative of the float64 softmax of the new float32
weights: one rounding to float (2^-24), a factor 2 of margin for the double exp and sum."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import input_grad_restatement as igr  # noqa: E402
from cnnlstm_support import GEOMETRIES, adam_bar, bits, build, same  # noqa: E402
from oracle import cnnlstm_train_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu

LR = 1e-2


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


class Weights:
    """w, exp_avg, exp_avg_sq, p_next and dw_out of one item on the device."""

    def __init__(self, w0):
        import torch
        self.w = dev(np.asarray(w0, np.float32))
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.p_next, self.dw_out = torch.full_like(self.w, -1.0), torch.full_like(self.w, -1.0)

    def all_bits(self):
        return [bits(t) for t in (self.w, self.m, self.v, self.p_next)]


def launch(records):
    """One ``rsaf_layer_mix_adam_group`` call: records of (Weights, mode, step, p, dp, dw)."""
    from robust_speech_analysis_framework_amd import _lib
    from robust_speech_analysis_framework_amd.cnnlstm_train import _launch_chunked

    def fill(it, rec, _k):
        s, mode, step, p, dp, dw = rec
        it.L, it.mode = s.w.numel(), mode
        it.p, it.dp, it.dw = _lib.optr(p), _lib.optr(dp), _lib.optr(dw)
        it.dw_out = s.dw_out.data_ptr() if mode == _lib.LAYER_MIX_FROM_DP else None
        it.w, it.exp_avg, it.exp_avg_sq, it.p_next = s.w.data_ptr(), s.m.data_ptr(), s.v.data_ptr(), s.p_next.data_ptr()
        it.lr, it.beta1, it.beta2, it.eps, it.step = LR, 0.9, 0.999, 1e-8, step

    _launch_chunked("rsaf_layer_mix_adam_group", _lib.LayerMixAdamItem, records, fill)


def sequences(L, seed, steps=5):
    """w0 [L] and per step (z, dp): p of the step is torch's softmax of z."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.uniform(-1.5, 1.5, L).astype(np.float32),
            [(rng.uniform(-2, 2, L).astype(np.float32), (10.0 ** rng.uniform(-4, 0, L) * rng.choice([-1.0, 1.0], L)).astype(np.float32))
             for _ in range(steps)])


@pytest.mark.parametrize("L", [3, 32])
def test_five_steps_against_float64(rsaf_lib, L):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    w0, seq = sequences(L, 29700 + L)
    s = Weights(w0)
    ref = torch.nn.Parameter(dev(w0))
    topt = torch.optim.Adam([ref], lr=LR)
    oracle, state = {"w": w0.astype(np.float64)}, {}
    for it, (z, dp) in enumerate(seq):
        zt = dev(z).requires_grad_(True)
        p = torch.softmax(zt, dim=0)
        p.backward(dev(dp))                                   # torch's own Jacobian of the same p and dp
        ref.grad = zt.grad.clone()
        topt.step()
        launch([(s, _lib.LAYER_MIX_FROM_DP, it + 1, p.detach().contiguous(), dev(dp), None)])
        torch.cuda.synchronize()
        p64, dp64 = p.detach().cpu().numpy().astype(np.float64), dp.astype(np.float64)
        dw64 = igr.softmax_jacobian_apply(p64, dp64)
        to.adam_step(oracle, {"w": dw64}, state, LR)
        got_dw = s.dw_out.cpu().numpy().astype(np.float64)
        assert (np.abs(got_dw - dw64) <= 2.0 ** -24 * np.abs(dw64) + 2 * L * 2.0 ** -53 * np.abs(p64 * dp64).sum()).all(), (it, got_dw, dw64)
        tst = topt.state[ref]
        adam_bar(s.w.cpu().numpy(), ref.detach().cpu().numpy(), oracle["w"], f"L {L} step {it} w")
        adam_bar(s.m.cpu().numpy(), tst["exp_avg"].cpu().numpy(), state["m"]["w"], f"L {L} step {it} exp_avg")
        adam_bar(s.v.cpu().numpy(), tst["exp_avg_sq"].cpu().numpy(), state["v"]["w"], f"L {L} step {it} exp_avg_sq")
        want_p = igr.softmax64(s.w.cpu().numpy())
        got_p = s.p_next.cpu().numpy().astype(np.float64)
        assert (np.abs(got_p - want_p) <= 2.0 ** -23 * want_p).all(), (it, np.abs(got_p / want_p - 1).max())
    assert not np.array_equal(bits(s.w), w0.view(np.uint32))


def test_softmax_only_mode(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    for L in (1, 3, 32):
        w0 = sequences(L, 29750 + L)[0]
        w0[0] = 60.0 if L > 1 else w0[0]                      # max-subtracted: no overflow next to a large weight
        s = Weights(w0)
        launch([(s, _lib.LAYER_MIX_SOFTMAX_ONLY, 0, None, None, None)])
        torch.cuda.synchronize()
        want = igr.softmax64(w0)
        got = s.p_next.cpu().numpy().astype(np.float64)
        tiny = want < 2.0 ** -126                             # below the normal floats the rounding is absolute
        assert (np.abs(got - want)[~tiny] <= 2.0 ** -23 * want[~tiny]).all() and (np.abs(got - want)[tiny] <= 2.0 ** -149).all()
        same(bits(s.w), w0.view(np.uint32), "w")
        assert not s.m.any() and not s.v.any()
    assert got[0] > 0.99


def test_one_layer_leaves_its_weight(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    s = Weights([0.37])
    for it, dp in enumerate((0.5, -3.0, 1e-3)):
        launch([(s, _lib.LAYER_MIX_FROM_DP, it + 1, dev(np.ones(1, np.float32)), dev(np.array([dp], np.float32)), None)])
    torch.cuda.synchronize()
    same(bits(s.w), np.array([0.37], np.float32).view(np.uint32), "w at L = 1")
    assert s.dw_out.item() == 0.0 and s.p_next.item() == 1.0


def test_dw_mode_equals_dp_mode_and_groups_equal_singles(rsaf_lib):
    import torch
    from robust_speech_analysis_framework_amd import _lib
    Ls = (3, 13, 32)
    runs = [sequences(L, 29800 + L, steps=3) for L in Ls]
    from_dp = [Weights(w0) for w0, _ in runs]
    from_dw = [Weights(w0) for w0, _ in runs]
    single = [Weights(w0) for w0, _ in runs]
    for it in range(3):
        ps = [torch.softmax(dev(seq[it][0]), dim=0) for _, seq in runs]
        dps = [dev(seq[it][1]) for _, seq in runs]
        launch([(s, _lib.LAYER_MIX_FROM_DP, it + 1, p, dp, None) for s, p, dp in zip(from_dp, ps, dps)])       # K = 3, one launch
        launch([(s, _lib.LAYER_MIX_FROM_DW, it + 1, None, None, t.dw_out.clone()) for s, t in zip(from_dw, from_dp)])
        for s, p, dp in zip(single, ps, dps):
            launch([(s, _lib.LAYER_MIX_FROM_DP, it + 1, p, dp, None)])
        torch.cuda.synchronize()
        for k, L in enumerate(Ls):
            for name, a, b, c in zip(("w", "exp_avg", "exp_avg_sq", "p_next"), from_dp[k].all_bits(), from_dw[k].all_bits(), single[k].all_bits()):
                same(b, a, f"L {L} step {it} {name}: dw mode against p / dp mode")
                same(c, a, f"L {L} step {it} {name}: three launches against one")


def test_fused_adam_owns_the_mix_and_interchanges_state_with_torch_adam(rsaf_lib):
    import torch
    from src.models import FusedAdam, LayerMix
    D, C, H, act = GEOMETRIES["shortcut_conv_silu"][:4]
    L = 5
    w0, seq = sequences(L, 29900, steps=4)

    def setup():
        m, _ = build(D, C, H, 29901, act)
        mix = LayerMix(L).cuda()
        with torch.no_grad():
            mix.weights.copy_(dev(w0))
        return m, mix

    def give_grads(m, mix, it):
        g = torch.Generator(device="cuda").manual_seed(29910 + it)
        for p in m.parameters():
            p.grad = 1e-2 * torch.randn(p.shape, device="cuda", generator=g)
        mix.weights.grad = dev(seq[it][1])

    m, mix = setup()
    rm, rmix = setup()
    opt = FusedAdam(m, lr=1e-3, layer_mix=mix, layer_mix_lr=LR)
    topt = torch.optim.Adam([{"params": rm.parameters()}, {"params": [rmix.weights], "lr": LR}], lr=1e-3)
    assert [g["lr"] for g in opt.param_groups] == [1e-3, LR] and opt.param_groups[1]["params"][0] is mix.weights
    assert FusedAdam(setup()[0], lr=2e-3, layer_mix=mix).param_groups[1]["lr"] == 2e-3        # None: the classifier's lr
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    tsched = torch.optim.lr_scheduler.StepLR(topt, step_size=1, gamma=0.5)
    oracle, state = {"w": w0.astype(np.float64)}, {}
    for it in range(2):
        give_grads(m, mix, it)
        give_grads(rm, rmix, it)
        opt.step()
        topt.step()
        to.adam_step(oracle, {"w": seq[it][1].astype(np.float64)}, state, LR * 0.5 ** it)
        sched.step()
        tsched.step()
        torch.cuda.synchronize()
        adam_bar(mix.weights.detach().cpu().numpy(), rmix.weights.detach().cpu().numpy(), oracle["w"], f"step {it} mix weights")
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in topt.param_groups]       # schedulers scale both groups
        want_p = igr.softmax64(mix.weights.detach().cpu().numpy())
        assert (np.abs(opt.mix_p().cpu().numpy() - want_p) <= 2.0 ** -23 * want_p).all()
    assert int(opt.state[mix.weights]["step"]) == 2
    # state dicts in torch.optim.Adam's two-group format, in both directions
    sd, tsd = opt.state_dict(), topt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in tsd["param_groups"]]
    assert set(sd["param_groups"][1]) == set(tsd["param_groups"][1]) and set(sd["state"]) == set(tsd["state"])
    # torch -> fused: a fused optimizer takes over torch's weights and state; fused -> torch: the other way round.  Each pair
    # continues for two steps beside a float64 restatement that starts from the same float32 weights and moments.
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)                     # noqa: E731
    m2, mix2 = setup()
    rm2, rmix2 = setup()
    for a, b in ((m2, rm), (mix2, rmix), (rm2, m), (rmix2, mix)):
        a.load_state_dict(b.state_dict())
    opt2 = FusedAdam(m2, lr=1e-3, layer_mix=mix2, layer_mix_lr=LR)
    topt2 = torch.optim.Adam([{"params": rm2.parameters()}, {"params": [rmix2.weights], "lr": LR}], lr=1e-3)
    opt2.load_state_dict(copy.deepcopy(tsd))
    topt2.load_state_dict(copy.deepcopy(sd))
    assert opt2.param_groups[1]["lr"] == topt.param_groups[1]["lr"] and topt2.param_groups[1]["lr"] == opt.param_groups[1]["lr"]
    lr_now = opt.param_groups[1]["lr"]
    pairs = []                                                # (fused side, torch side, float64 weights, float64 state)
    for fmix, tmix, st in ((mix2, rmix, topt.state[rmix.weights]), (mix, rmix2, opt.state[mix.weights])):
        pairs.append((fmix, tmix, {"w": f64(tmix.weights if st is topt.state[rmix.weights] else fmix.weights)},
                      {"step": 2, "m": {"w": f64(st["exp_avg"])}, "v": {"w": f64(st["exp_avg_sq"])}}))
    for it in range(2, 4):
        for mm, xx in ((m, mix), (m2, mix2), (rm, rmix), (rm2, rmix2)):
            give_grads(mm, xx, it)
        for o in (opt, opt2, topt, topt2):
            o.step()
        for _, _, prm, st in pairs:
            to.adam_step(prm, {"w": seq[it][1].astype(np.float64)}, st, lr_now)
    torch.cuda.synchronize()
    for (fmix, tmix, prm, _), what in zip(pairs, ("torch -> fused", "fused -> torch")):
        adam_bar(fmix.weights.detach().cpu().numpy(), tmix.weights.detach().cpu().numpy(), prm["w"], what)
    assert int(opt2.state[mix2.weights]["step"]) == 4 and int(topt2.state[rmix2.weights]["step"]) == 4
