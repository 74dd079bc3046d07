"""Generate tests/golden/cnnlstm_input_grad_*.npz: ``x.grad`` of the REFERENCE module (src/models.py) in training mode.

Run in the build container only (needs /root/reference):  python tests/golden/make_cnnlstm_input_grad_golden.py
The four cases, seeds and conventions of make_cnnlstm_train_golden.py (float64 module, dropout probabilities 0,
CrossEntropyLoss, one backward), with the input as a leaf.  Loss and logits must be the ones cnnlstm_train_*.npz already
hold: the step is the same step.  What is committed is data: weights.sample_tensor(x.grad) (evenly spaced samples + sum +
sum of squares).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")
from src.models import CNNLSTM  # noqa: E402  (the reference)
from weights import sample_tensor, synth_input, synth_state_dict  # noqa: E402

torch.set_num_threads(4)
torch.use_deterministic_algorithms(True)

# (name, input_dim, C, H, act, B, T, seed): make_cnnlstm_train_golden.py
CASES = [
    ("d16_c32_h64_silu", 16, 32, 64, "silu", 3, 20, 201),
    ("d16_c64_h128_gelu", 16, 64, 128, "gelu", 2, 13, 202),
    ("d768_c128_h128_silu", 768, 128, 128, "silu", 4, 33, 203),
    ("d32_c32_h64_identity_shortcut", 32, 32, 64, "silu", 2, 16, 204),
]

for name, D, C, H, act, B, T, seed in CASES:
    m = CNNLSTM(input_dim=D, cnn_out_channels=C, lstm_hidden_dim=H, activation_fn=act, dropout_rate=0.0).double()
    full = m.state_dict()
    for k, v in synth_state_dict(D, C, H, seed).items():
        full[k] = torch.from_numpy(v).double()
    m.load_state_dict(full)
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    m.train()
    x = torch.from_numpy(synth_input(B, T, D, seed + 1000)).double().requires_grad_(True)
    labels = torch.from_numpy(np.random.Generator(np.random.PCG64(seed + 2000)).integers(0, 2, B))
    out = m(x)
    loss = nn.CrossEntropyLoss()(out, labels)
    loss.backward()
    z = np.load(os.path.join(HERE, f"cnnlstm_train_{name}.npz"))
    assert [int(v) for v in z["meta"]] == [D, C, H, B, T, seed] and np.array_equal(z["labels"], labels.numpy())
    assert float(z["loss"]) == loss.item() and np.array_equal(z["logits"], out.detach().numpy()), name
    g = x.grad.numpy()
    assert g.shape == (B, T, D)
    np.savez_compressed(os.path.join(HERE, f"cnnlstm_input_grad_{name}.npz"), meta=np.array([D, C, H, B, T, seed]),
                        act=np.array(act), dx=sample_tensor(g), dx_max=np.array(np.abs(g).max()))
    print(name, loss.item(), np.abs(g).max(), np.abs(g[:, -1]).max())
