"""NumPy restatement of the dropout mask mapping that include/rsaf.h documents (helper of test_dropout_rng_host.py and
test_dropout_masks_gpu.py; no test lives here).  Written from the published Philox4x32-10 and the header comment alone: it
shares no code with csrc/dropout_rng.h."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

SEEDS = (0, 1, 0x5EED, 2 ** 63 + 12345)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> uint32 array [..., 4]."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, step, slot, n):
    """The raw word of each of the n elements of a slot."""
    j = np.arange((n + 3) // 4, dtype=np.uint64)
    out = philox4x32_10((j, slot, step & MASK32, step >> 32), (seed & MASK32, seed >> 32))
    return out.reshape(-1)[:n]


def threshold(p):
    return int(math.floor(p * 2.0 ** 32))


def keep_value(p):
    return np.float32(1.0) / np.float32(1.0 - p)


def mask(seed, step, slot, n, p):
    """float32 [n]: 1 / (1 - p) where the element's word >= floor(p * 2^32), else 0; all zeros for p >= 1."""
    if p >= 1.0:
        return np.zeros(n, dtype=np.float32)
    keep = words(seed, step, slot, n) >= np.uint32(threshold(p))
    return np.where(keep, keep_value(p), np.float32(0.0)).astype(np.float32)


def model_masks(dims, B, T, p_block1, p_block2, p_lstm, p_fc, seed, step):
    """The masks of one training step in the format of ``draw_masks`` (NumPy arrays; None where p == 0)."""
    C, H, L, Tp = dims["channels"], dims["hidden"], dims["layers"], T // 2

    def mk(slot, shape, p):
        return None if p <= 0.0 else mask(seed, step, slot, int(np.prod(shape)), p).reshape(shape)

    return {"res_block1": mk(0, (B, T, C), p_block1), "res_block2": mk(1, (B, Tp, C), p_block2),
            "fc": mk(2, (B, 2 * H), p_fc), "lstm": [mk(3 + l, (B, Tp, 2 * H), p_lstm) for l in range(L - 1)]}
