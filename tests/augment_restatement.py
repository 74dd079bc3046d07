"""NumPy restatement of the augmentation mapping that include/rsaf.h documents (helper of test_augment_host.py and
test_augment_gpu.py; no test lives here).  Written from the header comment and the published Philox4x32-10 (the
restatement of tests/dropout_restatement.py): it shares no code with csrc/augment_rng.h.  Normals are float64."""
import math

import numpy as np

from dropout_restatement import MASK32, philox4x32_10

SCALE, GAUSSIAN_NOISE, TIME_MASK, FEATURE_MASK = 0, 1, 2, 3
STREAM0 = 0x100
Z_MAX = math.sqrt(48.0 * math.log(2.0))         # r at u1 = 2^-24: no normal lies beyond it


def _key(seed):
    return seed & MASK32, seed >> 32


def param_words(seed, epoch, sample, s):
    """w0 .. w3 of op number s: counter (0, 0x100 + 2 s, draw low, draw high), draw = (epoch << 32) | sample."""
    draw = (epoch << 32) | sample
    return [int(v) for v in philox4x32_10((0, STREAM0 + 2 * s, draw & MASK32, draw >> 32), _key(seed))]


def fires(p, w0):
    return p >= 1.0 or w0 < math.floor(p * 2.0 ** 32)


def unit(w):
    return (w >> 8) * 2.0 ** -24


def uniform32(lo, hi, w):
    """float32(lo + (hi - lo) * u(w)), the arithmetic in float64 (Python floats), one rounding to float32."""
    return np.float32(lo + (hi - lo) * unit(w))


def span(n, min_part, max_part, w1, w2):
    """(start, len) of the masked span out of n frames or columns."""
    lo, hi = math.floor(n * min_part), math.floor(n * max_part)
    length = lo + ((w1 * (hi - lo + 1)) >> 32)
    start = (w2 * (n - length + 1)) >> 32
    return start, length


def normals(seed, epoch, sample, s, n):
    """float64 [n]: the normals of elements 0 .. n - 1 of op number s."""
    draw = (epoch << 32) | sample
    j = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((j, STREAM0 + 2 * s + 1, draw & MASK32, draw >> 32), _key(seed)).astype(np.uint64)
    out = np.empty((len(j), 4), dtype=np.float64)
    for pair in (0, 1):
        u1 = ((w[:, 2 * pair] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[:, 2 * pair + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * pair] = r * np.cos(2.0 * np.pi * u2)
        out[:, 2 * pair + 1] = r * np.sin(2.0 * np.pi * u2)
    return out.reshape(-1)[:n]


def decisions(ops, seed, epoch, sample, T, D):
    """What each op of the pipeline decides for one sequence [T, D]: a list of dicts with `fires` and, by kind, `factor` /
    `amp` (float32) or `start`, `len`.  ops: (kind, a, b, p) tuples."""
    out = []
    for s, (kind, a, b, p) in enumerate(ops):
        w = param_words(seed, epoch, sample, s)
        d = {"kind": kind, "fires": fires(p, w[0])}
        if kind == SCALE:
            d["factor"] = uniform32(a, b, w[1])
        elif kind == GAUSSIAN_NOISE:
            d["amp"] = uniform32(a, b, w[1])
        else:
            d["start"], d["len"] = span(T if kind == TIME_MASK else D, a, b, w[1], w[2])
        out.append(d)
    return out


def apply(x, ops, seed, epoch, sample):
    """The pipeline applied to one float32 sequence [T, D] -> (ref, amp_sum).  Deterministic ops are applied in float32
    (bit-exact); noise is added in float64, and from the first noise op on `ref` is float64 (what the bound of the noise
    test is taken against).  amp_sum [T, D]: the sum of the amplitudes of the noise ops that touched each element and
    whose contribution was not masked out afterwards."""
    T, D = x.shape
    ref = x.astype(np.float32).copy()
    amp_sum = np.zeros((T, D), dtype=np.float64)
    for s, d in enumerate(decisions(ops, seed, epoch, sample, T, D)):
        if not d["fires"]:
            continue
        if d["kind"] == SCALE:
            ref = ref * d["factor"] if ref.dtype == np.float32 else ref * np.float64(d["factor"])
        elif d["kind"] == GAUSSIAN_NOISE:
            z = normals(seed, epoch, sample, s, T * D).reshape(T, D)
            ref = ref.astype(np.float64) + np.float64(d["amp"]) * z
            amp_sum += float(d["amp"])
        elif d["kind"] == TIME_MASK:
            ref[d["start"]:d["start"] + d["len"], :] = 0.0
            amp_sum[d["start"]:d["start"] + d["len"], :] = 0.0
        else:
            ref[:, d["start"]:d["start"] + d["len"]] = 0.0
            amp_sum[:, d["start"]:d["start"] + d["len"]] = 0.0
    return ref, amp_sum
