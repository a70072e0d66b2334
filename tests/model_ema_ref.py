"""Model EMA restated without a GPU (include/sfcvit.h, "Model EMA"): the decay of step t in numpy float32, operation by
operation as the kernel computes it, and the average itself in fp64."""
import numpy as np


def decay_at(decay, warmup, t):
    """d_t of the t-th update (t 1-based) as a Python float holding an fp32 value: `decay` rounded to fp32, or with warm-up
    min(decay, float(1 + t) / float(10 + t)) with a correctly rounded fp32 division."""
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + t) / np.float32(10 + t))
    return float(d)


def ema_steps(e0, masters, decay, warmup, t0):
    """The averages after each of len(masters) updates, in fp64: e0 the average before, masters[k] the fp32 master weights
    after update t0 + 1 + k (t0 updates were taken before).  1 - d_t is the kernel's fp32 difference (exact for d_t >= 0.5,
    a rounded fp32 value otherwise: either way the number the kernel multiplies by)."""
    e = np.asarray(e0, dtype=np.float64).copy()
    out = []
    for k, w in enumerate(masters):
        d = np.float32(decay_at(decay, warmup, t0 + 1 + k))
        omd = float(np.float32(1.0) - d)
        e = e + omd * (np.asarray(w, dtype=np.float64) - e)
        out.append(e.copy())
    return out


def ema_bar(K, e0, masters, refs):
    """Element-wise bound on |ema - ref| after K updates (tests/test_model_ema_gpu.py derives it):
    2 * K * 3 * 2^-24 * max(|w|, |e|), the maximum taken over every step."""
    big = np.abs(np.asarray(e0, dtype=np.float64))
    for a in list(masters) + list(refs):
        big = np.maximum(big, np.abs(np.asarray(a, dtype=np.float64)))
    return 2.0 * K * 3.0 * 2.0 ** -24 * big
