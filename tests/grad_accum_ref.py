"""Gradient accumulation restated without a GPU (include/sfcvit.h, "Gradient accumulation"): both kernels in numpy float32,
operation by operation, with bf16 round-to-nearest-even done on the bit pattern, and the sum of squares in fp64.

bf16 values travel as uint16 bit patterns (numpy has no bf16)."""
import numpy as np


def bf16_to_f32(bits):
    """uint16 bf16 bit patterns -> the float32 values they denote (exact)."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x):
    """float32 -> bf16 bit patterns, round to nearest, ties to even, on the bit pattern; NaN stays NaN (quiet)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(x)
    if nan.any():
        r = np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)
    return r


def accum(grad_bits, acc, first):
    """sfcvit_grad_accum: float(grad) when `first` (acc is not read), else acc + float(grad) -- one fp32 add."""
    g = bf16_to_f32(grad_bits)
    if first:
        return g.copy()
    return (np.asarray(acc, dtype=np.float32) + g).astype(np.float32)


def scale_of(k):
    """float32(1 / K), the scale FlatGradBuffer.fold hands to the kernel for K micro-batches."""
    return np.float32(1.0 / k)


def finish(grad_bits, acc, scale):
    """sfcvit_grad_accum_finish: bf16_rne((acc + float(grad)) * scale) -- one fp32 add, one fp32 multiply, one rounding.
    -> (the new bf16 bit patterns, the fp64 sum of the squares of the stored values)."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = (np.asarray(acc, dtype=np.float32) + bf16_to_f32(grad_bits)).astype(np.float32)
        out = f32_to_bf16((s * np.float32(scale)).astype(np.float32))
    return out, float(np.sum(bf16_to_f32(out).astype(np.float64) ** 2))


def fold(grads_bits):
    """K >= 2 micro-batch gradients (bf16 bit patterns, in order) -> (averaged gradient bits, fp64 sum of squares, the fp32
    running sum the last call read): first, add ..., finish with scale float32(1 / K).  K = 1 is never folded."""
    k = len(grads_bits)
    if k < 2:
        raise ValueError("a single micro-batch is not folded: its gradient is used as it is")
    acc = accum(grads_bits[0], None, True)
    for g in grads_bits[1:-1]:
        acc = accum(g, acc, False)
    out, sumsq = finish(grads_bits[-1], acc, scale_of(k))
    return out, sumsq, acc
