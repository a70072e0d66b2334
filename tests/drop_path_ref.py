"""References for stochastic depth (DropPath): the keep flag restated in numpy (the dropout hash of csrc/device_common.h), the
scaled residual add + LayerNorm in torch at any precision with its backward by autograd, and the post-norm encoder layer with
explicit dropout masks and per-image branch flags."""
import math

import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
DROP_G, DROP_C = np.uint64(0x9E3779B1), np.uint64(0x2C1B3C6D)


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def row_key(seed, rows):
    """drop_row_key for rows < 2^32: mix32(row * G + mix32(seed))."""
    rows = np.asarray(rows, dtype=np.uint64)
    return mix32(((rows & M32) * DROP_G + mix32(np.full(rows.shape, seed & 0xFFFFFFFF, np.uint64))) & M32)


def keep_flags(seed, rate, B):
    """bool [B]: element (row b, column 0) of the dropout mask of `seed` at p = rate: (key(b) ^ 0 * G) * C >= thresh << 16."""
    thresh = np.uint64(int(np.float32(rate) * np.float32(65536.0) + np.float32(0.5)))
    h = (row_key(seed, np.arange(B)) * DROP_C) & M32
    return h >= (thresh << np.uint64(16))


def dropout_keep(seed, p, rows, cols):
    """bool [rows, cols]: the whole dropout mask of `seed` at rate p for rows < 2^32, as csrc/device_common.h states it:
    keep(row, col) = ((drop_row_key(seed, row) ^ col * G) * C mod 2^32) >= (thresh << 16), thresh = uint32(p * 65536.f + 0.5f).
    `rows` is a count (rows 0 .. rows - 1) or an array of row numbers."""
    thresh = np.uint64(int(np.float32(p) * np.float32(65536.0) + np.float32(0.5)))
    rows = np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else np.asarray(rows, dtype=np.uint64)
    assert rows.size == 0 or int(rows.max()) < 2 ** 32
    col_g = (np.arange(cols, dtype=np.uint64) * DROP_G) & M32
    h = ((row_key(seed, rows)[:, None] ^ col_g[None, :]) * DROP_C) & M32
    return h >= (thresh << np.uint64(16))


def layer_rates(rate, L):
    return [rate * l / (L - 1) if L > 1 else rate for l in range(L)]


def add_layernorm(x, branch, c_rows, gamma, beta, eps=1e-5):
    """s = x + c[row] * branch, LayerNorm(s); tensors of one dtype (fp64 / fp32), c_rows [M]."""
    s = x + c_rows[:, None] * branch
    return s, torch.nn.functional.layer_norm(s, (x.shape[1],), gamma, beta, eps)


def layernorm_of(s, gamma, beta, eps=1e-5):
    """fp64 LayerNorm of a stored bf16 s -> (y, mean, rstd)."""
    s = s.double()
    mean = s.mean(1)
    var = s.var(1, unbiased=False)
    rstd = (var + eps).rsqrt()
    return (s - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double(), mean, rstd


def encoder_layer(x, P, H, masks, c1, c2, attn_mask=None, eps=1e-5):
    """Post-norm encoder layer in the dtype of its inputs.  masks = (ma [B, H, N, N], m1 [B, N, D], mf [B, N, F], m2 [B, N, D]),
    each {0, 1 / (1 - p)}; c1, c2 [B] = keep / (1 - rate) of the two residual sites; attn_mask additive [N, N] or None."""
    B, N, D = x.shape
    hd = D // H
    ma, m1, mf, m2 = masks
    qkv = x @ P["in_w"].t() + P["in_b"]
    q, k, v = qkv.split(D, dim=-1)
    sp = lambda t: t.reshape(B, N, H, hd).transpose(1, 2)      # noqa: E731
    s = (sp(q) @ sp(k).transpose(-1, -2)) / math.sqrt(hd)
    if attn_mask is not None:
        s = s + attn_mask
    o = ((torch.softmax(s, -1) * ma) @ sp(v)).transpose(1, 2).reshape(B, N, D)
    a = (o @ P["out_w"].t() + P["out_b"]) * m1
    x1 = torch.nn.functional.layer_norm(x + c1[:, None, None] * a, (D,), P["n1_w"], P["n1_b"], eps)
    h = torch.relu(x1 @ P["w1"].t() + P["b1"]) * mf
    f = (h @ P["w2"].t() + P["b2"]) * m2
    return torch.nn.functional.layer_norm(x1 + c2[:, None, None] * f, (D,), P["n2_w"], P["n2_b"], eps)
