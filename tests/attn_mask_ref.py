"""Reference and tolerances of masked attention, shared by test_attention_mask_cpu.py and test_attention_mask_gpu.py.
`bf`, `close` and `attn_ref` are the ones of tests/test_kernels_gpu.py (the arithmetic of the masked kernels is that of
the unmasked ones), `attn_ref` with the additive mask in the scores: torch in fp32 on the bf16-rounded inputs,
softmax(q k^T * scale + M) v and its logsumexp; gradients come from autograd on it.  The tests run it on the CPU."""
import math

import numpy as np
import torch


def bf(t):
    return t.to(torch.bfloat16)


def close(got, ref, rel=1.0 / 128, abs_scale=1.0 / 64):
    got, ref = got.float(), ref.float()
    tol = rel * ref.abs() + abs_scale * ref.pow(2).mean().sqrt().clamp_min(1e-6)
    bad = (got - ref).abs() > tol
    assert not bad.any(), f"{int(bad.sum())}/{bad.numel()} off, max err {float((got - ref).abs().max())}, ref rms {float(ref.pow(2).mean().sqrt())}"


def attn_ref(qkv, H, mask=None):
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    q, k, v = qkv.float().split(D, dim=-1)
    sp = lambda t: t.reshape(B, N, H, hd).transpose(1, 2)
    s = (sp(q) @ sp(k).transpose(-1, -2)) / math.sqrt(hd)
    if mask is not None:
        s = s + mask.float()
    p = torch.softmax(s, -1)
    o = (p @ sp(v)).transpose(1, 2).reshape(B, N, D)
    return o, torch.logsumexp(s, -1)


def block_map_ref(mask, blk=64):
    """numpy restatement of sfcvit_attention_mask_blocks: per (blk x blk) block 0 = no finite entry, 2 = every entry 0.0,
    1 = anything else."""
    m = mask.numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    N = m.shape[0]
    nb = (N + blk - 1) // blk
    out = np.zeros((nb, nb), dtype=np.uint8)
    for i in range(nb):
        for j in range(nb):
            t = m[i * blk:(i + 1) * blk, j * blk:(j + 1) * blk]
            out[i, j] = 0 if not np.isfinite(t).any() else 2 if (t == 0).all() else 1
    return out


def random_mask(N, density=0.3, seed=0):
    """A 0 / -inf mask with `density` of the pairs visible, one visible key forced per row; (when N >= 3) row 0 sees key
    N - 1 only, and key column 1 is hidden from every row.  -> (mask, hidden column or None)."""
    g = torch.Generator().manual_seed(seed)
    vis = torch.rand(N, N, generator=g) < density
    vis[torch.arange(N), torch.randint(0, N, (N,), generator=g)] = True
    hidden = None
    if N >= 3:
        hidden = 1
        vis[:, hidden] = False
        empty = ~vis.any(dim=1)
        vis[empty, 0] = True                 # a row whose forced key was the hidden column
        vis[0, :] = False
        vis[0, N - 1] = True
    m = torch.full((N, N), float("-inf"))
    m[vis] = 0.0
    return m, hidden


def bias_mask(N):
    """Finite additive bias -0.1 |i - j|: nothing is hidden, nothing is skipped."""
    i = torch.arange(N, dtype=torch.float32)
    return -0.1 * (i[:, None] - i[None, :]).abs()
