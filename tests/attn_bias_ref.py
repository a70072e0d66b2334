"""References of attention with a learned relative position bias, shared by test_attention_bias_cpu.py,
test_attention_bias_gpu.py and test_attention_bias_containment_gpu.py.

    s[b,h,i,j] = scale * q_i . k_j + table[h, index[i,j]]      (index -1: -inf)
    P = softmax_j(s),  lse_i = log sum_j exp(s_ij)
    dTable[h,t] = sum over b and (i,j) with index[i,j] == t of  P_ij (keep_ij dP_ij - delta_i)

`bias_term` turns (table, index) into the per-head additive term [H, N, N] that tests/attn_mask_ref.py's `attn_ref` takes as
its mask (fp32 reference of out, lse, dqkv).  `backward64` is the manual fp64 statement of the formulas above -- what the
table-gradient tests hold the kernels to -- and `blocks_ref` the numpy restatement of sfcvit_attention_bias_blocks."""
import math

import numpy as np
import torch


def bias_term(table, index):
    """[H, N, N] in table's dtype: table[h, index[i,j]], -inf where index is -1."""
    idx = torch.as_tensor(index).long()
    term = table[:, idx.clamp_min(0)]
    return term.masked_fill((idx < 0)[None], float("-inf"))


def blocks_ref(index, n_buckets, blk=64):
    """numpy restatement of sfcvit_attention_bias_blocks -> (map [nb, nb] uint8: 1 where a block has an entry >= 0,
    offsets [T + 1] int32, positions int32: per bucket the i * N + j with index[i,j] == t, ascending)."""
    ix = index.numpy() if isinstance(index, torch.Tensor) else np.asarray(index)
    N = ix.shape[0]
    nb = (N + blk - 1) // blk
    bmap = np.zeros((nb, nb), dtype=np.uint8)
    for i in range(nb):
        for j in range(nb):
            bmap[i, j] = int((ix[i * blk:(i + 1) * blk, j * blk:(j + 1) * blk] >= 0).any())
    flat = ix.reshape(-1)
    offsets, positions = [0], []
    for t in range(n_buckets):
        where = np.nonzero(flat == t)[0]                        # ascending i * N + j
        positions.append(where)
        offsets.append(offsets[-1] + len(where))
    return bmap, np.asarray(offsets, dtype=np.int32), (np.concatenate(positions) if positions else np.zeros(0)).astype(np.int32)


def _heads(t, B, N, H, hd):
    return t.reshape(B, N, H, hd).transpose(1, 2)


def forward64(qkv, H, table, index):
    """fp64 forward on the given (bf16-rounded) inputs -> out [B, N, D], lse [B, H, N], both fp64."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    q, k, v = (_heads(t, B, N, H, hd) for t in qkv.double().split(D, dim=-1))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd) + bias_term(table.double(), index)[None]
    lse = torch.logsumexp(s, -1)
    out = (torch.exp(s - lse[..., None]) @ v).transpose(1, 2).reshape(B, N, D)
    return out, lse


def backward64(qkv, H, table, index, dout, out, lse, keep=None):
    """The manual fp64 backward from the formulas in the module docstring, on exactly the inputs a backward kernel gets:
    qkv / dout / out (bf16 values) and lse (fp32 values), all promoted to fp64.  keep: None, or [B, H, N, N] of 0 or
    1 / (1 - p).  -> dqkv [B, N, 3 D], dtable [H, T], A [H, T] = sum |P (keep dP - delta)| per bucket (the scale of the
    table gradient's rounding bound)."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    T = table.shape[1]
    scale = 1.0 / math.sqrt(hd)
    q, k, v = (_heads(t, B, N, H, hd) for t in qkv.double().split(D, dim=-1))
    do, o = _heads(dout.double(), B, N, H, hd), _heads(out.double(), B, N, H, hd)
    s = (q @ k.transpose(-1, -2)) * scale + bias_term(table.double(), index)[None]
    p = torch.exp(s - lse.double()[..., None])
    kp = torch.ones_like(p) if keep is None else keep.double()
    dp = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    g = p * (kp * dp - delta)                                   # dS before the scale; a hidden pair has p = 0
    dq, dk, dv = (g @ k) * scale, (g.transpose(-1, -2) @ q) * scale, (p * kp).transpose(-1, -2) @ do
    dqkv = torch.cat([t.transpose(1, 2).reshape(B, N, D) for t in (dq, dk, dv)], dim=-1)
    idx = torch.as_tensor(index).long()
    vis = (idx >= 0).reshape(-1)
    flat = idx.reshape(-1)[vis]
    gs = g.sum(0).reshape(H, N * N)[:, vis]
    ga = g.abs().sum(0).reshape(H, N * N)[:, vis]
    dtable = torch.zeros(H, T, dtype=torch.float64).index_add_(1, flat, gs)
    A = torch.zeros(H, T, dtype=torch.float64).index_add_(1, flat, ga)
    return dqkv, dtable, A


def autograd64(qkv, H, table, index, dout):
    """torch autograd in fp64 on softmax(scale q k^T + table[:, index]) v -> out, lse, dqkv, dtable."""
    qf = qkv.detach().double().clone().requires_grad_(True)
    tf = table.detach().double().clone().requires_grad_(True)
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    q, k, v = (_heads(t, B, N, H, hd) for t in qf.split(D, dim=-1))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd) + bias_term(tf, index)[None]
    out = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, N, D)
    out.backward(dout.double())
    return out.detach(), torch.logsumexp(s.detach(), -1), qf.grad, tf.grad


def worst_ratio(got, ref, A):
    """max over buckets of |got - ref| / A_t (buckets with A_t = 0 must match exactly and count as 0)."""
    err = (got.double().cpu() - ref).abs()
    assert bool((err[A == 0] == 0).all()), "an empty bucket's gradient is not exactly 0"
    return float((err / A.clamp_min(1e-300))[A > 0].max()) if bool((A > 0).any()) else 0.0


def random_positions(n, cell=16, seed=0):
    """n distinct cell centres of a grid, in a random order: token centres as analysis.token_positions gives them."""
    side = int(math.ceil(math.sqrt(n)))
    g = torch.Generator().manual_seed(seed)
    pick = torch.randperm(side * side, generator=g)[:n]
    return torch.stack(((pick // side).float() * cell + (cell - 1) / 2.0, (pick % side).float() * cell + (cell - 1) / 2.0), dim=1)
