"""References for QK-norm, written from the formula: a LayerNorm over the head dim on the queries and keys of every head before
q k^T (parameters P [4, hd]: q_weight, q_bias, k_weight, k_bias, shared by the heads).  The layer references stand on
drop_path_ref.encoder_layer (post-norm) and prenorm_ref.pre_norm_layer: with qk_norm=None they ARE those functions; with
parameters they are the same statements with the norm between the projection and the scores.  Also: the exact-answer inputs
of the kernel tests (Walsh rows) and fp64 restatements of both kernel directions on a packed, padded buffer."""
import math

import torch

import drop_path_ref
import prenorm_ref


def _ln(t, w, b, eps):
    return torch.nn.functional.layer_norm(t, (t.shape[-1],), w, b, eps)


def qk_normed(qkv, H, qk_norm, eps=1e-6):
    """qkv [B, N, 3 D] -> (q, k, v) as [B, H, N, hd], q and k normalised over hd on the [B, N, 3, H, hd] view."""
    B, N, D3 = qkv.shape
    hd = D3 // 3 // H
    t = qkv.reshape(B, N, 3, H, hd)
    q = _ln(t[:, :, 0], qk_norm[0], qk_norm[1], eps)
    k = _ln(t[:, :, 1], qk_norm[2], qk_norm[3], eps)
    return q.transpose(1, 2), k.transpose(1, 2), t[:, :, 2].transpose(1, 2)


def attention(qkv, H, qk_norm, eps=1e-6, attn_mask=None, rel_bias=None, ma=None):
    """softmax(LN(q) LN(k)^T / sqrt(hd) [+ mask] [+ bias]) [* ma] v -> ([B, N, D], probabilities [B, H, N, N])."""
    B, N, D3 = qkv.shape
    q, k, v = qk_normed(qkv, H, qk_norm, eps)
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    if attn_mask is not None:
        sc = sc + attn_mask
    if rel_bias is not None:
        sc = sc + rel_bias
    p = torch.softmax(sc, -1)
    pm = p if ma is None else p * ma
    return (pm @ v).transpose(1, 2).reshape(B, N, D3 // 3), p


def encoder_layer(x, P, H, masks, c1, c2, attn_mask=None, eps=1e-5, qk_norm=None, qk_eps=1e-6, rel_bias=None):
    """Post-norm layer: drop_path_ref.encoder_layer, with QK-norm (and then an additive rel_bias [H, N, N] too) when qk_norm
    [4, hd] is given."""
    if qk_norm is None:
        assert rel_bias is None
        return drop_path_ref.encoder_layer(x, P, H, masks, c1, c2, attn_mask, eps)
    B, N, D = x.shape
    ma, m1, mf, m2 = masks
    qkv = x @ P["in_w"].t() + P["in_b"]
    o, _ = attention(qkv, H, qk_norm, qk_eps, attn_mask, rel_bias, ma)
    a = (o @ P["out_w"].t() + P["out_b"]) * m1
    x1 = _ln(x + c1[:, None, None] * a, P["n1_w"], P["n1_b"], eps)
    h = torch.relu(x1 @ P["w1"].t() + P["b1"]) * mf
    f = (h @ P["w2"].t() + P["b2"]) * m2
    return _ln(x1 + c2[:, None, None] * f, P["n2_w"], P["n2_b"], eps)


def pre_norm_layer(s, n, P, H, masks=None, c1=None, c2=None, lam=None, act="relu", attn_mask=None, rel_bias=None, eps=1e-5,
                   keep=None, qk_norm=None, qk_eps=1e-6):
    """Pre-norm layer: prenorm_ref.pre_norm_layer, with QK-norm when qk_norm [4, hd] is given."""
    if qk_norm is None:
        return prenorm_ref.pre_norm_layer(s, n, P, H, masks, c1, c2, lam, act, attn_mask, rel_bias, eps, keep)
    B, N, D = s.shape
    one = s.new_ones(())
    ma, m1, mf, m2 = masks if masks is not None else (one, one, one, one)
    c1 = s.new_ones(B) if c1 is None else c1
    c2 = s.new_ones(B) if c2 is None else c2
    l1, l2 = lam if lam is not None else (one, one)
    qkv = n @ P["in_w"].t() + P["in_b"]
    o, _ = attention(qkv, H, qk_norm, qk_eps, attn_mask, rel_bias, ma)
    a = (o @ P["out_w"].t() + P["out_b"]) * m1
    s1 = s + c1[:, None, None] * l1 * a
    n1 = _ln(s1, P["n2_w"], P["n2_b"], eps)
    u = n1 @ P["w1"].t() + P["b1"]
    h = (torch.relu(u) if act == "relu" else torch.nn.functional.gelu(u)) * mf
    f = (h @ P["w2"].t() + P["b2"]) * m2
    s2 = s1 + c2[:, None, None] * l2 * f
    n2 = _ln(s2, P["next_w"], P["next_b"], eps)
    if keep is not None:
        keep.update(a=a, s1=s1, n1=n1, u=u, h=h, f=f)
    return s2, n2


# ---- the kernels on a packed, padded buffer ------------------------------------------------------------------------------------
def heads(buf, H, hp, thirds):
    """[M, thirds * H * hp] -> [M, thirds, H, hp] view."""
    return buf.reshape(buf.shape[0], thirds, H, hp)


def forward64(qkv, P, H, hd, hp, eps):
    """fp64 QK-norm of a packed bf16 buffer [M, 3 H hp] -> fp64 [M, 3, H, hp]: q, k normalised over their hd real columns with
    zeros behind, v as it is."""
    t = heads(qkv.double(), H, hp, 3).clone()
    Pd = P.double()
    for i in range(2):
        t[:, i, :, :hd] = _ln(t[:, i, :, :hd], Pd[2 * i], Pd[2 * i + 1], eps)
        t[:, i, :, hd:] = 0
    return t


def backward64(dy, raw, P, H, hd, hp, eps):
    """fp64 backward on the kernel's own inputs: dy [M, 3 H hp] (q | k thirds used), raw [M, 2 H hp] -> (dx [M, 2, H, hp] with
    zeros in the padding, dP [4, hd], and the sums of |addends| of dgamma and of dbeta, [2, hd] each: q, k)."""
    x = heads(raw.double(), H, hp, 2)[..., :hd]
    g = heads(dy.double(), H, hp, 3)[:, :2, :, :hd]
    mean = x.mean(-1, keepdim=True)
    rstd = (x.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    xh = (x - mean) * rstd
    gamma = P.double()[[0, 2]][None, :, None, :]
    gy = g * gamma
    dx = rstd * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))
    out = torch.zeros(dy.shape[0], 2, H, hp, dtype=torch.float64, device=dy.device)
    out[..., :hd] = dx
    dgam, dbet = (g * xh).sum((0, 2)), g.sum((0, 2))
    return out, torch.stack([dgam[0], dbet[0], dgam[1], dbet[1]]), (g * xh).abs().sum((0, 2)), g.abs().sum((0, 2))


def walsh(n):
    """The n x n Sylvester-Hadamard matrix (n a power of two), entries +-1; row 0 is the ones row, every other row is balanced
    and the rows are mutually orthogonal."""
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def exact_inputs(M, H, hd):
    """The exact-answer case for hd a power of two >= 64 (no padding) -> x [M, 2 H, hd] = 2^k * Walsh row r(slot) (a different
    balanced row per head slot, k in 0..5 per row), gy [M, 2 H, hd] = 2^m * another balanced Walsh row (orthogonal to x's row
    and to the ones row, m in -3..2), k [M, 2H], m [M, 2H], gamma, beta [hd].  Then mean = 0 and var = 4^k exactly, x_hat is the
    sign row up to rstd's rounding, LN(x) = gamma * sign + beta rounds to itself in bf16, and dx = 2^(m - k) * gy's row."""
    W = walsh(hd)
    slots = torch.arange(2 * H)
    rows = torch.arange(M)
    rx = 1 + (slots[None, :] * 2 + rows[:, None] * 0) % (hd - 1)                  # balanced rows 1 .. hd - 1, one per slot
    rg = 1 + (rx - 1 + 1 + (rows[:, None] % 5)) % (hd - 1)                        # another balanced row
    assert bool((rx != rg).all())
    k = (rows[:, None] + slots[None, :]) % 6
    m = (rows[:, None] * 3 + slots[None, :]) % 6 - 3
    x = W[rx] * torch.pow(2.0, k.float())[..., None]
    gy = W[rg] * torch.pow(2.0, m.float())[..., None]
    d = torch.arange(hd)
    gamma = torch.pow(2.0, ((d % 3) - 1).float()) * (1 - 2 * ((d // 3) % 2)).float()
    beta = ((d % 5) - 2).float() / 4 + 1 / 8
    return x, gy, k, m, W[rx], W[rg], gamma, beta
