"""References for rotary position embeddings, written from the formula: channel pair p = columns (2 p, 2 p + 1) of every query
and key head row of token n goes through the 2 x 2 map [c -s; s c] with (c, s) = table[n, p] (table [N, hd / 2, 2], shared by
the heads, the batch, and q and k), after QK-norm and before q k^T.  The layer references stand on qk_norm_ref.encoder_layer /
pre_norm_layer: with rope=None they ARE those functions; with a table they are the same statements with the rotation between
the norm and the scores.  Also: the exact-answer inputs of the kernel tests and fp64 restatements of both kernel directions on
a packed, padded buffer."""
import math

import torch

import qk_norm_ref
from qk_norm_ref import _ln, heads          # noqa: F401  (heads: [M, thirds * H * hp] -> [M, thirds, H, hp])


def rotate(t, table):
    """t [..., N, hd] (token axis second to last), table [N, hd / 2, 2] -> [c -s; s c] on the interleaved pairs."""
    x0, x1 = t[..., 0::2], t[..., 1::2]
    c, s = table[:, :, 0], table[:, :, 1]
    return torch.stack((x0 * c - x1 * s, x0 * s + x1 * c), dim=-1).flatten(-2)


def rotate_t(g, table):
    """The transposed map [c s; -s c]: the backward of rotate."""
    g0, g1 = g[..., 0::2], g[..., 1::2]
    c, s = table[:, :, 0], table[:, :, 1]
    return torch.stack((g0 * c + g1 * s, g1 * c - g0 * s), dim=-1).flatten(-2)


def rotate_complex(t, table):
    """The same map as a complex multiplication, RoPE-ViT's statement: view_as_complex of the pairs times c + i s."""
    z = torch.view_as_complex(t.reshape(*t.shape[:-1], -1, 2).contiguous())
    w = torch.view_as_complex(table.contiguous())
    return torch.view_as_real(z * w).flatten(-2)


def attention(qkv, H, rope, qk_norm=None, eps=1e-6, attn_mask=None, rel_bias=None, ma=None):
    """softmax(R LN(q) (R LN(k))^T / sqrt(hd) [+ mask] [+ bias]) [* ma] v -> ([B, N, D], probabilities [B, H, N, N]); LN only with
    qk_norm, R the rotation by `rope` [N, hd / 2, 2]."""
    B, N, D3 = qkv.shape
    hd = D3 // 3 // H
    if qk_norm is not None:
        q, k, v = qk_norm_ref.qk_normed(qkv, H, qk_norm, eps)
    else:
        t = qkv.reshape(B, N, 3, H, hd)
        q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
    q, k = rotate(q, rope), rotate(k, rope)
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    if attn_mask is not None:
        sc = sc + attn_mask
    if rel_bias is not None:
        sc = sc + rel_bias
    p = torch.softmax(sc, -1)
    pm = p if ma is None else p * ma
    return (pm @ v).transpose(1, 2).reshape(B, N, D3 // 3), p


def encoder_layer(x, P, H, masks, c1, c2, attn_mask=None, eps=1e-5, qk_norm=None, qk_eps=1e-6, rel_bias=None, rope=None):
    """Post-norm layer: qk_norm_ref.encoder_layer, with the rotation of q and k when rope [N, hd / 2, 2] is given."""
    if rope is None:
        return qk_norm_ref.encoder_layer(x, P, H, masks, c1, c2, attn_mask, eps, qk_norm, qk_eps, rel_bias)
    ma, m1, mf, m2 = masks
    qkv = x @ P["in_w"].t() + P["in_b"]
    o, _ = attention(qkv, H, rope, qk_norm, qk_eps, attn_mask, rel_bias, ma)
    a = (o @ P["out_w"].t() + P["out_b"]) * m1
    x1 = _ln(x + c1[:, None, None] * a, P["n1_w"], P["n1_b"], eps)
    h = torch.relu(x1 @ P["w1"].t() + P["b1"]) * mf
    f = (h @ P["w2"].t() + P["b2"]) * m2
    return _ln(x1 + c2[:, None, None] * f, P["n2_w"], P["n2_b"], eps)


def pre_norm_layer(s, n, P, H, masks=None, c1=None, c2=None, lam=None, act="relu", attn_mask=None, rel_bias=None, eps=1e-5,
                   keep=None, qk_norm=None, qk_eps=1e-6, rope=None):
    """Pre-norm layer: qk_norm_ref.pre_norm_layer, with the rotation of q and k when rope [N, hd / 2, 2] is given."""
    if rope is None:
        return qk_norm_ref.pre_norm_layer(s, n, P, H, masks, c1, c2, lam, act, attn_mask, rel_bias, eps, keep, qk_norm, qk_eps)
    B, N, D = s.shape
    one = s.new_ones(())
    ma, m1, mf, m2 = masks if masks is not None else (one, one, one, one)
    c1 = s.new_ones(B) if c1 is None else c1
    c2 = s.new_ones(B) if c2 is None else c2
    l1, l2 = lam if lam is not None else (one, one)
    qkv = n @ P["in_w"].t() + P["in_b"]
    o, _ = attention(qkv, H, rope, qk_norm, qk_eps, attn_mask, rel_bias, ma)
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
def _rows(table, M):
    """table [N, hd / 2, 2] -> [M, 1, 1, hd / 2, 2]: row m uses table row m mod N."""
    N = table.shape[0]
    return table.double()[torch.arange(M, device=table.device) % N][:, None, None]


def forward64(qkv, table, H, hd, hp):
    """fp64 rotation of a packed bf16 buffer [M, 3 H hp] -> fp64 [M, 3, H, hp]: q, k rotated over their hd real columns with zeros
    behind, v as it is.  table: fp32 [N, hd / 2, 2] on the buffer's device."""
    t = heads(qkv.double(), H, hp, 3).clone()
    cs = _rows(table, t.shape[0])
    x0, x1 = t[:, :2, :, 0:hd:2], t[:, :2, :, 1:hd:2]
    c, s = cs[..., 0], cs[..., 1]
    y = torch.stack((x0 * c - x1 * s, x0 * s + x1 * c), dim=-1).flatten(-2)
    t[:, :2, :, :hd] = y
    t[:, :2, :, hd:] = 0
    return t


def backward64(dy, table, H, hd, hp):
    """fp64 backward on the kernel's own inputs: dy [M, 3 H hp] (q | k thirds used) -> dx [M, 2, H, hp], zeros in the padding."""
    g = heads(dy.double(), H, hp, 3)[:, :2]
    cs = _rows(table, g.shape[0])
    g0, g1 = g[..., 0:hd:2], g[..., 1:hd:2]
    c, s = cs[..., 0], cs[..., 1]
    out = torch.zeros(dy.shape[0], 2, H, hp, dtype=torch.float64, device=dy.device)
    out[..., :hd] = torch.stack((g0 * c + g1 * s, g1 * c - g0 * s), dim=-1).flatten(-2)
    return out


CS_VALUES = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)


def exact_inputs(B, N, H, hd, seed=0):
    """The exact-answer case -> x [M, 2 H, hd] and dy [M, 2 H, hd] integers in [-4, 4], table [N, hd / 2, 2] with (c, s) drawn per
    (token, pair) from {0, +-1/2, +-1, +-2}^2 -- deliberately no rotations: the kernel applies [c -s; s c] as given.  Every output
    x0 c -+ x1 s is then a multiple of 1/2 of magnitude at most 16: exact in bf16 (6 significant bits), and column sums of a few
    hundred such rows are exact in fp32 in any order."""
    g = torch.Generator().manual_seed(4000 + 97 * seed + 13 * B + N + 31 * H + hd)
    M = B * N
    x = torch.randint(-4, 5, (M, 2 * H, hd), generator=g).float()
    dy = torch.randint(-4, 5, (M, 2 * H, hd), generator=g).float()
    table = torch.tensor(CS_VALUES)[torch.randint(0, len(CS_VALUES), (N, hd // 2, 2), generator=g)]
    return x, dy, table.contiguous()


def exact_answers(x, dy, table):
    """-> (y, dx) [M, 2 H, hd] fp32 of exact_inputs, exact by construction (every product and sum is exact in fp32)."""
    M, N = x.shape[0], table.shape[0]
    cs = table[torch.arange(M) % N][:, None]                   # [M, 1, hd / 2, 2]
    c, s = cs[..., 0], cs[..., 1]
    x0, x1, g0, g1 = x[..., 0::2], x[..., 1::2], dy[..., 0::2], dy[..., 1::2]
    y = torch.stack((x0 * c - x1 * s, x0 * s + x1 * c), dim=-1).flatten(-2)
    dx = torch.stack((g0 * c + g1 * s, g1 * c - g0 * s), dim=-1).flatten(-2)
    return y, dx
