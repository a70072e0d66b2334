"""Table builders for rotary position embeddings (include/sfcvit.h, "RoPE").  Every builder returns an fp32 CPU
tensor [N, head_dim / 2, 2]: row n, pair p holds (cos, sin) of the angle by which the channel pair (2 p, 2 p + 1) of every
query and key head row of token n is rotated.  The angles are formed and their cos / sin taken in fp64 and rounded once to
fp32.  sfcvit.ops.RopeTable validates a table and keeps its device copy.

The two kinds are the two views this repository compares everywhere: `curve_table` rotates by the index along the token
sequence (the Hilbert, Z or raster order), so q_i . k_j depends on the offset j - i along the curve; `image_table` rotates
half of the pairs by the column and half by the row of the token centre in the image, whatever the order, so the score
depends on the 2-D displacement (the axial form of RoPE-ViT).
"""
import math

import torch


def _base(what, base):
    base = float(base)
    if not (math.isfinite(base) and base > 0.0):
        raise ValueError(f"{what}: base={base} (finite, > 0)")
    return base


def _table(theta):
    return torch.stack((torch.cos(theta), torch.sin(theta)), dim=-1).to(torch.float32).contiguous()


def curve_table(n_tokens, head_dim, base=10000.0):
    """theta[n, p] = n * base^(-2 p / head_dim), n the index along the token sequence -> [N, head_dim / 2, 2]."""
    n, hd = int(n_tokens), int(head_dim)
    if n < 1:
        raise ValueError(f"curve_table: n_tokens={n_tokens} (>= 1)")
    if hd < 2 or hd % 2:
        raise ValueError(f"curve_table: head_dim={head_dim} must be even and >= 2: channels rotate in pairs")
    base = _base("curve_table", base)
    p = torch.arange(hd // 2, dtype=torch.float64)
    freq = torch.pow(torch.tensor(base, dtype=torch.float64), -2.0 * p / hd)
    return _table(torch.arange(n, dtype=torch.float64)[:, None] * freq[None, :])


def image_table(positions, cell, head_dim, base=100.0):
    """positions: the [N, 2] (row, col) token centres of sfcvit.analysis.token_positions, in pixels; cell: the pixel pitch the
    coordinates are counted in.  f_j = base^(-4 j / head_dim) for j < head_dim / 4; pairs 0 .. head_dim / 4 - 1 rotate by
    col / cell * f_j, pairs head_dim / 4 .. head_dim / 2 - 1 by row / cell * f_j.  head_dim % 4 == 0."""
    pos = torch.as_tensor(positions, dtype=torch.float64).cpu()
    if pos.dim() != 2 or pos.shape[1] != 2 or pos.shape[0] < 1:
        raise ValueError(f"image_table: positions must be [N, 2], got {tuple(pos.shape)}")
    if not bool(torch.isfinite(pos).all()):
        raise ValueError("image_table: positions hold a non-finite entry")
    cell = float(cell)
    if not (math.isfinite(cell) and cell > 0.0):
        raise ValueError(f"image_table: cell={cell} (finite, > 0)")
    hd = int(head_dim)
    if hd < 4 or hd % 4:
        raise ValueError(f"image_table: head_dim={head_dim} must be a multiple of 4: half of the pairs turn with the column, "
                         "half with the row")
    base = _base("image_table", base)
    j = torch.arange(hd // 4, dtype=torch.float64)
    freq = torch.pow(torch.tensor(base, dtype=torch.float64), -4.0 * j / hd)
    row, col = pos[:, 0] / cell, pos[:, 1] / cell
    return _table(torch.cat((col[:, None] * freq[None, :], row[:, None] * freq[None, :]), dim=1))


def with_cls_token(table):
    """A table for N tokens carried to the N + 1 tokens of a model built with pool="cls": the CLS token is row 0 and gets the
    identity (1, 0) in every pair -- it is not rotated; the patch tokens keep their rows, shifted by one."""
    table = torch.as_tensor(table)
    if table.dim() != 3 or table.shape[2] != 2 or not table.is_floating_point():
        raise ValueError(f"with_cls_token: a floating [N, head_dim / 2, 2] table is expected, got {table.dtype} {tuple(table.shape)}")
    ident = torch.zeros((1, table.shape[1], 2), dtype=torch.float32)
    ident[..., 0] = 1.0
    return torch.cat((ident, table.to("cpu", torch.float32)), dim=0).contiguous()


DEFAULT_BASE = {"curve": 10000.0, "image": 100.0}
