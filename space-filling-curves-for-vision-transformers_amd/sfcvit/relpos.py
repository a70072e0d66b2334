"""Bucket-index builders for the learned relative position bias (include/sfcvit.h, "Self-attention core with a learned
relative position bias").  Every builder returns (index, n_buckets): an int32 CPU tensor [N, N] whose entry
(i, j) names the bucket of head h's table that query i adds to its score for key j -- or -1 where the pair is hidden, which
is how a window is expressed -- and the number of buckets T.  sfcvit.ops.AttentionBiasIndex validates the pair.

The two kinds are the two views this repository compares everywhere: `curve_offsets` takes the offset along the token
sequence (the Hilbert, Z or raster order), `image_offsets` the 2-D displacement of the token centres in the image,
whatever the order.
"""
import torch


def curve_offsets(n_tokens, window=None):
    """Bucket j - i + (N - 1), T = 2 N - 1.  window=w: bucket j - i + w, T = 2 w + 1, and -1 where |i - j| > w."""
    n = int(n_tokens)
    if n < 1:
        raise ValueError(f"curve_offsets: n_tokens={n_tokens} (>= 1)")
    i = torch.arange(n, dtype=torch.int32)
    d = i[None, :] - i[:, None]                                 # d[i, j] = j - i
    if window is None:
        return (d + (n - 1)).contiguous(), 2 * n - 1
    w = int(window)
    if w < 0:
        raise ValueError(f"curve_offsets: window={window} (>= 0)")
    index = d + w
    index[d.abs() > w] = -1
    return index.contiguous(), 2 * w + 1


def image_offsets(positions, cell, radius=None):
    """positions: the [N, 2] (row, col) token centres of sfcvit.analysis.token_positions, in pixels; cell: the pixel pitch
    the displacement is counted in.  d = round((pos_j - pos_i) / cell) per axis, bucket (d_row + R) (2 R + 1) + (d_col + R)
    with R the largest |d| present, T = (2 R + 1)^2.  radius: -1 where max(|d row|, |d col|) in pixels exceeds it (the
    window of sfcvit.masks.image_window)."""
    pos = torch.as_tensor(positions, dtype=torch.float64).cpu()
    if pos.dim() != 2 or pos.shape[1] != 2 or pos.shape[0] < 1:
        raise ValueError(f"image_offsets: positions must be [N, 2], got {tuple(pos.shape)}")
    if not cell > 0:
        raise ValueError(f"image_offsets: cell={cell} (> 0)")
    if radius is not None and not radius >= 0:
        raise ValueError(f"image_offsets: radius={radius} (>= 0)")
    delta = pos[None, :, :] - pos[:, None, :]                   # delta[i, j] = pos_j - pos_i
    d = torch.round(delta / float(cell)).to(torch.int64)
    R = int(d.abs().max())
    index = ((d[..., 0] + R) * (2 * R + 1) + (d[..., 1] + R)).to(torch.int32)
    if radius is not None:
        index[delta.abs().amax(dim=-1) > float(radius)] = -1
    return index.contiguous(), (2 * R + 1) ** 2


def with_cls_token(index, n_buckets):
    """An [N, N] index carried to the N + 1 tokens of a model built with pool="cls": the CLS token is row 0 and column 0
    and gets three buckets of its own, as in BEiT -- n_buckets: CLS to a patch token, n_buckets + 1: a patch token to CLS,
    n_buckets + 2: CLS to CLS -- so it sees and is seen by every token; the patch tokens keep their buckets, shifted by one
    row and column.  -> (index [N + 1, N + 1], n_buckets + 3)."""
    index = torch.as_tensor(index)
    if index.dim() != 2 or index.shape[0] != index.shape[1] or index.is_floating_point():
        raise ValueError(f"with_cls_token: a square integer [N, N] index is expected, got {index.dtype} {tuple(index.shape)}")
    n, T = index.shape[0], int(n_buckets)
    out = torch.empty((n + 1, n + 1), dtype=torch.int32)
    out[1:, 1:] = index.to("cpu", torch.int32)
    out[0, 1:] = T
    out[1:, 0] = T + 1
    out[0, 0] = T + 2
    return out, T + 3


def bucket_offsets(kind, n_buckets, n_tokens=None, window=None, cls_token=False):
    """What each bucket of a table means: a list of n_buckets entries -- for kind "curve" the offset j - i along the sequence
    (an int), for "image" the displacement (d_row, d_col) in cells -- with "cls->token", "token->cls" and "cls->cls" for the
    three buckets with_cls_token adds."""
    T = int(n_buckets) - (3 if cls_token else 0)
    if kind == "curve":
        half = int(window) if window is not None else int(n_tokens) - 1
        if T != 2 * half + 1:
            raise ValueError(f"bucket_offsets: {T} buckets do not belong to a curve index of half-width {half}")
        out = [t - half for t in range(T)]
    elif kind == "image":
        side = int(round(T ** 0.5))
        if side * side != T or side % 2 == 0:
            raise ValueError(f"bucket_offsets: {T} buckets are not (2 R + 1)^2")
        R = side // 2
        out = [(t // side - R, t % side - R) for t in range(T)]
    else:
        raise ValueError(f"bucket_offsets: kind={kind!r}: 'curve' or 'image' expected")
    return out + (["cls->token", "token->cls", "cls->cls"] if cls_token else [])
