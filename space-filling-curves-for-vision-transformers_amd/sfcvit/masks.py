"""Attention-mask builders.  Every builder returns an additive fp32 CPU tensor [N, N]: 0 where query i may attend to key
j, -inf where it may not -- the form sfcvit.ops.AttentionMask validates and the masked attention kernels read
(include/sfcvit.h, "Masked / windowed self-attention core").

Two windows answer the question this repository exists for: `curve_window` keeps neighbours along the token sequence
(the Hilbert, Z or raster order), `image_window` keeps a true 2-D neighbourhood in the image whatever the order.
"""
import torch

_NEG_INF = float("-inf")


def _additive(visible):
    out = torch.full(visible.shape, _NEG_INF, dtype=torch.float32)
    out[visible] = 0.0
    return out


def curve_window(n_tokens, w):
    """0 where |i - j| <= w along the token sequence, -inf elsewhere."""
    n_tokens, w = int(n_tokens), int(w)
    if n_tokens < 1 or w < 0:
        raise ValueError(f"curve_window: n_tokens={n_tokens} (>= 1), w={w} (>= 0)")
    i = torch.arange(n_tokens)
    return _additive((i[:, None] - i[None, :]).abs() <= w)


def image_window(positions, radius):
    """0 where max(|d row|, |d col|) <= radius between the token centres, -inf elsewhere.  positions: the [N, 2] (row, col)
    tensor of sfcvit.analysis.token_positions; radius in pixels, as the distances of the attention report."""
    pos = torch.as_tensor(positions, dtype=torch.float32).cpu()
    if pos.dim() != 2 or pos.shape[1] != 2:
        raise ValueError(f"image_window: positions must be [N, 2], got {tuple(pos.shape)}")
    if not radius >= 0:
        raise ValueError(f"image_window: radius={radius} (>= 0)")
    d = (pos[:, None, :] - pos[None, :, :]).abs().amax(dim=-1)
    return _additive(d <= float(radius))


def from_bool(blocked):
    """nn.Transformer's boolean convention: True = query i may NOT attend to key j."""
    blocked = torch.as_tensor(blocked)
    if blocked.dtype != torch.bool or blocked.dim() != 2 or blocked.shape[0] != blocked.shape[1]:
        raise ValueError(f"from_bool: a square bool matrix is expected, got {blocked.dtype} {tuple(blocked.shape)}")
    return _additive(~blocked.cpu())


def with_cls_token(mask):
    """An [N, N] mask (additive float, or bool with True = blocked) carried to the N + 1 tokens of a model built with
    pool="cls": the CLS token (row 0 and column 0) sees every token and is seen by every token, and the patch tokens keep
    their mask, shifted by one.  -> additive fp32 [N + 1, N + 1]."""
    mask = torch.as_tensor(mask)
    if mask.dim() != 2 or mask.shape[0] != mask.shape[1]:
        raise ValueError(f"with_cls_token: a square [N, N] mask is expected, got {tuple(mask.shape)}")
    if mask.dtype == torch.bool:
        mask = from_bool(mask)
    elif not mask.is_floating_point():
        raise ValueError(f"with_cls_token: a float additive or a bool mask is expected, got {mask.dtype}")
    n = mask.shape[0]
    out = torch.zeros((n + 1, n + 1), dtype=torch.float32)
    out[1:, 1:] = mask.detach().to("cpu", torch.float32)
    return out
