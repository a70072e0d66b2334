"""Masked attention without a GPU: mask validation and the block map (sfcvit_attention_mask_blocks) against a numpy
restatement, the mask builders, the refusals of sfcvit_attention_masked_fwd / _bwd (decided before any HIP call), and the
model surface (attn_mask= leaves state_dict alone)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from attn_mask_ref import block_map_ref, random_mask

EINVAL = 1
WINDOWS = [(4, 1, 1, 1), (70, 1, 4, 4), (130, 40, 7, 9), (196, 32, 10, 16), (576, 64, 25, 81)]     # N, w, visited, total


def _blocks(mask):
    """(return code, message, map) of the C function on an exactly-sized numpy buffer."""
    from sfcvit._lib import lib
    m = np.ascontiguousarray(mask.numpy(), dtype=np.float32)
    N = m.shape[0]
    nb = (N + 63) // 64
    out = np.full((nb, nb), 7, dtype=np.uint8)
    rc = lib.sfcvit_attention_mask_blocks(ctypes.c_void_p(m.ctypes.data), N, ctypes.c_void_p(out.ctypes.data))
    return rc, lib.sfcvit_last_error().decode(), out


@pytest.mark.parametrize("N,w,visited,total", WINDOWS)
def test_block_map_of_curve_windows(N, w, visited, total):
    from sfcvit import masks, ops
    m = masks.curve_window(N, w)
    i = np.arange(N)
    want = np.where(np.abs(i[:, None] - i[None, :]) <= w, 0.0, -np.inf).astype(np.float32)
    assert m.dtype == torch.float32 and not m.is_cuda and np.array_equal(m.numpy(), want)
    rc, msg, got = _blocks(m)
    assert rc == 0, msg
    ref = block_map_ref(m)
    assert np.array_equal(got, ref), (got, ref)
    assert int((got != 0).sum()) == visited and got.size == total
    # value 2 exactly where a block is all zero
    for bi in range(got.shape[0]):
        for bj in range(got.shape[1]):
            tile = want[bi * 64:(bi + 1) * 64, bj * 64:(bj + 1) * 64]
            assert (got[bi, bj] == 2) == bool((tile == 0).all()), (bi, bj)
    holder = ops.AttentionMask(m)
    assert (holder.visited_blocks, holder.total_blocks, holder.n_tokens) == (visited, total, N)
    assert np.array_equal(holder.block_map.numpy(), ref)


def test_block_map_of_an_image_window_on_hilbert_positions():
    from sfcvit import masks, ops
    from sfcvit.analysis import token_positions
    from sfcvit.tokenizers import HilbertEmbedding1D
    pos = token_positions(HilbertEmbedding1D(224, 256, 3, 8))          # 14 x 14 tokens of 16 x 16 pixels in Hilbert order
    assert tuple(pos.shape) == (196, 2)
    m = masks.image_window(pos, 32)                                    # two tokens each way: at most 5 x 5 visible
    p = pos.numpy().astype(np.float64)
    d = np.abs(p[:, None, :] - p[None, :, :]).max(axis=-1)
    assert np.array_equal(np.isfinite(m.numpy()), d <= 32)
    vis = np.isfinite(m.numpy()).sum(axis=1)
    assert vis.min() == 9 and vis.max() == 25 and np.array_equal(m.numpy(), m.numpy().T)
    rc, msg, got = _blocks(m)
    assert rc == 0, msg
    assert np.array_equal(got, block_map_ref(m))
    holder = ops.AttentionMask(m)
    assert holder.visited_blocks == int((got != 0).sum()) and holder.total_blocks == 16


def test_block_map_of_a_random_mask_and_of_finite_biases():
    m, hidden = random_mask(130, 0.3, seed=3)
    assert not torch.isfinite(m[:, hidden]).any() and int(torch.isfinite(m[0]).sum()) == 1 and bool(torch.isfinite(m[0, 129]))
    rc, msg, got = _blocks(m)
    assert rc == 0, msg
    assert np.array_equal(got, block_map_ref(m))
    sparse = torch.full((200, 200), float("-inf"))
    sparse[:, 0] = 0.0                                                 # one visible key: key blocks 1 .. 3 are never visited
    sparse[70, 199] = -2.5                                             # a finite non-zero entry makes its block mixed
    sparse[130:192, 128:192] = 0.0
    rc, msg, got = _blocks(sparse)
    assert rc == 0, msg
    assert np.array_equal(got, block_map_ref(sparse))
    assert got.tolist() == [[1, 0, 0, 0], [1, 0, 0, 1], [1, 0, 1, 0], [1, 0, 0, 0]]
    zero = torch.zeros(64, 64)
    zero[3, 5] = -0.0                                                  # -0.0 adds nothing: still an all-zero block
    assert _blocks(zero)[2].tolist() == [[2]]
    zero[3, 5] = 1e-30
    assert _blocks(zero)[2].tolist() == [[1]]


def test_refusals_each_with_its_message():
    from sfcvit import ops
    from sfcvit._lib import lib
    m = torch.zeros(70, 70)
    m[69, 3] = float("nan")
    rc, msg, _ = _blocks(m)
    assert rc == EINVAL and "NaN" in msg and "row 69" in msg
    m[69, 3] = float("inf")
    rc, msg, _ = _blocks(m)
    assert rc == EINVAL and "+inf" in msg and "row 69" in msg
    m[69, :] = float("-inf")
    rc, msg, _ = _blocks(m)
    assert rc == EINVAL and "row 69 " in msg and "no finite entry" in msg
    with pytest.raises(ValueError, match="row 69 has no finite entry"):
        ops.AttentionMask(m)
    one = np.zeros(1, dtype=np.float32)
    out = np.zeros(1, dtype=np.uint8)
    pm, po = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    for N in (0, -1, 4097):
        assert lib.sfcvit_attention_mask_blocks(pm, N, po) == EINVAL
        assert f"N={N}" in lib.sfcvit_last_error().decode()
    assert lib.sfcvit_attention_mask_blocks(None, 1, po) == EINVAL and "null" in lib.sfcvit_last_error().decode()
    assert lib.sfcvit_attention_mask_blocks(pm, 1, None) == EINVAL and "null" in lib.sfcvit_last_error().decode()
    with pytest.raises(ValueError, match="CPU fp32"):
        ops.AttentionMask(torch.zeros(4, 5))
    with pytest.raises(ValueError, match="CPU fp32"):
        ops.AttentionMask(torch.zeros(4, 4, dtype=torch.float64))


def test_n_4096_is_accepted():
    from sfcvit import masks, ops
    holder = ops.AttentionMask(masks.curve_window(4096, 0))            # the diagonal alone
    assert (holder.visited_blocks, holder.total_blocks) == (64, 4096)


def test_from_bool_follows_torchs_convention():
    """True = may NOT attend.  nn.TransformerEncoderLayer gives equal outputs for the bool form and for from_bool's float
    form of one window, and differs from the unmasked layer."""
    from sfcvit import masks
    N, w = 12, 2
    m = masks.curve_window(N, w)
    blocked = ~torch.isfinite(m)
    assert torch.equal(masks.from_bool(blocked), m)
    torch.manual_seed(0)
    layer = nn.TransformerEncoderLayer(32, 2, 64, dropout=0.0, batch_first=True).eval()
    x = torch.randn(2, N, 32)
    with torch.no_grad():
        y_bool, y_float, y_none = layer(x, src_mask=blocked), layer(x, src_mask=masks.from_bool(blocked)), layer(x)
    assert torch.allclose(y_bool, y_float, atol=1e-6, rtol=0)
    assert not torch.allclose(y_bool, y_none, atol=1e-3)
    with pytest.raises(ValueError):
        masks.from_bool(torch.zeros(3, 3))
    with pytest.raises(ValueError):
        masks.curve_window(0, 1)


def _masked_args(**over):
    from sfcvit import _lib
    a = _lib.AttnMaskArgs()
    for name in ("qkv", "out", "lse", "dout", "dqkv", "delta", "mask", "block_map"):
        setattr(a, name, 0x100000)                    # never dereferenced: the checks decide first
    a.B, a.N, a.H, a.hd, a.scale, a.dropout_p = 2, 130, 2, 64, 0.125, 0.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("entry", ["sfcvit_attention_masked_fwd", "sfcvit_attention_masked_bwd"])
@pytest.mark.parametrize("over,frag", [({"hd": 128}, "head dim 128"), ({"hd": 32}, "head dim 32"), ({"mask": None}, "null"),
                                       ({"block_map": None}, "null"), ({"qkv": None}, "null"), ({"dropout_p": 1.0}, "dropout_p"),
                                       ({"dropout_p": -0.5}, "dropout_p"), ({"N": 0}, "N=0"), ({"N": 4097}, "N=4097"),
                                       ({"qkv": 0x100008}, "aligned"), ({"mask": 0x100004}, "aligned")])
def test_entry_points_refuse_bad_arguments_without_a_device(entry, over, frag):
    from sfcvit._lib import lib
    fn = getattr(lib, entry)
    assert fn(ctypes.byref(_masked_args(**over)), None) == EINVAL
    assert frag in lib.sfcvit_last_error().decode(), lib.sfcvit_last_error().decode()
    assert fn(None, None) == EINVAL


def test_backward_refuses_null_gradient_tensors_and_short_colsum_workspace():
    from sfcvit._lib import lib
    assert lib.sfcvit_attention_masked_bwd(ctypes.byref(_masked_args(dout=None)), None) == EINVAL
    assert "null" in lib.sfcvit_last_error().decode()
    assert lib.sfcvit_attention_masked_bwd(ctypes.byref(_masked_args(colsum_out=0x100000, colsum_part=0x100000, colsum_part_bytes=16)), None) == EINVAL
    assert "colsum" in lib.sfcvit_last_error().decode()


def test_state_dict_keys_do_not_change_with_a_mask():
    from oracle.cases import MODEL_CASES
    from sfcvit import masks, ops
    from sfcvit.models import VisionTransformer, VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    cfg, _ = MODEL_CASES["hilbert32_1d"]
    for cls in (VisionTransformer1D, VisionTransformer):
        torch.manual_seed(1)
        plain = cls(HilbertEmbedding1D(32, 4, 3, 128), depth=cfg.depth, n_heads=cfg.n_heads, mlp_dim=cfg.mlp_dim)
        torch.manual_seed(1)
        masked = cls(HilbertEmbedding1D(32, 4, 3, 128), depth=cfg.depth, n_heads=cfg.n_heads, mlp_dim=cfg.mlp_dim,
                     attn_mask=masks.curve_window(256, 8))
        a, b = plain.state_dict(), masked.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        assert plain.attn_mask is None and isinstance(masked.attn_mask, ops.AttentionMask)
        assert (masked.attn_mask.visited_blocks, masked.attn_mask.total_blocks) == (10, 16)
        assert not any("mask" in k for k in b) and not any("mask" in k for k, _ in masked.named_buffers())
        plain.load_state_dict(b)
    # a bool mask (True = blocked) and an AttentionMask are taken as well; a wrong size is refused at construction
    blocked = ~torch.isfinite(masks.curve_window(256, 8))
    m = VisionTransformer1D(HilbertEmbedding1D(32, 4, 3, 128), depth=1, n_heads=2, attn_mask=blocked)
    assert torch.equal(m.attn_mask.mask, masks.curve_window(256, 8))
    with pytest.raises(ValueError, match="256"):
        VisionTransformer1D(HilbertEmbedding1D(32, 4, 3, 128), depth=1, n_heads=2, attn_mask=masks.curve_window(64, 8))


def test_main_py_window_flags_are_mutually_exclusive():
    """Decided by argparse, before any device is touched."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = os.path.join(root, "space-filling-curves-for-vision-transformers_amd", "main.py")
    out = subprocess.run([sys.executable, main, "--synthetic", "--attn-window", "8", "--attn-window-2d", "4"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 2 and "not allowed with" in out.stderr, out.stderr[-2000:]
