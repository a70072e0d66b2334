"""Containment of the relative-position-bias attention kernels, in the shape of tests/test_containment_gpu.py (its `contain`):
forward and backward through the C ABI with every buffer -- qkv, out, lse, dout, dqkv, delta, the block map, index, table,
offsets, positions, dtable, the table gradient's workspace and the column sums -- inside guarded allocations
(tests/guarded.py).  Guards intact, every output written and torch.equal to the plain run, inputs unchanged, and the same
outputs whether the workspaces held 0xFF or 0x00 before the call.  No tolerance: byte patterns and torch.equal only."""
import ctypes
import math

import pytest
import torch

from test_containment_gpu import SEED, _name, _rand, _stream, contain

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def L():
    from sfcvit import _lib
    return _lib


def _args(L, t, B, N, H, T, visited, p):
    a = L.AttnBiasArgs()
    for k in ("qkv", "out", "lse", "dout", "dqkv", "delta", "colsum_part", "colsum_out", "block_map", "index", "table", "offsets",
              "positions", "dtable", "workspace"):
        if k in t:
            setattr(a, k, t[k].data_ptr())
    if "colsum_part" in t:
        a.colsum_part_bytes = t["colsum_part"].numel()
        a.colsum_bf16 = int(t["colsum_out"].dtype == BF16)
    if "workspace" in t:
        a.workspace_bytes = t["workspace"].numel()
    a.B, a.N, a.H, a.hd, a.scale, a.T, a.visited_blocks = B, N, H, 64, 1.0 / math.sqrt(64), T, visited
    a.dropout_p, a.dropout_seed = p, SEED
    return a


@pytest.mark.parametrize("N,kind", [(70, "w20"), (130, "w20"), (130, "cls")])
def test_attention_bias_forward_and_backward(L, N, kind):
    """curve_offsets(N, 20): at N = 130 the corner blocks of the 3 x 3 map are skipped.  "cls": with_cls_token over a window of
    5, every block visited through the CLS row and column, three extra buckets."""
    from sfcvit import ops, relpos
    lib = L.lib
    B, H = 2, 2
    D = H * 64
    index, T = relpos.curve_offsets(N, 20) if kind == "w20" else relpos.with_cls_token(*relpos.curve_offsets(N - 1, 5))
    holder = ops.AttentionBiasIndex(index, T)
    assert (N, kind) != (130, "w20") or (int(holder.block_map[0, 2]) == 0 and holder.visited_blocks == 7)
    g = torch.Generator().manual_seed(70 + N)
    qkv, dout = _rand(g, B, N, 3 * D), _rand(g, B, N, D)
    table = 0.5 * torch.randn(H, T, generator=g)
    static = dict(block_map=holder.block_map, index=holder.index, table=table)
    last = lambda: _name(lib.sfcvit_last_attn_kernel)                                       # noqa: E731
    for p in (0.0, 0.1):
        what = f"bias N={N} {kind} p={p}"

        def run_fwd(t):
            L.check(lib.sfcvit_attention_bias_fwd(ctypes.byref(_args(L, t, B, N, H, T, holder.visited_blocks, p)), _stream()), what + " forward")

        f = contain(what + " forward", run_fwd, dict(qkv=qkv, **static), {"out": ((B, N, D), BF16), "lse": ((B, H, N), F32)},
                    last_kernel=last, expect="attn_bias_fwd_kernel")

        def run_bwd(t):
            L.check(lib.sfcvit_attention_bias_bwd(ctypes.byref(_args(L, t, B, N, H, T, holder.visited_blocks, p)), _stream()), what + " backward")

        inputs = dict(qkv=qkv, dout=dout, out=f["out"], lse=f["lse"], offsets=holder.offsets, positions=holder.positions, **static)
        ws = {"delta": B * H * N * 4, "workspace": lib.sfcvit_attention_bias_workspace(B, N, H, holder.visited_blocks)}
        outs = {"dqkv": ((B, N, 3 * D), BF16), "dtable": ((H, T), F32)}
        b0 = contain(what + " backward", run_bwd, inputs, outs, ws, last_kernel=last, expect="attn_bias_bwd_kv_kernel")
        for cdt in (F32, BF16):
            ws2 = dict(ws, colsum_part=lib.sfcvit_attention_colsum_workspace(B, N, H, 64))
            b1 = contain(f"{what} backward + column sums {cdt}", run_bwd, inputs, dict(outs, colsum_out=((3 * D,), cdt)), ws2,
                         last_kernel=last, expect="attn_bias_bwd_kv_kernel")
            assert torch.equal(b1["dqkv"], b0["dqkv"]) and torch.equal(b1["dtable"], b0["dtable"]), what + ": gradients change with the column sums"
