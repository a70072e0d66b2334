"""Containment of the GEMM, attention, row-wise and tokenizer kernels: nothing is read or written outside the buffers of a
call, every output element is written, and no result depends on what a workspace held before the call.

Every case runs the C ABI (sfcvit._lib) twice or three times: once on ordinary dense tensors (the plain run), then with every
input, output and workspace inside guarded allocations (tests/guarded.py; workspaces pre-filled with 0xFF in one run and 0x00
in another, sized by the library's own queries and not a byte more).  After synchronizing: all guards intact, every output
finite and torch.equal to the plain run, the inputs unchanged, and the same kernel ran as in the plain run (and it is the one
the case is about).  No tolerance appears anywhere: byte patterns and torch.equal only.  Numeric accuracy is the business of
tests/test_kernels_gpu.py, the attention test files and tests/test_tokenizer_kernels_gpu.py.

The tokenizer kernels (pe_fwd_kernel / pe_bwd_kernel / pe_bwd_reduce, pe2_*, the three token gathers and their mixing
instances, hier_fwd_kernel in both forms, hier_resample_concat_kernel / _bwd_kernel) address memory through tables: pixel
tables, tile descriptors, orders, origins, perm and the mix record are guarded INPUTS.  Their 0xFF guards read as -1, an
offset that lands in a guard of the same allocation, so a stray table read shows up as a NaN or a broken guard, never as a
fault.  Every table used is valid for its image.
"""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import tokenizer_ref as TR
from guarded import assert_guards_intact, assert_written, guarded_inout, guarded_input, guarded_output, guarded_workspace

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
NONE, RELU, GELU = 0, 1, 2
SEED = 0x2545F491
ATTN_SWITCHES = ("SFCVIT_ATTN_LONG", "SFCVIT_ATTN_BWD_FUSED", "SFCVIT_ATTN_WIDE_STREAM", "SFCVIT_ATTN_BWD_PERSIST", "SFCVIT_ATTN_DQSUM")


@pytest.fixture(scope="module")
def L():
    from sfcvit import _lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _name(fn):
    buf = ctypes.create_string_buffer(96)
    fn(buf, 96)
    return buf.value.decode()


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF16)


def _bytes(t):
    return t.contiguous().view(-1).view(U8)


def contain(what, launch, inputs, outputs, workspaces=None, inouts=None, last_kernel=None, expect=None):
    """The shape of every case (module docstring).  launch(dict name -> tensor) makes the call(s); inputs / inouts: name ->
    tensor, outputs: name -> (shape, dtype), workspaces: name -> bytes.  Returns the plain run's outputs and inouts."""
    workspaces, inouts = workspaces or {}, inouts or {}
    dense = {k: v.cuda() for k, v in inputs.items()}
    dense.update({k: torch.zeros(s, dtype=d, device="cuda") for k, (s, d) in outputs.items()})
    dense.update({k: torch.zeros(n, dtype=U8, device="cuda") for k, n in workspaces.items()})
    dense.update({k: v.cuda().clone() for k, v in inouts.items()})
    launch(dense)
    torch.cuda.synchronize()
    name0 = last_kernel() if last_kernel else None
    if expect is not None:
        assert name0.startswith(expect), f"{what}: ran {name0}, the case is about {expect}"
    plain = {k: dense[k].clone() for k in list(outputs) + list(inouts)}
    for k in outputs:
        if plain[k].dtype.is_floating_point:
            assert bool(torch.isfinite(plain[k].float()).all()), f"{what}: plain run, '{k}' is not finite"
    for fill in ((0xFF, 0x00) if workspaces else (0xFF,)):
        tag = f"{what} [workspace fill {fill:#04x}]"
        bufs = {k: guarded_input(k, v) for k, v in inputs.items()}
        bufs.update({k: guarded_output(k, s, d) for k, (s, d) in outputs.items()})
        bufs.update({k: guarded_workspace(k, n, fill) for k, n in workspaces.items()})
        bufs.update({k: guarded_inout(k, v) for k, v in inouts.items()})
        launch({k: b.t for k, b in bufs.items()})
        torch.cuda.synchronize()
        assert_guards_intact(bufs.values(), tag)
        for k in outputs:
            assert_written(bufs[k], tag)
            assert torch.equal(_bytes(bufs[k].t), _bytes(plain[k])), f"{tag}: '{k}' differs from the plain run"
        for k in inouts:
            assert torch.equal(_bytes(bufs[k].t), _bytes(plain[k])), f"{tag}: '{k}' differs from the plain run"
        for k, v in inputs.items():
            assert torch.equal(_bytes(bufs[k].t), _bytes(v.cuda())), f"{tag}: input '{k}' was written"
        if last_kernel:
            assert last_kernel() == name0, f"{tag}: ran {last_kernel()}, the plain run {name0}"
    return plain


# ---- GEMM --------------------------------------------------------------------------------------------------------------------
def _gemm_case(L, what, M, N, K, mode, expect, akm=False, bkm=False, bias=False, residual=False, act=NONE, dact=NONE, aux_out=False,
               c_f32=False, splitk=1, dropout=0.0, colsum=None, actmask=False):
    lib = L.lib
    g = torch.Generator().manual_seed(1000 + M + 3 * N + 7 * K)
    inputs = {"a": _rand(g, *((K, M) if akm else (M, K))), "b": _rand(g, *((K, N) if bkm else (N, K)), scale=K ** -0.5)}
    outputs = {"c": ((M, N), F32 if c_f32 else BF16)}
    workspaces = {}
    if bias:
        inputs["bias"] = _rand(g, N)
    if residual:
        inputs["residual"] = _rand(g, M, N)
    if dact:
        inputs["aux_in"] = _rand(g, M, N)
    if aux_out:
        outputs["aux_out"] = ((M, N), BF16)
    if actmask and act == RELU:
        outputs["actmask"] = ((M, N // 8), U8)
    elif actmask:                                                # read in place of aux_in: the sign bits of aux_in
        bits = (inputs["aux_in"].float() > 0).view(M, N // 8, 8).to(torch.int32)
        inputs["actmask"] = (bits << torch.arange(8, dtype=torch.int32)).sum(-1).to(U8)
    if colsum is not None:
        outputs["colsum_out"] = ((N,), colsum)
        workspaces["workspace"] = lib.sfcvit_gemm_colsum_workspace(M, N)
    if splitk > 1:
        workspaces["workspace"] = lib.sfcvit_gemm_workspace(M, N, splitk)

    def launch(t):
        a = L.GemmArgs()
        a.a, a.b, a.c = t["a"].data_ptr(), t["b"].data_ptr(), t["c"].data_ptr()
        a.M, a.N, a.K = M, N, K
        a.lda, a.ldb, a.ldc, a.ldr, a.ldaux = (M if akm else K), (N if bkm else K), N, N, N
        a.a_kmajor, a.b_kmajor, a.act, a.dact, a.c_is_f32, a.splitk, a.force_generic = int(akm), int(bkm), act, dact, int(c_f32), splitk, mode
        for k in ("bias", "residual", "aux_in", "aux_out", "colsum_out", "actmask", "workspace"):
            if k in t:
                setattr(a, k, t[k].data_ptr())
        if "workspace" in t:
            a.workspace_bytes = t["workspace"].numel()
        a.ld_actmask, a.colsum_bf16 = N // 8, int(colsum == BF16)
        a.dropout_p, a.dropout_seed = dropout, SEED
        L.check(lib.sfcvit_gemm(ctypes.byref(a), _stream()), what)

    return contain(what, launch, inputs, outputs, workspaces, last_kernel=lambda: _name(lib.sfcvit_last_gemm_kernel), expect=expect)


LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]


@pytest.mark.parametrize("akm,bkm", LAYOUTS, ids=["kc-kc", "kc-km", "km-kc", "km-km"])
def test_gemm_generic_layouts(L, akm, bkm):
    tf = ("false", "true")
    _gemm_case(L, "generic 200x136x328", 200, 136, 328, 1, f"gemm_kernel<{tf[akm]}, {tf[bkm]}, false>", akm=akm, bkm=bkm)


def test_gemm_generic_fewer_rows_than_a_tile_and_n_a_multiple_of_4_only(L):
    _gemm_case(L, "generic 7x132x64", 7, 132, 64, 1, "gemm_kernel<false, false, false>")


def test_gemm_generic_odd_k_with_both_operands_k_major(L):
    _gemm_case(L, "generic 72x40x1001", 72, 40, 1001, 1, "gemm_kernel<true, true, false>", akm=True, bkm=True)


GENERIC_EPILOGUES = {
    "bias+gelu+aux_out": dict(bias=True, act=GELU, aux_out=True),
    "bias+residual": dict(bias=True, residual=True),
    "aux_in+dgelu": dict(dact=GELU),
    "fp32-c": dict(c_f32=True),
    "colsum-fp32": dict(colsum=F32),
    "colsum-bf16": dict(colsum=BF16),
}


@pytest.mark.parametrize("variant", list(GENERIC_EPILOGUES))
def test_gemm_generic_epilogue_buffers(L, variant):
    kw = GENERIC_EPILOGUES[variant]
    heavy = "true" if GELU in (kw.get("act"), kw.get("dact")) else "false"
    _gemm_case(L, "generic 300x264x192 " + variant, 300, 264, 192, 1, f"gemm_kernel<false, false, {heavy}>", **kw)


def test_gemm_generic_relu_writes_the_bit_mask_through_the_separate_pass(L):
    _gemm_case(L, "generic 300x272x192 relu+actmask", 300, 272, 192, 1, "gemm_kernel<false, false, false>", act=RELU, actmask=True)


@pytest.mark.parametrize("c_f32", [False, True], ids=["bf16-c", "fp32-c"])
@pytest.mark.parametrize("M,N,K,splitk,km", [(192, 136, 3000, 5, True), (128, 128, 192, 2, False)],
                         ids=["192x136x3000-s5", "128x128x192-s2-empty-ranges"])
def test_gemm_generic_split_k(L, M, N, K, splitk, km, c_f32):
    """(128, 128, 192) with splitk = 2: one output tile, so the split is rounded up to 8 k-ranges of 64 (one set per XCD)
    and five of them are empty (kbeg >= K); their slabs must come out as zeros, inside the workspace."""
    tf = "true" if km else "false"
    _gemm_case(L, f"generic split-K {M}x{N}x{K}", M, N, K, 1, f"gemm_kernel<{tf}, {tf}, false>", akm=km, bkm=km, splitk=splitk, c_f32=c_f32)


@pytest.mark.parametrize("mode", [4, 6, 7])
@pytest.mark.parametrize("variant", ["bias+residual", "drelu", "splitk4"])
def test_gemm_ring_kernel(L, mode, variant):
    if variant == "splitk4":
        _gemm_case(L, f"ring mode {mode} 256x256x4096 split-K", 256, 256, 4096, mode, "gemm256_kernel<false, false, ", splitk=4)
    else:
        kw = dict(bias=True, residual=True) if variant == "bias+residual" else dict(dact=RELU)
        _gemm_case(L, f"ring mode {mode} 512x384x256 {variant}", 512, 384, 256, mode, "gemm256_kernel<false, false, ", **kw)


P8_VARIANTS = {                                                  # name -> (epilogue MASK of dispatch.h, arguments)
    "plain": (0, dict()),
    "bias+residual+dropout": (2 | 4, dict(bias=True, residual=True, dropout=0.1)),
    "bias+relu+dropout+bits": (1 | 2 | 32, dict(bias=True, act=RELU, dropout=0.1, actmask=True)),
    "drelu+bits+colsum": (8 | 16 | 32, dict(dact=RELU, actmask=True, colsum=F32)),
}


@pytest.mark.parametrize("variant", list(P8_VARIANTS))
@pytest.mark.parametrize("mode,M", [(8, 1000), (9, 1001), (10, 200)], ids=["256-rows-M1000", "224-rows-M1001", "192-rows-M200"])
def test_gemm_persistent_kernel_ragged_rows(L, mode, M, variant):
    """The tile height does not divide M: the last row tile overlaps its predecessor and ends exactly at row M - 1."""
    mask, kw = P8_VARIANTS[variant]
    _gemm_case(L, f"persistent mode {mode} M={M} {variant}", M, 512, 256, mode, f"gemm8p_kernel<{16 - mode}, {mask}, ", **kw)


@pytest.mark.parametrize("M,N,K,splitk", [(256, 256, 1024 + 72, 3), (256, 512, 640, 2)], ids=["tail-slab", "whole-k-tiles"])
@pytest.mark.parametrize("c_f32", [False, True], ids=["bf16-c", "fp32-c"])
def test_gemm_weight_gradient_kernel(L, M, N, K, splitk, c_f32):
    """K = 1024 + 72: the persistent kernel takes 1024 rows, the generic kernel writes the other 72 as one more slab."""
    _gemm_case(L, f"weight gradient {M}x{N}x{K}", M, N, K, 0, "gemm8p_km_kernel<", akm=True, bkm=True, splitk=splitk, c_f32=c_f32)


# ---- attention ---------------------------------------------------------------------------------------------------------------
# (id, head dim, N, H, environment, any_length, forward kernel, backward kernel)
SEQ2 = {"SFCVIT_ATTN_BWD_FUSED": "0"}
ATTN_CASES = (
    [(f"seq-fused-N{n}", 64, n, 2, {}, False, "attn_seq_fwd_kernel<%d, " % (13 if n == 200 else 0),
      "attn_seq_bwd_fused_kernel<%d, " % (13 if n == 200 else 0)) for n in (5, 70, 200, 224)]
    + [(f"seq-two-kernel-N{n}", 64, n, 2, SEQ2, False, "attn_seq_fwd_kernel<%d, " % (13 if n == 200 else 0),
        "attn_seq_bwd_kv_kernel<%d>" % (13 if n == 200 else 0)) for n in (5, 70, 200, 224)]
    + [(f"long-N{n}", 64, n, 2, {}, False, "attn_long_fwd_kernel<", "attn_long_bwd_kv_kernel") for n in (257, 300, 608)]
    + [("tiled-N609", 64, 609, 2, {}, False, "attn_fwd_kernel", "attn_bwd_kv_kernel"),
       ("tiled-N257", 64, 257, 2, {"SFCVIT_ATTN_LONG": "0"}, False, "attn_fwd_kernel", "attn_bwd_kv_kernel"),
       ("wide128-N5", 128, 5, 2, {}, False, "attn_wide_fwd_kernel<2>", "attn_wide_bwd_kv_kernel<2>"),
       ("wide128-N100", 128, 100, 2, {}, False, "attn_wide_fwd_kernel<2>", "attn_wide_bwd_kv_kernel<2>"),
       ("wide192-N180", 192, 180, 1, {}, False, "attn_wide_fwd_kernel<3>", "attn_wide_bwd_kv_kernel<3>"),
       ("wide256-N100", 256, 100, 1, {}, False, "attn_wide_fwd_kernel<4>", "attn_wide_bwd_kv_kernel<4>"),
       ("stream128-N257", 128, 257, 2, {}, True, "attn_wide_stream_fwd_kernel<2>", "attn_wide_stream_bwd_kv_kernel<2>"),
       ("stream256-N161", 256, 161, 2, {}, True, "attn_wide_stream_fwd_kernel<4>", "attn_wide_stream_bwd_kv_kernel<4>"),
       ("stream128-N1", 128, 1, 2, {"SFCVIT_ATTN_WIDE_STREAM": "1"}, True, "attn_wide_stream_fwd_kernel<2>", "attn_wide_stream_bwd_kv_kernel<2>"),
       ("stream128-N5", 128, 5, 2, {"SFCVIT_ATTN_WIDE_STREAM": "1"}, True, "attn_wide_stream_fwd_kernel<2>", "attn_wide_stream_bwd_kv_kernel<2>")])
ATTN_IDS = [c[0] for c in ATTN_CASES]
# one case per family also with dropout on the probabilities
ATTN_DROPOUT = {"seq-fused-N200", "seq-two-kernel-N70", "long-N300", "tiled-N609", "wide128-N100", "stream128-N257"}


def _set_env(monkeypatch, env):
    for k in ATTN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _attn_args(L, t, B, N, H, hd, p, masked=False):
    a = L.AttnMaskArgs() if masked else L.AttnArgs()
    for k in ("qkv", "out", "lse", "dout", "dqkv", "delta", "colsum_part", "colsum_out", "mask", "block_map"):
        if k in t:
            setattr(a, k, t[k].data_ptr())
    if "colsum_part" in t:
        a.colsum_part_bytes = t["colsum_part"].numel()
        a.colsum_bf16 = int(t["colsum_out"].dtype == BF16)
    a.B, a.N, a.H, a.hd, a.scale = B, N, H, hd, 1.0 / math.sqrt(hd)
    a.dropout_p, a.dropout_seed = p, SEED
    return a


def _attn_contained(L, what, B, N, H, hd, p, any_length, fwd_kernel, bwd_kernel, mask=None):
    """Forward, then backward without and with column sums (fp32 and bf16), every buffer guarded."""
    lib = L.lib
    D = H * hd
    g = torch.Generator().manual_seed(50 + N + hd)
    qkv, dout = _rand(g, B, N, 3 * D), _rand(g, B, N, D)
    masked = mask is not None
    extra = {"mask": mask.mask, "block_map": mask.block_map} if masked else {}
    last = lambda: _name(lib.sfcvit_last_attn_kernel)                                       # noqa: E731
    if masked:
        fwd, bwd = lib.sfcvit_attention_masked_fwd, lib.sfcvit_attention_masked_bwd
    elif any_length:
        fwd, bwd = lib.sfcvit_attention_fwd_any, lib.sfcvit_attention_bwd_any
    else:
        fwd, bwd = lib.sfcvit_attention_fwd, lib.sfcvit_attention_bwd

    def planned(t, is_bwd):
        if masked:
            return
        buf = ctypes.create_string_buffer(96)
        L.check(lib.sfcvit_attention_plan(ctypes.byref(_attn_args(L, t, B, N, H, hd, p)), int(is_bwd), int(any_length), buf, 96), what + " plan")
        want = bwd_kernel if is_bwd else fwd_kernel
        assert buf.value.decode().startswith(want), f"{what}: planned {buf.value.decode()}, the case is about {want}"
        return buf.value.decode()

    def run_fwd(t):
        name = planned(t, False)
        L.check(fwd(ctypes.byref(_attn_args(L, t, B, N, H, hd, p, masked)), _stream()), what + " forward")
        assert masked or last() == name

    f = contain(what + " forward", run_fwd, dict(qkv=qkv, **extra), {"out": ((B, N, D), BF16), "lse": ((B, H, N), F32)}, last_kernel=last,
                expect=fwd_kernel)

    def run_bwd(t):
        name = planned(t, True)
        L.check(bwd(ctypes.byref(_attn_args(L, t, B, N, H, hd, p, masked)), _stream()), what + " backward")
        assert masked or last() == name

    inputs = dict(qkv=qkv, dout=dout, out=f["out"], lse=f["lse"], **extra)
    delta = {"delta": B * H * N * 4}
    b0 = contain(what + " backward", run_bwd, inputs, {"dqkv": ((B, N, 3 * D), BF16)}, delta, last_kernel=last, expect=bwd_kernel)
    for cdt in (F32, BF16):
        ws = dict(delta, colsum_part=lib.sfcvit_attention_colsum_workspace(B, N, H, hd))
        b1 = contain(f"{what} backward + column sums {cdt}", run_bwd, inputs, {"dqkv": ((B, N, 3 * D), BF16), "colsum_out": ((3 * D,), cdt)}, ws,
                     last_kernel=last, expect=bwd_kernel)
        assert torch.equal(b1["dqkv"], b0["dqkv"]), what + ": dqkv changes with the column sums"


@pytest.mark.parametrize("case", ATTN_CASES, ids=ATTN_IDS)
def test_attention_forward_and_backward(L, case, monkeypatch):
    name, hd, N, H, env, any_length, fk, bk = case
    _set_env(monkeypatch, env)
    for p in (0.0, 0.1) if name in ATTN_DROPOUT else (0.0,):
        drop = "true" if p > 0 else "false"
        fk_p = fk + drop if fk.startswith("attn_seq_fwd_kernel<") else fk                 # the instances that carry the dropout flag
        bk_p = bk + drop if bk.startswith("attn_seq_bwd_fused_kernel<") else bk
        _attn_contained(L, f"{name} p={p}", 2, N, H, hd, p, any_length, fk_p, bk_p)


def _window(N):
    from sfcvit import masks, ops
    return ops.AttentionMask(masks.curve_window(N, 20))


@pytest.mark.parametrize("N", [70, 130])
def test_attention_masked_forward_and_backward(L, N, monkeypatch):
    """masks.curve_window(N, 20): at N = 130 the corner blocks of the 3 x 3 map are skipped, the others read the mask."""
    _set_env(monkeypatch, {})
    m = _window(N)
    assert N != 130 or (int(m.block_map[0, 2]) == 0 and int(m.block_map[1, 1]) == 1)
    for p in (0.0, 0.1):
        _attn_contained(L, f"masked N={N} p={p}", 2, N, 2, 64, p, False, "attn_masked_fwd_kernel", "attn_masked_bwd_kv_kernel", mask=m)


# ---- isolation: nothing crosses the batch or the head boundary ----------------------------------------------------------------
def _attn_run(ops, qkv, dout, H, any_length, mask, out=None, lse=None):
    """forward (unless out / lse are given) + backward through sfcvit.ops on dense tensors -> out, lse, dqkv"""
    if mask is None:
        if out is None:
            out, lse = ops.attention_fwd(qkv, H, any_length=any_length)
        dqkv = ops.attention_bwd(qkv, out, lse, dout, H, any_length=any_length)
    else:
        md, bm = mask.on("cuda")
        if out is None:
            out, lse = ops.attention_masked_fwd(qkv, H, md, bm)
        dqkv = ops.attention_masked_bwd(qkv, out, lse, dout, H, md, bm)
    return out, lse, dqkv


def _isolated(ops, what, B, N, H, hd, any_length, mask=None):
    D = H * hd
    g = torch.Generator().manual_seed(90 + N + hd)
    qkv, dout = _rand(g, B, N, 3 * D).cuda(), _rand(g, B, N, D).cuda()
    out, lse, dqkv = _attn_run(ops, qkv, dout, H, any_length, mask)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in (out, lse, dqkv)), what
    nan = float("nan")
    # every input of batch item 1 is NaN: item 0 comes out bit for bit as before
    q1, d1, o1, l1 = qkv.clone(), dout.clone(), out.clone(), lse.clone()
    for t in (q1, d1, o1, l1):
        t[1:] = nan
    out_b, lse_b, _ = _attn_run(ops, q1, d1, H, any_length, mask)
    _, _, dqkv_b = _attn_run(ops, q1, d1, H, any_length, mask, out=o1, lse=l1)
    assert torch.equal(out_b[0], out[0]) and torch.equal(lse_b[0], lse[0]), what + ": batch item 1 leaks into the forward of item 0"
    assert torch.equal(dqkv_b[0], dqkv[0]), what + ": batch item 1 leaks into the backward of item 0"
    assert bool(torch.isnan(out_b[1:].float()).any())                  # (and the poison did reach the kernel)
    # the q, k, v and dout columns of head 1 (and its out / lse) are NaN: head 0 comes out bit for bit as before
    q2, d2, o2, l2 = qkv.clone(), dout.clone(), out.clone(), lse.clone()
    for third in range(3):
        q2[:, :, third * D + hd:third * D + 2 * hd] = nan
    d2[:, :, hd:2 * hd] = nan
    o2[:, :, hd:2 * hd] = nan
    l2[:, 1] = nan
    out_h, lse_h, _ = _attn_run(ops, q2, d2, H, any_length, mask)
    _, _, dqkv_h = _attn_run(ops, q2, d2, H, any_length, mask, out=o2, lse=l2)
    assert torch.equal(out_h[:, :, :hd], out[:, :, :hd]) and torch.equal(lse_h[:, 0], lse[:, 0]), what + ": head 1 leaks into the forward of head 0"
    for third in range(3):
        cols = slice(third * D, third * D + hd)
        assert torch.equal(dqkv_h[:, :, cols], dqkv[:, :, cols]), what + ": head 1 leaks into the backward of head 0"


@pytest.mark.parametrize("case", ATTN_CASES, ids=ATTN_IDS)
def test_attention_batch_items_and_heads_are_isolated(case, monkeypatch):
    """Without column sums (those sum over the batch).  H = 2 everywhere here, also for head dims 192 and 256, so that there
    is a head to poison.  B = 2, H = 2: the fused backward's grid is capped at the item count, so each workgroup takes one
    item; the walk over several items per workgroup is test_attention_fused_backward_walks_several_items_per_workgroup."""
    from sfcvit import ops
    name, hd, N, _, env, any_length, _, bwd_kernel = case
    _set_env(monkeypatch, env)
    _isolated(ops, name, 2, N, 2, hd, any_length)
    assert ops.last_attn_kernel().startswith(bwd_kernel), name + ": ran " + ops.last_attn_kernel()


@pytest.mark.parametrize("N", [70, 200])
def test_attention_fused_backward_walks_several_items_per_workgroup(N, monkeypatch):
    """B H = 3 x 172 = 516 items on at most 256 workgroups: every workgroup stages the next (batch, head) item behind the
    current one.  Items of batch 1.. and of head 1 are poisoned in turn."""
    from sfcvit import ops
    _set_env(monkeypatch, {})
    _isolated(ops, f"fused backward, 516 items, N={N}", 3, N, 172, 64, False)
    assert ops.last_attn_kernel().startswith("attn_seq_bwd_fused_kernel<")


def test_attention_masked_batch_items_and_heads_are_isolated(monkeypatch):
    from sfcvit import ops
    _set_env(monkeypatch, {})
    _isolated(ops, "masked N=130", 2, 130, 2, 64, False, mask=_window(130))
    assert ops.last_attn_kernel() == "attn_masked_bwd_kv_kernel"


# ---- row-wise ----------------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("M,D", [(7, 192), (5, 4096), (4097, 768)], ids=["7x192", "5x4096", "4097x768-two-rows-odd-last-wave"])
def test_layernorm_forward(L, M, D):
    g = torch.Generator().manual_seed(M + D)
    inputs = {"x": _rand(g, M, D), "gamma": _rand(g, D), "beta": _rand(g, D)}
    outputs = {"y": ((M, D), BF16), "mean": ((M,), F32), "rstd": ((M,), F32)}

    def launch(t):
        L.check(L.lib.sfcvit_layernorm_fwd(_p(t["x"]), _p(t["gamma"]), _p(t["beta"]), _p(t["y"]), _p(t["mean"]), _p(t["rstd"]), M, D, 1e-5,
                                           _stream()), "layernorm_fwd")

    contain(f"layernorm_fwd {M}x{D}", launch, inputs, outputs)


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["fp32-grads", "bf16-grads"])
@pytest.mark.parametrize("M,D,kernel", [(7, 192, "ln_bwd_kernel<1, true>"), (513, 1024, "ln_bwd_cols_kernel<4, true>"),
                                        (300, 768, "ln_bwd_cols_kernel<3, true>"), (70, 1536, "ln_bwd_kernel<4, true>")],
                         ids=["7x192", "513x1024-cols", "300x768-cols", "70x1536"])
def test_layernorm_backward_with_residual_dropout_and_column_sums(L, M, D, kernel, gdt):
    from sfcvit import ops
    lib = L.lib
    g = torch.Generator().manual_seed(2 * M + D)
    x, gamma = _rand(g, M, D), _rand(g, D)
    _, mean, rstd = ops.layernorm_fwd(x.cuda(), gamma.cuda(), gamma.cuda())
    inputs = {"dy": _rand(g, M, D), "x": x, "mean": mean.cpu(), "rstd": rstd.cpu(), "gamma": gamma, "dx_add": _rand(g, M, D)}
    outputs = {"dx": ((M, D), BF16), "dx_drop": ((M, D), BF16), "dgamma": ((D,), gdt), "dbeta": ((D,), gdt), "dcol": ((D,), gdt)}

    def launch(t):
        L.check(lib.sfcvit_layernorm_bwd_drop(_p(t["dy"]), _p(t["x"]), _p(t["mean"]), _p(t["rstd"]), _p(t["gamma"]), _p(t["dx_add"]),
                                              _p(t["dx"]), _p(t["dx_drop"]), 0.1, SEED, None, _p(t["dgamma"]), _p(t["dbeta"]), _p(t["dcol"]),
                                              int(gdt == BF16), M, D, _p(t["ws"]), _stream()), "layernorm_bwd_drop")

    contain(f"layernorm_bwd_drop {M}x{D}", launch, inputs, outputs, {"ws": lib.sfcvit_layernorm_bwd_ws(M, D)},
            last_kernel=lambda: _name(lib.sfcvit_last_rowwise_kernel), expect=kernel)


@pytest.mark.parametrize("odt", [F32, BF16], ids=["fp32-out", "bf16-out"])
@pytest.mark.parametrize("c0,N", [(0, 328), (64, 128)], ids=["dense", "columns-64..191"])
def test_colsum(L, c0, N, odt):
    lib = L.lib
    M, ld = 5000, 328
    inputs = {"x": _rand(torch.Generator().manual_seed(4), M, ld)}
    nbytes = lib.sfcvit_colsum_workspace(M, N)

    def launch(t):
        x = t["x"][:, c0:c0 + N]                                   # a strided view: ld stays 328
        L.check(lib.sfcvit_colsum(_p(x), M, N, ld, _p(t["out"]), int(odt == BF16), _p(t["ws"]), nbytes, _stream()), "colsum")

    contain(f"colsum columns {c0}..{c0 + N - 1}", launch, inputs, {"out": ((N,), odt)}, {"ws": nbytes})


@pytest.mark.parametrize("n", [8, 4096 + 8])
def test_gelu(L, n):
    g = torch.Generator().manual_seed(n)
    inputs = {"x": _rand(g, n, scale=2.0), "dy": _rand(g, n)}

    def launch(t):
        L.check(L.lib.sfcvit_gelu_fwd(_p(t["x"]), _p(t["y"]), n, _stream()), "gelu_fwd")
        L.check(L.lib.sfcvit_gelu_bwd(_p(t["dy"]), _p(t["x"]), _p(t["dx"]), n, _stream()), "gelu_bwd")

    contain(f"gelu n={n}", launch, inputs, {"y": ((n,), BF16), "dx": ((n,), BF16)})


def test_gelu_with_dropout(L):
    rows, cols = 37, 264
    g = torch.Generator().manual_seed(37)
    inputs = {"x": _rand(g, rows, cols, scale=2.0), "dy": _rand(g, rows, cols)}

    def launch(t):
        L.check(L.lib.sfcvit_gelu_drop_fwd(_p(t["x"]), _p(t["y"]), rows, cols, 0.1, SEED, None, _stream()), "gelu_drop_fwd")
        L.check(L.lib.sfcvit_gelu_drop_bwd(_p(t["dy"]), _p(t["x"]), _p(t["dx"]), rows, cols, 0.1, SEED, None, _stream()), "gelu_drop_bwd")

    contain("gelu_drop 37x264", launch, inputs, {"y": ((rows, cols), BF16), "dx": ((rows, cols), BF16)})


def test_dropout_mask_with_odd_columns(L):
    def launch(t):
        L.check(L.lib.sfcvit_dropout_mask(_p(t["out"]), 5, 7, 0.1, SEED, _stream()), "dropout_mask")

    contain("dropout_mask 5x7", launch, {}, {"out": ((5, 7), BF16)})


CE_SHAPES = [(37, 10, 16), (3, 1000, 1000), (5, 77, 80)]


@pytest.mark.parametrize("B,C,ld", CE_SHAPES, ids=["37x10-ld16", "3x1000-ld1000", "5x77-ld80"])
def test_soft_ce(L, B, C, ld):
    g = torch.Generator().manual_seed(B + C)
    inputs = {"logits": _rand(g, B, ld, scale=3.0), "targets": torch.softmax(torch.randn(B, C, generator=g), -1)}

    def launch(t):
        L.check(L.lib.sfcvit_soft_ce(_p(t["logits"]), _p(t["targets"]), _p(t["loss_rows"]), _p(t["dlogits"]), B, C, ld, 1.0 / B, _stream()),
                "soft_ce")

    out = contain(f"soft_ce {B}x{C} ld {ld}", launch, inputs, {"loss_rows": ((B,), F32), "dlogits": ((B, ld), BF16)})
    assert not bool(out["dlogits"][:, C:].any())                    # the padding columns are written as zeros


@pytest.mark.parametrize("B,C,ld", CE_SHAPES, ids=["37x10-ld16", "3x1000-ld1000", "5x77-ld80"])
def test_soft_ce_pair(L, B, C, ld):
    g = torch.Generator().manual_seed(B + C + 1)
    rec = np.zeros(8, dtype=np.uint32)
    rec[0] = 1                                                      # MixUp
    rec[5:7] = np.array([0.3, 0.7], dtype=np.float32).view(np.uint32)
    inputs = {"logits": _rand(g, B, ld, scale=3.0), "y_a": torch.randint(0, C, (B,), generator=g), "y_b": torch.randint(0, C, (B,), generator=g),
              "rec": torch.from_numpy(rec.view(np.int32).copy())}
    inputs["y_b"][0] = inputs["y_a"][0]                             # one row with a single target

    def launch(t):
        L.check(L.lib.sfcvit_soft_ce_pair(_p(t["logits"]), _p(t["y_a"]), _p(t["y_b"]), _p(t["rec"]), _p(t["loss_rows"]), _p(t["dlogits"]),
                                          _p(t["hit_rows"]), B, C, ld, 1.0 / B, _stream()), "soft_ce_pair")

    out = contain(f"soft_ce_pair {B}x{C} ld {ld}", launch, inputs,
                  {"loss_rows": ((B,), F32), "dlogits": ((B, ld), BF16), "hit_rows": ((B,), F32)})
    assert not bool(out["dlogits"][:, C:].any())


SUMSQ_WORKSPACE_BYTES = 4096                                        # SFCVIT_SUMSQ_WORKSPACE_BYTES (include/sfcvit.h)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [3, 10007, 1024 * 256 * 8 + 2048 + 5], ids=["tail-only", "n10007", "partial-cap"])
def test_sumsq_accum(L, n, dt):
    """out is pre-set: the kernel accumulates.  The largest n needs more than 1024 workgroups of 256 x 8 elements, so the grid
    sits at the cap of 1024 partials."""
    src = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000)).to(dt)

    def launch(t):
        L.check(L.lib.sfcvit_sumsq_accum(_p(t["g"]), n, int(dt == F32), _p(t["out"]), _p(t["ws"]), _stream()), "sumsq_accum")

    out = contain(f"sumsq n={n}", launch, {"g": src}, {}, {"ws": SUMSQ_WORKSPACE_BYTES}, inouts={"out": torch.tensor([2.5])})
    assert bool(torch.isfinite(out["out"]).all()) and float(out["out"]) > 2.5


def _adamw(L, t, lo, hi):
    a = L.AdamWArgs()
    a.param, a.grad = t["param"].data_ptr() + 2 * lo, t["grad"].data_ptr() + 2 * lo
    a.master, a.m, a.v = t["master"].data_ptr() + 4 * lo, t["m"].data_ptr() + 4 * lo, t["v"].data_ptr() + 4 * lo
    a.sumsq, a.n = t["sumsq"].data_ptr(), hi - lo
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.max_norm, a.grad_scale, a.step = 3e-4, 0.9, 0.999, 1e-8, 5e-2, 1.0, 1.0, 3
    L.check(L.lib.sfcvit_adamw_step(ctypes.byref(a), _stream()), "adamw_step")


ADAMW_LARGE = 2 * 2048 * 256 * 4 + 4 * 300 + 3                       # past the two-group loop: 300 single groups and 3 tail elements


@pytest.mark.parametrize("n", [3, 10007, ADAMW_LARGE], ids=["tail-only", "n10007", "two-group-loop"])
def test_adamw_step(L, n):
    """The update is elementwise: the run over all n elements must equal, bit for bit, the same buffers updated as two calls
    split at a multiple of 8 (each of those is a different grid and a different walk through the main loop)."""
    g = torch.Generator().manual_seed(n % 1000)
    w = torch.randn(n, generator=g)
    grad = _rand(g, n, scale=0.1)
    inputs = {"grad": grad, "sumsq": grad.float().pow(2).sum().reshape(1) * 4.0}          # (norm > max_norm: the clip is active)
    state = {"param": w.to(BF16), "master": w, "m": torch.randn(n, generator=g) * 0.01, "v": torch.rand(n, generator=g) * 1e-3}
    whole = contain(f"adamw n={n}", lambda t: _adamw(L, t, 0, n), inputs, {}, inouts=state)
    assert all(bool(torch.isfinite(whole[k].float()).all()) for k in state)
    assert not torch.equal(whole["master"], w.cuda())
    if n >= 16:
        cut = (n // 3) // 8 * 8

        def halves(t):
            _adamw(L, t, 0, cut)
            _adamw(L, t, cut, n)

        split = contain(f"adamw n={n} as two calls", halves, inputs, {}, inouts=state)
        for k in state:
            assert torch.equal(split[k], whole[k]), f"adamw n={n}: '{k}' of one call differs from two calls split at {cut}"


TRANSPOSE_SHAPES = [(136, 72), (8, 200)]


@pytest.mark.parametrize("R,C", TRANSPOSE_SHAPES, ids=["136x72", "8x200"])
def test_transpose(L, R, C):
    src = _rand(torch.Generator().manual_seed(R), R, C)

    def launch(t):
        L.check(L.lib.sfcvit_transpose(_p(t["src"]), R, C, C, _p(t["dst"]), R, _stream()), "transpose")

    out = contain(f"transpose {R}x{C}", launch, {"src": src}, {"dst": ((C, R), BF16)})
    assert torch.equal(out["dst"].cpu(), src.t().contiguous())


def test_transpose_batched(L):
    g = torch.Generator().manual_seed(5)
    mats = [_rand(g, r, c) for r, c in TRANSPOSE_SHAPES]
    offs = [0, mats[0].numel()]
    total = sum(m.numel() for m in mats)
    rows = [(o, o, r, c, r0, c0) for (r, c), o in zip(TRANSPOSE_SHAPES, offs) for r0 in range(0, r, 64) for c0 in range(0, c, 64)]
    table = np.array(rows, dtype=np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("R", "<i4"), ("C", "<i4"), ("r0", "<i4"), ("c0", "<i4")]))
    inputs = {"src": torch.cat([m.flatten() for m in mats]), "tiles": torch.from_numpy(table.view(np.uint8).copy())}

    def launch(t):
        L.check(L.lib.sfcvit_transpose_batched(_p(t["src"]), _p(t["dst"]), _p(t["tiles"]), len(rows), _stream()), "transpose_batched")

    out = contain("transpose_batched", launch, inputs, {"dst": ((total,), BF16)})
    for m, o in zip(mats, offs):
        assert torch.equal(out["dst"][o:o + m.numel()].cpu().view(m.shape[1], m.shape[0]), m.t().contiguous())


# ---- tokenizers ------------------------------------------------------------------------------------------------------------------
def _last_tok(L):
    return lambda: _name(L.lib.sfcvit_last_tokenizer_kernel)


def _desc_host(L, pix_h, img):
    N = pix_h.shape[0]
    desc = np.zeros(16 + 2 * N + 2 * 8 * 256, dtype=np.int32)
    n = L.lib.sfcvit_tile_descriptors(ctypes.c_void_p(pix_h.ctypes.data), N, 256, img, ctypes.c_void_p(desc.ctypes.data), desc.size)
    assert n > 0
    return desc[:n].copy()


def _pe_contain(L, what, dims, pix_h, desc_h, xdt, want_dbias, fwd_expect, bwd_expect):
    (HW, N, P, C), D, B = dims
    lib = L.lib
    g = torch.Generator().manual_seed(2000 + HW + D + B)
    H, W = TR.image_hw(HW)
    inputs = {"x": torch.randn(B, C, H, W, generator=g).to(xdt), "pix": torch.from_numpy(pix_h), "w": _rand(g, D, P * C, scale=(P * C) ** -0.5),
              "bias": _rand(g, D)}
    if desc_h is not None:
        inputs["desc"] = torch.from_numpy(desc_h)

    def args(t, bwd):
        a = L.PatchEmbedArgs()
        a.x, a.pix, a.y = t["x"].data_ptr(), t["pix"].data_ptr(), t["y"].data_ptr()
        a.B, a.C, a.HW, a.N, a.P, a.D, a.x_is_bf16 = B, C, HW, N, P, D, int(xdt == BF16)
        a.workspace, a.workspace_bytes = t["ws"].data_ptr(), t["ws"].numel()
        if desc_h is not None:
            a.desc, a.desc_ncls = t["desc"].data_ptr(), int(desc_h[1])
            for c in range(int(desc_h[1])):
                a.desc_cnt[c] = int(desc_h[7 + c] - desc_h[6 + c])
        if bwd:
            a.dw, a.dbias = t["dw"].data_ptr(), (t["dbias"].data_ptr() if want_dbias else None)
        else:
            a.w, a.bias = t["w"].data_ptr(), t["bias"].data_ptr()
        return a

    contain(what + " fwd", lambda t: L.check(lib.sfcvit_patch_embed_fwd(ctypes.byref(args(t, False)), _stream()), what), inputs,
            {"y": ((B * N, D), BF16)}, {"ws": lib.sfcvit_patch_embed_workspace(B, C, N, P, D, 0)}, last_kernel=_last_tok(L), expect=fwd_expect)
    binputs = {k: v for k, v in inputs.items() if k in ("x", "pix", "desc")}
    binputs["y"] = _rand(g, B * N, D)
    outputs = {"dw": ((D, P * C), F32)}
    if want_dbias:
        outputs["dbias"] = ((D,), F32)
    contain(what + " bwd", lambda t: L.check(lib.sfcvit_patch_embed_bwd(ctypes.byref(args(t, True)), _stream()), what), binputs,
            outputs, {"ws": lib.sfcvit_patch_embed_workspace(B, C, N, P, D, 1)}, last_kernel=_last_tok(L), expect=bwd_expect)


@pytest.mark.parametrize("want_dbias", [True, False], ids=["dbias", "no-dbias"])
@pytest.mark.parametrize("dims", TR.CONTAIN_PE, ids=lambda d: "HW%d-N%d-P%d-C%d-D%d-B%d" % (*d[0], d[1], d[2]))
def test_patch_embed_generic(L, dims, want_dbias):
    """Scalar gather with K padded to 32; M and D past a 128 tile; 66 split slabs in a workspace of exactly the queried size."""
    (HW, N, P, C), D, B = dims
    xdt = F32 if want_dbias else BF16
    _pe_contain(L, f"patch_embed generic {dims}", dims, TR.hostile_table(HW, N, P, seed=HW + B), None, xdt, want_dbias,
                f"pe_fwd_kernel<{'fp32' if xdt == F32 else 'bf16'}>", f"pe_bwd_kernel<{'fp32' if xdt == F32 else 'bf16'}>")


@pytest.mark.parametrize("case", TR.CONTAIN_PE2, ids=lambda c: "%s%d-C%d-B%d" % c)
def test_patch_embed_tiled(L, case):
    """Hilbert at B = 33 (ragged classes, padded row tiles) and the 8-class table (classes of 3-6 rows inside 128-row tiles)."""
    name, img, C, B = case
    pix_h = TR.pe2_table(name, img)
    _pe_contain(L, f"patch_embed tiled {case}", ((img * img, pix_h.shape[0], 256, C), TR.PE2_D, B), pix_h, _desc_host(L, pix_h, img), F32, True,
                "pe2_fwd_kernel<fp32>", "pe2_bwd_kernel<fp32>")


@pytest.mark.parametrize("table,B,extra", TR.CONTAIN_GATHER, ids=["p256-P16", "general-P512", "general-P512-ld+24"])
def test_tokens_gather(L, table, B, extra):
    HW, N, P, C = table
    g = torch.Generator().manual_seed(2100 + P + extra)
    ld = (P * C + 7) // 8 * 8 + extra
    inputs = {"x": torch.randn(B, C, *TR.image_hw(HW), generator=g), "pix": torch.from_numpy(TR.hostile_table(HW, N, P, seed=P))}

    def launch(t):
        L.check(L.lib.sfcvit_tokens_gather(_p(t["x"]), 0, _p(t["pix"]), None, B, C, HW, N, P, _p(t["tokens"]), ld, _stream()), "tokens_gather")

    out = contain(f"tokens_gather {table} ld {ld}", launch, inputs, {"tokens": ((B * N, ld), BF16)}, last_kernel=_last_tok(L),
                  expect="tokens_gather_p256_kernel<fp32>" if P <= 256 else "tokens_gather_kernel<fp32>")
    assert not bool(out["tokens"][:, P * C:].any())


def _tile_tables(L, img):
    from sfcvit import ops
    pix_h = TR.curve_pixel_table("hilbert", img, 256)
    desc = _desc_host(L, pix_h, img)
    N = pix_h.shape[0]
    return pix_h, torch.from_numpy(desc[16 + N:16 + 2 * N].copy()), torch.from_numpy(ops.gather_order(pix_h))


@pytest.mark.parametrize("ordered", [True, False], ids=["order", "no-order"])
def test_tokens_gather_tiles(L, ordered):
    """48 px: nine tiles, so the last workgroup holds one token; B = 5: a second group of four images holding one."""
    img, C, B = 48, 3, 5
    pix_h, origin, order = _tile_tables(L, img)
    N = pix_h.shape[0]
    inputs = {"x": torch.randn(B, C, img, img, generator=torch.Generator().manual_seed(2200)), "pix": torch.from_numpy(pix_h), "origin": origin}
    if ordered:
        inputs["order"] = order

    def launch(t):
        L.check(L.lib.sfcvit_tokens_gather_tiles(_p(t["x"]), _p(t["pix"]), _p(t["order"]) if ordered else None, _p(t["origin"]), B, C, img, img, N,
                                                 _p(t["tokens"]), 256 * C, _stream()), "tokens_gather_tiles")

    contain(f"tokens_gather_tiles 48 px ordered={ordered}", launch, inputs, {"tokens": ((B * N, 256 * C), BF16)}, last_kernel=_last_tok(L),
            expect="tokens_gather_tiles_kernel<3, fp32>")


def _cutmix_rec(r0, r1, c0, c1, lam):
    bits = lambda v: struct.unpack("<i", struct.pack("<f", v))[0]              # noqa: E731
    return torch.tensor([2, r0, r1, c0, c1, bits(lam), bits(float(np.float32(1.0 - lam))), 0], dtype=torch.int32)


@pytest.mark.parametrize("path", ["tiles", "pixel"])
def test_tokens_gather_mix(L, path):
    """One CutMix box that cuts through tokens; perm and the record are guarded inputs like the tables."""
    C = 3
    img, P, B = (48, 256, 5) if path == "tiles" else (32, 16, 9)
    g = torch.Generator().manual_seed(2300 + P)
    if path == "tiles":
        pix_h, origin, order = _tile_tables(L, img)
    else:
        pix_h, origin, order = TR.curve_pixel_table("hilbert", img, P), None, None
    N = pix_h.shape[0]
    inputs = {"x": torch.randn(B, C, img, img, generator=g), "pix": torch.from_numpy(pix_h),
              "perm": torch.randperm(B, generator=g).to(torch.int32), "rec": _cutmix_rec(5, 30, 10, 27, 0.7)}
    if origin is not None:
        inputs.update(origin=origin, order=order)

    def launch(t):
        L.check(L.lib.sfcvit_tokens_gather_mix(_p(t["x"]), _p(t["pix"]), _p(t["order"]) if "order" in t else None,
                                               _p(t["origin"]) if "origin" in t else None, _p(t["perm"]), _p(t["rec"]), B, C, img, img, N, P,
                                               _p(t["tokens"]), P * C, _stream()), "tokens_gather_mix")

    out = contain(f"tokens_gather_mix {path}", launch, inputs, {"tokens": ((B * N, P * C), BF16)}, last_kernel=_last_tok(L),
                  expect="tokens_gather_tiles_kernel<3, mix>" if path == "tiles" else "tokens_gather_p256_kernel<mix>")
    plain = torch.zeros_like(out["tokens"])
    L.check(L.lib.sfcvit_tokens_gather(_p(inputs["x"].cuda()), 0, _p(inputs["pix"].cuda()), None, B, C, img * img, N, P, _p(plain), P * C, _stream()),
            "tokens_gather")
    assert not torch.equal(out["tokens"], plain)                                  # the box did mix something


@pytest.mark.parametrize("biased", [True, False], ids=["biases", "all-biases-null"])
@pytest.mark.parametrize("fuse", [True, False], ids=["fuse", "levels"])
@pytest.mark.parametrize("case", TR.CONTAIN_HIER, ids=["M65", "M20"])
def test_hier_tokenizer(L, case, fuse, biased):
    """M = 65: one row in the second workgroup; M = 20: wave 3 idle in the level phase (D = 192), four levels of K = 96.  In the wf = NULL form y is not
    passed; every bias null once per case and form."""
    Lv, D, C, P, N, B = case
    E = Lv * D
    g = torch.Generator().manual_seed(2400 + D)
    tabs = TR.hier_tables(case, True)
    inputs = {"x": torch.randn(B, C, *TR.image_hw(N * P), generator=g)}
    for l in range(Lv):
        inputs[f"pix{l}"], inputs[f"w{l}"] = torch.from_numpy(tabs[l]), _rand(g, D, P * C, scale=(P * C) ** -0.5)
        if biased:
            inputs[f"b{l}"] = _rand(g, D)
    outputs = {"h": ((B * N, E), BF16)}
    if fuse:
        inputs["wf"] = _rand(g, E, E, scale=E ** -0.5)
        outputs["y"] = ((B * N, E), BF16)
        if biased:
            inputs["bf"] = _rand(g, E)

    def launch(t):
        a = L.HierArgs()
        a.x, a.h = t["x"].data_ptr(), t["h"].data_ptr()
        for l in range(Lv):
            a.pix[l], a.w[l], a.P[l] = t[f"pix{l}"].data_ptr(), t[f"w{l}"].data_ptr(), P
            a.b[l] = t[f"b{l}"].data_ptr() if biased else None
        if fuse:
            a.wf, a.y = t["wf"].data_ptr(), t["y"].data_ptr()
            a.bf = t["bf"].data_ptr() if biased else None
        a.B, a.C, a.HW, a.N, a.L, a.D = B, C, N * P, N, Lv, D
        L.check(L.lib.sfcvit_hier_tokenizer_fwd(ctypes.byref(a), _stream()), "hier_tokenizer_fwd")

    contain(f"hier_tokenizer {case} fuse={fuse} biased={biased}", launch, inputs, outputs, last_kernel=_last_tok(L),
            expect=f"hier_fwd_kernel<fp32, {'fuse' if fuse else 'levels'}>")


@pytest.mark.parametrize("counts", TR.CONTAIN_RESAMPLE, ids=str)
def test_hier_resample_concat_pair(L, counts):
    D, B, n0, nl = TR.RESAMPLE_D[0], TR.RESAMPLE_B, counts[0], len(counts)
    g = torch.Generator().manual_seed(2500 + n0)
    levels = {f"lev{l}": _rand(g, B, n, D) for l, n in enumerate(counts)}
    n_tok = (ctypes.c_int32 * nl)(*counts)

    def fwd(t):
        ptrs = (ctypes.c_void_p * nl)(*[t[f"lev{l}"].data_ptr() for l in range(nl)])
        L.check(L.lib.sfcvit_hier_resample_concat(ptrs, n_tok, nl, B, n0, D, _p(t["out"]), _stream()), "hier_resample_concat")

    def bwd(t):
        ptrs = (ctypes.c_void_p * nl)(*[t[f"dlev{l}"].data_ptr() for l in range(nl)])
        L.check(L.lib.sfcvit_hier_resample_concat_bwd(_p(t["dout"]), n_tok, nl, B, n0, D, ptrs, _stream()), "hier_resample_concat_bwd")

    contain(f"hier_resample_concat {counts}", fwd, levels, {"out": ((B, n0, nl * D), BF16)}, last_kernel=_last_tok(L),
            expect="hier_resample_concat_kernel")
    contain(f"hier_resample_concat_bwd {counts}", bwd, {"dout": _rand(g, B, n0, nl * D)}, {f"dlev{l}": ((B, n, D), BF16) for l, n in enumerate(counts)},
            last_kernel=_last_tok(L), expect="hier_resample_concat_bwd_kernel")
