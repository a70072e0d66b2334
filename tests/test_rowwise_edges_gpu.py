"""The row-wise kernels (csrc/layernorm.hip, rowwise.hip, optim.hip) at every form their plans select, against
tests/rowwise_ref.py, whose docstring derives the bars and which tests/test_rowwise_ref_cpu.py qualifies without a GPU.

(a) Exact-sum inputs, the structural check: small integers and dyadic fractions, every partial sum an fp32 value in any order,
    so the answer is bit-exact and a dropped or doubled row, column, vector or partial changes it.
(b) fp64-referenced random and edge rows, the formula check: every output at most its derived bar off.

The shapes come from csrc/rowwise.cpp at today's constants (test_shapes_meet_the_library_geometry re-derives them on the CPU):
LayerNorm forward runs VPL = 1 / 2 / 4 / 8 vectors per lane up to D = 512 / 1024 / 2048 / 4096 and the two-row form at
D = 768 / 1024 from 4096 rows; backward runs <1> / <2> / <4> likewise, the column form at D = 768 / 1024, on at most 512 (768 at
D = 768) workgroups of 4 waves, so past 2048 (3072) rows a wave walks a second row and the prefetch path runs.
Every test prints its worst |err| / bar (FIGURE lines) before asserting <= 1."""
import ctypes

import numpy as np
import pytest
import torch

import rowwise_ref as R
from rowwise_ref import f64

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def fig(what, figures):
    print(f"FIGURE {what}: " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


def same(got, want64):
    """Equal as values (-0 = +0), element for element."""
    return np.array_equal(f64(got), np.asarray(want64, dtype=np.float64))


# ---- (a) exact sums -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", R.LN_FWD_EXACT)
def test_layernorm_fwd_exact_sums(ops, M, D):
    x, gamma, beta, mean, q = R.ln_exact_fwd_inputs(M, D)
    _, mu, rs = ops.layernorm_fwd(x.cuda(), gamma.cuda(), beta.cuda(), R.EPS)
    torch.cuda.synchronize()
    rstd_ref = 1.0 / np.sqrt(q / D + R.EPS)
    worst = R.ratio(f64(rs) / rstd_ref - 1, R.rstd_bar(x, q / D, exact=True))
    wrong = int((f64(mu) != mean).sum())
    fig(f"ln_fwd exact ({M}, {D}) {R.ln_fwd_form(M, D)}", dict(mean_rows_wrong=wrong, rstd=worst))
    assert wrong == 0 and worst <= 1


def _bwd_exact_check(ops, inp, M, D, with_add, as_bf16):
    w = inp["want"]
    dev = {k: inp[k].cuda() for k in ("x", "dy", "gamma", "mean", "rstd", "add")}
    go = tuple(torch.full((D,), float("nan"), device="cuda", dtype=BF16) for _ in range(3)) if as_bf16 else None
    dx, dg, db, dc = ops.layernorm_bwd(dev["dy"], dev["x"], dev["mean"], dev["rstd"], dev["gamma"], dx_add=dev["add"] if with_add else None,
                                       want_colsum=True, grad_out=go)
    torch.cuda.synchronize()
    assert ops.last_rowwise_kernel() == R.ln_bwd_form(M, D, with_add), ops.last_rowwise_kernel()
    want = dict(dx=w["dxa"] if with_add else w["dx"], dgamma=w["dgamma"], dbeta=w["dbeta"], dcol=w["dcol_add"] if with_add else w["dcol"])
    got = dict(dx=dx, dgamma=dg, dbeta=db, dcol=dc)
    wrong = {}
    for k in want:
        want_k = want[k].to(BF16).double() if as_bf16 and k != "dx" else want[k]          # round to nearest even of the exact sum
        wrong[k] = int((f64(got[k]) != want_k.numpy()).sum())
    return wrong


@pytest.mark.parametrize("M,D", R.LN_BWD_EXACT)
def test_layernorm_bwd_exact_sums(ops, M, D):
    inp = R.ln_exact_bwd_inputs(M, D)
    if M >= 259:                                  # dbeta's columns 0 and 1 are 257 and 259: bf16 ties, to 256 and 260
        assert inp["want"]["dbeta"][:2].to(BF16).tolist() == [256.0, 260.0]
    for with_add in (False, True):
        for as_bf16 in (False, True):
            wrong = _bwd_exact_check(ops, inp, M, D, with_add, as_bf16)
            fig(f"ln_bwd exact ({M}, {D}) {R.ln_bwd_form(M, D, with_add)} {'bf16' if as_bf16 else 'fp32'} grads, elements wrong", wrong)
            assert not any(wrong.values()), wrong


def test_layernorm_bwd_exact_sums_deferred(ops):
    """Through sfcvit_reduce_defer / sfcvit_reduce_flush: the three reductions are queued, and after the flush they hold the
    exact sums (257 partial rows: the reducer's remainder loop)."""
    from sfcvit._lib import lib
    M, D = 1025, 520
    inp = R.ln_exact_bwd_inputs(M, D)
    w = inp["want"]
    dev = {k: inp[k].cuda() for k in ("x", "dy", "gamma", "mean", "rstd")}
    dx = torch.empty_like(dev["x"])
    dg, db, dc = (torch.full((D,), float("nan"), device="cuda") for _ in range(3))
    ws = torch.empty(lib.sfcvit_layernorm_bwd_ws(M, D), device="cuda", dtype=torch.uint8)          # alive until the flush
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())                                                  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sfcvit_reduce_pending() == 0
    lib.sfcvit_reduce_defer(1)
    try:
        rc = lib.sfcvit_layernorm_bwd_drop(p_(dev["dy"]), p_(dev["x"]), p_(dev["mean"]), p_(dev["rstd"]), p_(dev["gamma"]), None, p_(dx), None,
                                           0.0, 0, None, p_(dg), p_(db), p_(dc), 0, M, D, p_(ws), stream)
    finally:
        lib.sfcvit_reduce_defer(0)
    pending = lib.sfcvit_reduce_pending()
    torch.cuda.synchronize()
    untouched = bool(torch.isnan(dg).all() and torch.isnan(db).all() and torch.isnan(dc).all())
    ops.flush_deferred()
    torch.cuda.synchronize()
    assert rc == 0 and pending == 3 and untouched and lib.sfcvit_reduce_pending() == 0
    assert same(dx, w["dx"]) and same(dg, w["dgamma"]) and same(db, w["dbeta"]) and same(dc, w["dcol"])


@pytest.mark.parametrize("M,N", R.COLSUM_EXACT)
def test_colsum_exact_sums(ops, M, N):
    x, want = R.colsum_exact_inputs(M, N)
    xd = x.cuda()
    out = ops.colsum(xd)
    out16 = ops.colsum(xd, out=torch.full((N,), float("nan"), device="cuda", dtype=BF16))
    torch.cuda.synchronize()
    wrong = dict(fp32=int((f64(out) != want.double().numpy()).sum()), bf16=int((f64(out16) != want.double().to(BF16).double().numpy()).sum()))
    fig(f"colsum exact ({M}, {N}), {R.colsum_parts(M, N)[1]} partial rows, columns wrong", wrong)
    assert not any(wrong.values())
    if M >= 259:
        assert out16[:2].tolist() == [256.0, 260.0]                                  # 257 and 259 round to even


def test_colsum_exact_sums_of_a_column_slice(ops):
    M, N = 5000, 328
    x, want = R.colsum_exact_inputs(M, N)
    big = torch.full((M, N + 16), 9.0, dtype=BF16)
    big[:, 8:8 + N] = x
    out = ops.colsum(big.cuda()[:, 8:8 + N])
    torch.cuda.synchronize()
    assert same(out, want.double().numpy())


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_sumsq_exact_sums(ops, n, dtype):
    v, s = R.sumsq_exact_inputs(n)
    out = torch.full((1,), 1000.0, device="cuda")
    ops.sumsq_accum(v.to(dtype).cuda(), out)
    torch.cuda.synchronize()
    fig(f"sumsq exact n={n} {dtype}, {R.sumsq_parts(n)} partials", dict(got=float(out), want=float(1000 + s)))
    assert float(out) == 1000.0 + s


# ---- (b) fp64-referenced random and edge rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", R.LN_RANDOM)
def test_layernorm_random_and_edge_rows(ops, M, D):
    x, gamma, beta, dy, add = R.ln_random_inputs(M, D)
    xd, gd = x.cuda(), gamma.cuda()
    y, mean, rstd = ops.layernorm_fwd(xd, gd, beta.cuda(), R.EPS)
    torch.cuda.synchronize()
    rat = R.ln_fwd_ratios(x, gamma, beta, (y, f64(mean), f64(rstd)))
    fig(f"ln_fwd random ({M}, {D}) {R.ln_fwd_form(M, D)}", rat)
    assert R.passes(rat), rat
    if D > R.LN_BWD_MAX_D:
        return
    for with_add in (False, True):                # backward takes the kernel's own mean / rstd, and so does the reference
        dx, dg, db, dc = ops.layernorm_bwd(dy.cuda(), xd, mean, rstd, gd, dx_add=add.cuda() if with_add else None, want_colsum=True)
        torch.cuda.synchronize()
        assert ops.last_rowwise_kernel() == R.ln_bwd_form(M, D, with_add), ops.last_rowwise_kernel()
        ref = R.ln_bwd_ref(dy, x, mean, rstd, gamma, add if with_add else None)
        rat = R.ln_bwd_ratios(ref, (dx, f64(dg), f64(db), f64(dc)), M, D, with_add)
        fig(f"ln_bwd random ({M}, {D}) {R.ln_bwd_form(M, D, with_add)}", rat)
        assert R.passes(rat), rat


GELU_TILES = 65                                   # 65 x 65 280 = 4 243 200 > 2048 x 256 x 8: the grid-stride loop's second sweep


@pytest.mark.parametrize("bwd,random_dy", [(False, False), (True, False), (True, True)], ids=["fwd", "bwd-dy1", "bwd-random-dy"])
def test_gelu_every_finite_bf16(ops, bwd, random_dy):
    one = R.gelu_all_finite()
    x = one.repeat(GELU_TILES)
    assert x.numel() > 2048 * 256 * 8 and x.numel() % 8 == 0
    if bwd:
        dy = R.bf(torch.randn(x.numel(), generator=torch.Generator().manual_seed(7))) if random_dy else torch.ones_like(x)
        got = ops.gelu_bwd(dy.cuda(), x.cuda()).cpu()
        ref = R.gelu_grad_ref(x if random_dy else one)
    else:
        dy = None
        got = ops.gelu_fwd(x.cuda()).cpu()
        ref = R.gelu_ref(one)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got.float()).all())
    if random_dy:
        ref = ref * f64(dy)
        ok, on_floor, worst = R.elementwise_verdict(got, ref, R.gelu_floor(x, dy))
    else:                                         # every tile holds the same bits; the first is held to the reference
        tiles = got.view(GELU_TILES, -1).view(torch.int16)
        assert torch.equal(tiles, tiles[:1].expand_as(tiles))
        ok, on_floor, worst = R.elementwise_verdict(got[:one.numel()], ref, R.gelu_floor(one))
    fig(f"gelu {'bwd' if bwd else 'fwd'}{' random dy' if random_dy else ''}",
        dict(outside=int((~ok).sum()), floor_share=float(on_floor.mean()), worst_of_floor=worst))
    assert ok.all() and on_floor.mean() <= 0.01


@pytest.mark.parametrize("B,C,ld", list(R.CE_CASES))
def test_soft_ce_dense(ops, B, C, ld):
    from sfcvit._lib import lib
    logits, targets, kinds = R.ce_inputs(B, C, ld)
    gscale = 1.0 / B
    ld_, td = logits.cuda(), targets.cuda()
    loss, dl = ops.soft_ce(ld_, td, C, gscale)
    loss_only = torch.full((B,), float("nan"), device="cuda")
    rc = lib.sfcvit_soft_ce(ctypes.c_void_p(ld_.data_ptr()), ctypes.c_void_p(td.data_ptr()), ctypes.c_void_p(loss_only.data_ptr()), None,
                            B, C, ld, gscale, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    v = R.ce_verdict(logits, targets, C, gscale, (f64(loss), dl[:, :C].cpu()))
    worst_rows = {k: int(max(v["steps"][i].max() for i in range(B) if kinds[i] == k)) for k in dict.fromkeys(kinds)}
    fig(f"soft_ce ({B}, {C}, {ld})", dict(loss=v["loss"], floor_share=v["floor_share"], worst_of_floor=v["floor_worst"]))
    fig(f"soft_ce ({B}, {C}, {ld}) dlogits bf16 steps by row kind", worst_rows)
    assert v["loss"] <= 1 and v["grad_ok"], v
    assert not dl[:, C:].any()                                                        # padding columns are written 0
    assert rc == 0 and torch.equal(loss_only.view(torch.int32), loss.view(torch.int32))
