"""Pre-norm encoder layers with GELU and LayerScale on the HIP path: the two LayerScale residual-site kernels bit for bit where the
arithmetic is exact (lam = 1 against the DropPath kernels, power-of-two lam, dropped images) and at the store-point bar elsewhere,
the layer against an fp32 reference with the same masks and flags in every combination of activation, LayerScale and DropPath,
and the models: eval against torch's own module tree, the post-norm path unchanged, training, the captured step, main.py,
torch.compile and the attention report."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prenorm_ref
from oracle import formula
from oracle.cases import MODEL_CASES
from prenorm_ref import keep_flags, layernorm_of
from test_drop_path_gpu import SHAPES, bits, inputs, rows_of, seeds_for
from token_pool_ref import build_with

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def vpl(D):
    return 1 if D <= 512 else 2 if D <= 1024 else 4 if D <= 2048 else 8


def bwd_kernel(D, add):
    tf = "true" if add else "false"
    if D in (768, 1024):
        return f"ln_bwd_cols_scale_kernel<{D // 256}, {tf}>"
    return f"ln_bwd_scale_kernel<{min(vpl(D), 4)}, {tf}>"


def lam_ones(D):
    return torch.ones(D, device="cuda", dtype=BF16)


def lam_pow2(D):
    """lam[d] = +-2^-(d mod 14), the sign changing every 14 channels: every product with it is exact."""
    d = torch.arange(D, device="cuda")
    return (torch.pow(2.0, -(d % 14).float()) * (1 - 2 * ((d // 14) % 2)).float()).to(BF16)


def lam_general(D):
    g = torch.Generator(device="cuda").manual_seed(900 + D)
    return (0.1 * torch.randn(D, device="cuda", generator=g)).to(BF16)


# ---- the forward kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_forward_with_lam_one_is_the_path_kernel(ops, B, N, D):
    """lam = 1: s, y, mean, rstd have the bits of ops.add_layernorm_path_fwd at rate 0.5 and 0.1; at rate 0 (no flag is drawn)
    s = bf16(x + branch) bit for bit."""
    x, a, _, _, gamma, beta, _, _ = inputs(B, N, D)
    one = lam_ones(D)
    for rate in (0.5, 0.1):
        for seed in seeds_for(B, rate):
            want = ops.add_layernorm_path_fwd(a, x, gamma, beta, B, rate, seed)
            got = ops.add_layernorm_scale_fwd(a, x, one, gamma, beta, B, rate, seed)
            name = ops.last_rowwise_kernel()
            torch.cuda.synchronize()
            assert name == f"add_ln_scale_kernel<{vpl(D)}>", name
            diff = [int((bits(u) != bits(v)).sum()) for u, v in zip(got[:2], want[:2])] + [int((u != v).sum()) for u, v in zip(got[2:], want[2:])]
            print(f"{(B, N, D)} rate {rate} seed {seed}: s / y / mean / rstd differ from the path kernel's in {diff}")
            assert diff == [0, 0, 0, 0]
    s, y, mean, rstd = ops.add_layernorm_scale_fwd(a, x, one, gamma, beta, B)
    torch.cuda.synchronize()
    assert torch.equal(bits(s), bits((x.float() + a.float()).to(BF16)))
    y64, mean64, rstd64 = layernorm_of(s, gamma, beta)
    assert torch.allclose(mean.double(), mean64, atol=1e-5, rtol=0) and torch.allclose(rstd.double(), rstd64, atol=0, rtol=1e-5)


@pytest.mark.parametrize("B,N,D", SHAPES)
def test_forward_with_power_of_two_lam_is_exact(ops, B, N, D):
    """lam[d] = +-2^-(d mod 14) at rate 0.5 (c = 2): kept rows of s are fp32 torch's bf16(x + 2 lam a) bit for bit; dropped images
    keep the bits of x (a planted -0.0 included), and NaNs in their branch rows reach no output."""
    x, a, _, _, gamma, beta, _, _ = inputs(B, N, D)
    lam = lam_pow2(D)
    for seed in seeds_for(B, 0.5):
        flags = keep_flags(seed, 0.5, B)
        kept = rows_of(flags, N)
        s, y, mean, rstd = ops.add_layernorm_scale_fwd(a, x, lam, gamma, beta, B, 0.5, seed)
        poisoned = a.clone()
        poisoned[~kept] = float("nan")
        s2, y2, mean2, rstd2 = ops.add_layernorm_scale_fwd(poisoned, x, lam, gamma, beta, B, 0.5, seed)
        torch.cuda.synchronize()
        want = (x[kept].float() + 2 * lam.float() * a[kept].float()).to(BF16)
        differing = int((bits(s[kept]) != bits(want)).sum())
        print(f"{(B, N, D)} seed {seed} flags {flags.astype(int).tolist()}: kept rows of s differ in {differing} elements")
        assert differing == 0
        assert torch.equal(bits(s[~kept]), bits(x[~kept])), "a dropped image's rows of s are not the bits of x"
        if (~kept).any():
            assert int(bits(s.view(B, N * D)[~torch.from_numpy(flags).cuda(), 0]).unique().item()) == -32768     # -0.0 stays -0.0
        assert all(bool(torch.isfinite(t.float()).all()) for t in (s2, y2, mean2, rstd2))
        assert torch.equal(bits(s2), bits(s)) and torch.equal(bits(y2), bits(y)) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd)


@pytest.mark.parametrize("B,N,D", SHAPES)
def test_forward_with_a_general_lam(ops, B, N, D):
    """lam = 0.1 randn (bf16) at rate 0.1: s at the store-point bar against fp32 math, y at the same bar against fp64 LayerNorm of
    the kernel's own stored s, mean to 1e-5 absolute and rstd to 1e-5 relative."""
    from test_parity_gpu import _store_point
    x, a, _, _, gamma, beta, _, _ = inputs(B, N, D)
    lam, rate = lam_general(D), 0.1
    for seed in seeds_for(B, rate):
        flags = keep_flags(seed, rate, B)
        kept = rows_of(flags, N)
        s, y, mean, rstd = ops.add_layernorm_scale_fwd(a, x, lam, gamma, beta, B, rate, seed)
        torch.cuda.synchronize()
        assert torch.equal(bits(s[~kept]), bits(x[~kept]))
        c = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(rate, dtype=torch.float32))
        rep = []
        if kept.any():
            want = (x[kept].float() + (float(c) * lam.float()) * a[kept].float()).to(BF16)
            _store_point("s", s[kept], want.float().cpu(), rep, 1e-3)
        y64, mean64, rstd64 = layernorm_of(s, gamma, beta)
        _store_point("y", y, y64.to(BF16).float().cpu(), rep, 1e-3)
        em, er = float((mean.double() - mean64).abs().max()), float(((rstd.double() - rstd64).abs() / rstd64).max())
        print(f"{(B, N, D)} seed {seed}: " + ", ".join(f"{t} {f:.1e} (worst {w:.2f} of a step)" for t, f, w in rep)
              + f"; mean abs err {em:.1e}, rstd rel err {er:.1e}")
        assert torch.allclose(mean.double(), mean64, atol=1e-5, rtol=0) and torch.allclose(rstd.double(), rstd64, atol=0, rtol=1e-5)


# ---- the backward kernel ------------------------------------------------------------------------------------------------------
CASES = [(0.1, True), (0.1, False), (0.0, True), (0.0, False)]
CASE_IDS = ["dropout0.1+dx_add", "dropout0.1", "dropout0+dx_add", "dropout0"]


def _same(pairs):
    return [int((bits(u) != bits(v)).sum()) if u.dtype == BF16 else int((u != v).sum()) for u, v in pairs]


@pytest.mark.parametrize("p,add", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_backward_with_lam_one_is_the_path_kernel(ops, B, N, D, p, add):
    """lam = 1.  Rate 0.5: dx, dgamma, dbeta, dx_drop, dcol have the bits of ops.layernorm_bwd_path.  Rate 0 (no flag is drawn): dx,
    dgamma, dbeta and dx_drop (dx itself at p = 0) have the bits of ops.layernorm_bwd.  dcol there cannot have them: this kernel
    sums the ROUNDED dx_drop, as the path kernel does, while ops.layernorm_bwd sums the fp32 values before rounding; it is held
    within the rounding of its addends (2^-8 of the sum of |dx_drop| per column) of that, and to close(5e-3, 5e-3) of the fp64 sum
    of the stored dx_drop."""
    from test_dropout_gpu import close
    x, a, dy, dx_add, gamma, _, mean, rstd = inputs(B, N, D)
    dx_add = dx_add if add else None
    one, dseed = lam_ones(D), 5
    for seed in seeds_for(B, 0.5):
        want = ops.layernorm_bwd_path(dy, x, mean, rstd, gamma, N, 0.5, seed, dx_add=dx_add, drop_p=p, drop_seed=dseed, want_colsum=True)
        dx, dg, db, dxd, dl, dcol = ops.layernorm_bwd_scale(dy, x, mean, rstd, gamma, a, one, N, 0.5, seed, dx_add=dx_add, drop_p=p,
                                                            drop_seed=dseed, want_colsum=True)
        name = ops.last_rowwise_kernel()
        torch.cuda.synchronize()
        assert name == bwd_kernel(D, add), name
        same = _same(zip((dx, dg, db, dxd, dcol), want))
        print(f"{(B, N, D)} p {p} add {add} seed {seed} rate 0.5: dx / dgamma / dbeta / dx_drop / dcol differ from the path kernel's in {same}")
        assert same == [0, 0, 0, 0, 0]
    if p > 0:
        dx0, dg0, db0, dxd0, dcol0 = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dx_add=dx_add, drop_p=p, drop_seed=dseed, want_colsum=True)
    else:
        dx0, dg0, db0, dcol0 = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dx_add=dx_add, want_colsum=True)
        dxd0 = dx0
    dx, dg, db, dxd, dl, dcol = ops.layernorm_bwd_scale(dy, x, mean, rstd, gamma, a, one, N, dx_add=dx_add, drop_p=p, drop_seed=dseed,
                                                        want_colsum=True)
    torch.cuda.synchronize()
    same = _same(((dx, dx0), (dg, dg0), (db, db0), (dxd, dxd0)))
    print(f"{(B, N, D)} p {p} add {add} rate 0: dx / dgamma / dbeta / dx_drop differ from ops.layernorm_bwd's in {same}; "
          f"dcol max diff {float((dcol - dcol0).abs().max()):.2e}")
    assert same == [0, 0, 0, 0]
    # each addend of dcol is a stored bf16 value, within half a bf16 step (2^-8 of itself) of the fp32 value ops.layernorm_bwd adds;
    # 2^-20 of the absolute sum covers the fp32 accumulation of both
    bound = (2.0 ** -8 + 2.0 ** -20) * dxd.float().abs().sum(0)
    assert bool(((dcol - dcol0).abs() <= bound).all()), float(((dcol - dcol0).abs() - bound).max())
    close(dcol, dxd.double().sum(0), rel=5e-3, abs_scale=5e-3)


@pytest.mark.parametrize("p,add", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_backward_with_power_of_two_lam_scales_exactly(ops, B, N, D, p, add):
    """dx_drop with lam[d] = +-2^-(d mod 14) is the lam = 1 result times lam[d], bit for bit; dx, dgamma, dbeta do not depend on lam."""
    x, a, dy, dx_add, gamma, _, mean, rstd = inputs(B, N, D)
    dx_add = dx_add if add else None
    lam = lam_pow2(D)
    seed = seeds_for(B, 0.5)[-1]
    one = ops.layernorm_bwd_scale(dy, x, mean, rstd, gamma, a, lam_ones(D), N, 0.5, seed, dx_add=dx_add, drop_p=p, drop_seed=5)
    two = ops.layernorm_bwd_scale(dy, x, mean, rstd, gamma, a, lam, N, 0.5, seed, dx_add=dx_add, drop_p=p, drop_seed=5)
    torch.cuda.synchronize()
    want = torch.where(one[3] == 0, torch.zeros_like(one[3]), (one[3].float() * lam.float()).to(BF16))      # a masked element is +0, not 0 * lam
    differing = int((bits(two[3]) != bits(want)).sum())
    print(f"{(B, N, D)} p {p} add {add}: dx_drop differs from lam * (the lam = 1 result) in {differing} elements")
    assert differing == 0 and _same(zip(two[:3], one[:3])) == [0, 0, 0]


def _g64(dy, x, mean, rstd, gamma, dx_add):
    """fp64 LayerNorm backward on the kernel's own inputs (the stored fp32 mean / rstd included): the gradient of s."""
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    gy = dy.double() * gamma.double()
    g = rstd.double()[:, None] * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    return g + dx_add.double() if dx_add is not None else g


@pytest.mark.parametrize("p,add", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_backward_with_a_general_lam(ops, B, N, D, p, add):
    """lam = 0.1 randn (bf16), rate 0.5.  dx_drop = bf16(g lam mask / ((1 - p)(1 - rate))) with g the fp32 gradient of s BEFORE its
    own rounding to dx (which is what makes the lam = 1 case the path kernel's bits): it is held (i) at the store-point bar, 1e-3
    of the elements one bf16 step away, against fp64 math on the kernel's own inputs, and (ii) within one bf16 step everywhere of
    fp32 math on the stored dx (that reference starts from a rounded g, so a step's difference is its own rounding, not an error:
    only the distance is asserted against it, not the fraction).  Dropped images: zero rows.  dcol and dlam: fp64 sums of the
    kernel's own stored outputs, close(rel=5e-3, abs_scale=5e-3), as fp32 and in the grad_out bf16 form.  NaNs in the branch rows of
    dropped images change nothing."""
    from test_dropout_gpu import close
    from test_parity_gpu import _store_point
    x, a, dy, dx_add, gamma, _, mean, rstd = inputs(B, N, D)
    dx_add = dx_add if add else None
    lam, rate, dseed = lam_general(D), 0.5, 5
    for seed in seeds_for(B, rate):
        flags = keep_flags(seed, rate, B)
        kept = rows_of(flags, N)
        dx, dg, db, dxd, dl, dcol = ops.layernorm_bwd_scale(dy, x, mean, rstd, gamma, a, lam, N, rate, seed, dx_add=dx_add, drop_p=p,
                                                            drop_seed=dseed, want_colsum=True)
        torch.cuda.synchronize()
        assert int((bits(dxd[~kept]) != 0).sum()) == 0, "a dropped image's rows of dx_drop are not zero"
        ks = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32))
        mask = (ops.dropout_mask(B * N, D, p, dseed) > 0).float() if p > 0 else torch.ones(B * N, D, device="cuda")
        mul = (float(ks) / (1 - rate)) * mask * kept[:, None].float()
        rep = []
        ref64 = (_g64(dy, x, mean, rstd, gamma, dx_add) * lam.double() * mul.double()).float().to(BF16)
        ref32 = (dx.float() * lam.float() * mul).to(BF16)
        worst32 = 0.0
        if kept.any():                                         # (everything dropped: dx_drop is all zeros, asserted above)
            _store_point("dx_drop | fp64 on the inputs", dxd, ref64.float().cpu(), rep, 1e-3)
            d = (dxd.float() - ref32.float()).abs()
            bound = 2.0 ** -7 * torch.maximum(dxd.float().abs(), ref32.float().abs()) + 1e-5 * ref32.float().abs().max()
            worst32 = float((d / bound).max())
        c_rows = kept.double() / (1 - rate)
        dcol64 = dxd.double().sum(0)
        dlam64 = (dx.double() * c_rows[:, None] * torch.where(kept[:, None], a.double(), torch.zeros((), device="cuda", dtype=torch.float64))).sum(0)
        print(f"{(B, N, D)} p {p} add {add} seed {seed} flags {flags.astype(int).tolist()}: " + ", ".join(f"{t} {f:.1e} (worst {w:.2f})" for t, f, w in rep)
              + f"; against fp32 math on the stored dx worst {worst32:.2f} of a step; dcol max err {float((dcol.double() - dcol64).abs().max()):.2e}, "
              f"dlam max err {float((dl.double() - dlam64).abs().max()):.2e} of rms {float(dlam64.pow(2).mean().sqrt()):.2e}")
        assert worst32 <= 1.0
        close(dcol, dcol64, rel=5e-3, abs_scale=5e-3)
        close(dl, dlam64, rel=5e-3, abs_scale=5e-3)
        go = tuple(torch.empty(D, device="cuda", dtype=BF16) for _ in range(4))
        out = ops.layernorm_bwd_scale(dy, x, mean, rstd, gamma, a, lam, N, rate, seed, dx_add=dx_add, drop_p=p, drop_seed=dseed,
                                      want_colsum=True, grad_out=go)
        assert out[1] is go[0] and out[2] is go[1] and out[5] is go[2] and out[4] is go[3] and torch.equal(bits(out[3]), bits(dxd))
        close(go[2], dcol64, rel=5e-3, abs_scale=5e-3)
        close(go[3], dlam64, rel=5e-3, abs_scale=5e-3)
        close(go[0], dg, rel=5e-3, abs_scale=5e-3)
        close(go[1], db, rel=5e-3, abs_scale=5e-3)
        poisoned = a.clone()
        poisoned[~kept] = float("nan")
        again = ops.layernorm_bwd_scale(dy, x, mean, rstd, gamma, poisoned, lam, N, rate, seed, dx_add=dx_add, drop_p=p, drop_seed=dseed,
                                        want_colsum=True)
        torch.cuda.synchronize()
        assert _same(zip(again, (dx, dg, db, dxd, dl, dcol))) == [0] * 6


def test_backward_deferred_reductions(ops):
    """With sfcvit_reduce_defer on, the call queues its FOUR reductions; the outputs are untouched before the flush and equal to
    the direct call's after it."""
    from sfcvit._lib import lib
    B, N, D = 3, 7, 520
    x, a, dy, _, gamma, _, mean, rstd = inputs(B, N, D)
    lam, seed = lam_general(D), seeds_for(B, 0.5)[0]
    _, dg0, db0, dxd0, dl0, dcol0 = ops.layernorm_bwd_scale(dy, x, mean, rstd, gamma, a, lam, N, 0.5, seed, drop_p=0.1, drop_seed=5,
                                                            want_colsum=True)
    dx, dxd = torch.empty_like(x), torch.empty_like(x)
    dg, db, dcol, dl = (torch.full((D,), float("nan"), device="cuda") for _ in range(4))
    ws = torch.empty(lib.sfcvit_layernorm_bwd_scale_ws(B * N, D), device="cuda", dtype=torch.uint8)      # alive until the flush
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())                                                         # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sfcvit_reduce_pending() == 0
    lib.sfcvit_reduce_defer(1)
    try:
        rc = lib.sfcvit_layernorm_bwd_scale(p_(dy), p_(x), p_(mean), p_(rstd), p_(gamma), None, p_(a), p_(lam), p_(dx), p_(dxd), 0.1, 5,
                                            None, p_(dg), p_(db), p_(dcol), p_(dl), 0, B, N, D, p_(ws), 0.5, seed, stream)
    finally:
        lib.sfcvit_reduce_defer(0)
    pending = lib.sfcvit_reduce_pending()
    torch.cuda.synchronize()
    untouched = all(bool(torch.isnan(t).all()) for t in (dg, db, dcol, dl))
    ops.flush_deferred()
    torch.cuda.synchronize()
    print(f"rc {rc}, {pending} reductions queued, outputs untouched before the flush: {untouched}")
    assert rc == 0 and pending == 4 and untouched and lib.sfcvit_reduce_pending() == 0
    assert torch.equal(dg, dg0) and torch.equal(db, db0) and torch.equal(dcol, dcol0) and torch.equal(dl, dl0)
    assert torch.equal(bits(dxd), bits(dxd0))


# ---- the layer ----------------------------------------------------------------------------------------------------------------
LAYER = (5, 68, 128, 2, 256)


def _layer_params(B, N, D, H, Fd):
    g = torch.Generator(device="cuda").manual_seed(5)
    r = lambda *s, sc=1.0: (torch.randn(*s, device="cuda", generator=g) * sc)     # noqa: E731
    bf = lambda t: t.to(BF16)                                                       # noqa: E731
    s = bf(r(B, N, D))
    P = dict(in_w=bf(r(3 * D, D, sc=D ** -0.5)), in_b=bf(r(3 * D, sc=0.1)), out_w=bf(r(D, D, sc=D ** -0.5)),
             out_b=bf(r(D, sc=0.1)), n2_w=bf(1 + r(D, sc=0.1)), n2_b=bf(r(D, sc=0.1)),
             w1=bf(r(Fd, D, sc=D ** -0.5)), b1=bf(r(Fd, sc=0.1)), w2=bf(r(D, Fd, sc=Fd ** -0.5)), b2=bf(r(D, sc=0.1)),
             next_w=bf(1 + r(D, sc=0.1)), next_b=bf(r(D, sc=0.1)))
    n = bf(torch.nn.functional.layer_norm(s.float(), (D,), 1 + r(D, sc=0.1), r(D, sc=0.1)))
    lam = bf(r(2, D, sc=0.1))
    return s, n, P, lam, bf(r(B, N, D)), bf(r(B, N, D))


def _run_layer(ops, act, with_lam, rate, masked=False, biased=False):
    import sfcvit.functional as F
    from sfcvit import masks, relpos
    from attn_bias_ref import bias_term
    from test_dropout_gpu import close
    from test_parity_gpu import _store_point
    B, N, D, H, Fd = LAYER
    p, M = 0.1, B * N
    seeds, pseeds = (11, 22, 33, 44), (66, 1234)
    k1, k2 = (keep_flags(s_, rate, B) for s_ in pseeds) if rate > 0 else (np.ones(B, bool), np.ones(B, bool))
    if rate > 0:
        assert 0 < k1.sum() < B and 0 < k2.sum() < B and not np.array_equal(k1, k2)
    s, n, P, lam, ds, dn = _layer_params(B, N, D, H, Fd)
    window = masks.curve_window(N, 8) if masked else None
    am = ops.as_attention_mask(window, N) if masked else None
    table = index = None
    if biased:
        idx, T = relpos.curve_offsets(N, 20)
        index = ops.AttentionBiasIndex(idx, T)
        table = (0.5 * torch.randn(H, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))).requires_grad_(True)
    leaves = [s.clone().requires_grad_(True), n.clone().requires_grad_(True)] + [P[k].clone().requires_grad_(True) for k in prenorm_ref.ORDER]
    lam_leaf = lam.clone().requires_grad_(True) if with_lam else None
    cfg = F._LayerCfg(H, 1e-5, p, seeds, None, act, am, (rate, pseeds) if rate > 0 else None, index)
    ops.KERNEL_LOG = []
    try:
        s2, n2 = F._PreNormLayer.apply(*leaves, lam_leaf, table, cfg)
        saved = [t.detach() for t in s2.grad_fn.saved_tensors]
        torch.autograd.backward([s2, n2], [ds, dn])
        ran = list(ops.KERNEL_LOG)
    finally:
        ops.KERNEL_LOG = None
    # the launch rules
    if with_lam:
        assert ran.count("add_ln_scale_kernel<1>") == 2 and ran.count("ln_bwd_scale_kernel<1, true>") == 2 and not any("path" in k for k in ran), ran
    elif rate > 0:
        assert ran.count("add_ln_path_kernel<1>") == 2 and ran.count("ln_bwd_path_kernel<1, true>") == 2 and not any("scale" in k for k in ran), ran
    else:
        assert not any("scale" in k or "path" in k for k in ran) and ran.count("ln_bwd_kernel<1, true>") == 2, ran
    assert masked == any("masked" in k for k in ran) and biased == any("attn_bias" in k for k in ran)

    ma = ops.dropout_mask(B * H * N, N, p, seeds[0]).float().view(B, H, N, N)
    m1 = ops.dropout_mask(M, D, p, seeds[1]).float().view(B, N, D)
    mf = ops.dropout_mask(M, Fd, p, seeds[2]).float().view(B, N, Fd)
    m2 = ops.dropout_mask(M, D, p, seeds[3]).float().view(B, N, D)
    c1, c2 = (torch.from_numpy(k).cuda().float() / (1 - rate) for k in (k1, k2))
    sr, nr = s.float().requires_grad_(True), n.float().requires_grad_(True)
    R = {k: v.float().requires_grad_(True) for k, v in P.items()}
    lr = lam.float().requires_grad_(True) if with_lam else None
    tr = table.detach().clone().requires_grad_(True) if biased else None
    inter = {}
    s2r, n2r = prenorm_ref.pre_norm_layer(sr, nr, R, H, (ma, m1, mf, m2), c1, c2, (lr[0], lr[1]) if with_lam else None, act,
                                          attn_mask=window.cuda() if masked else None,
                                          rel_bias=bias_term(tr, idx.cuda()) if biased else None, keep=inter)
    torch.autograd.backward([s2r, n2r], [ds.float(), dn.float()])
    tag = f"{act} lam={with_lam} drop_path={rate}" + (" masked" if masked else "") + (" rel_bias" if biased else "")
    print(f"[{tag}] s' max err {float((s2.float() - s2r.detach()).abs().max()):.3e}, n' max err {float((n2.float() - n2r.detach()).abs().max()):.3e}")
    close(s2, s2r.detach(), rel=1 / 32, abs_scale=1 / 24)
    close(n2, n2r.detach(), rel=1 / 32, abs_scale=1 / 24)
    pairs = list(zip(["s", "n"] + prenorm_ref.ORDER, leaves, [sr, nr] + [R[k] for k in prenorm_ref.ORDER]))
    if with_lam:
        pairs.append(("lam", lam_leaf, lr))
    if biased:
        pairs.append(("rel_table", table, tr))
    for name, got, ref in pairs:
        gg, rr = got.grad.float().flatten(), ref.grad.flatten()
        cos, ratio = float(torch.dot(gg, rr) / (gg.norm() * rr.norm() + 1e-30)), float(gg.norm() / rr.norm())
        print(f"    d{name}: cosine {cos:.5f}, norm ratio {ratio:.4f}")
        assert cos > 0.99, (name, cos)
        assert abs(ratio - 1) < 5e-2, (name, ratio)

    # the bf16 stores this layer adds, each against fp32 math on the HIP path's own inputs to it
    rb = lambda t: t.to(BF16).float()                                              # noqa: E731
    cpu = lambda t: t.detach().float().cpu()                                       # noqa: E731
    n0, _, o_s, _, s1_s, n1_s, _, _, h_s, s2_s = saved[:10]
    opt = saved[18:]
    W = {k: cpu(v) for k, v in P.items()}
    ln = lambda t, w_, b_: torch.nn.functional.layer_norm(t, (D,), w_, b_, 1e-5)    # noqa: E731
    rep = []
    if with_lam or rate > 0:
        a_s = ops.gemm(o_s.view(M, D), P["out_w"], bias=P["out_b"], dropout_p=p, dropout_seed=seeds[1])       # the branch stores, again
        f_s = ops.gemm(h_s, P["w2"], bias=P["b2"], dropout_p=p, dropout_seed=seeds[3])
        l1, l2 = (cpu(lam[0]), cpu(lam[1])) if with_lam else (1.0, 1.0)
        r1, r2 = (cpu(c).repeat_interleave(N)[:, None] for c in (c1, c2))
        _store_point("s1 = s + c1 lam1 a", s1_s, rb(cpu(s).view(M, D) + (r1 * l1) * cpu(a_s)), rep, 1e-3)
        _store_point("s2 = s1 + c2 lam2 f", s2_s, rb(cpu(s1_s) + (r2 * l2) * cpu(f_s)), rep, 1e-3)
        d1, d2 = (torch.from_numpy(np.repeat(~k, N)) for k in (k1, k2))
        assert torch.equal(bits(s1_s.cpu()[d1]), bits(s.view(M, D).cpu()[d1])) and torch.equal(bits(s2_s.cpu()[d2]), bits(s1_s.cpu()[d2]))
    _store_point("n1 = LN2(s1)", n1_s, rb(ln(cpu(s1_s), W["n2_w"], W["n2_b"])), rep, 1e-3)
    _store_point("n' = LN_next(s')", n2.view(M, D), rb(ln(cpu(s2_s), W["next_w"], W["next_b"])), rep, 1e-3)
    if act == "gelu":
        u_s = opt[1] if with_lam else opt[0]
        ks = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)))
        _store_point("h = drop(gelu(u))", h_s, rb(torch.nn.functional.gelu(cpu(u_s)) * (cpu(mf).view(M, Fd) > 0).float() * ks), rep, 1e-3)
    print(f"[{tag} store points] " + ", ".join(f"{t} {f:.1e}" for t, f, _ in rep))


@pytest.mark.parametrize("rate", [0.0, 0.5], ids=["no_drop_path", "drop_path0.5"])
@pytest.mark.parametrize("with_lam", [False, True], ids=["no_lam", "lam"])
@pytest.mark.parametrize("act", ["relu", "gelu"])
def test_layer_against_the_fp32_reference(ops, act, with_lam, rate):
    """(B, N, D, H, F) = (5, 68, 128, 2, 256), dropout 0.1, against fp32 torch autograd of prenorm_ref with the same masks and flags
    at the bars of the post-norm layer test: outputs close(1/32, 1/24), every gradient (s, n, the weights, lam, the following norm)
    cosine > 0.99 and norm within 5 %; the layer's bf16 stores at the store-point bar; the launch rules in ops.KERNEL_LOG."""
    _run_layer(ops, act, with_lam, rate)


def test_layer_with_a_curve_window(ops):
    _run_layer(ops, "gelu", True, 0.5, masked=True)


def test_layer_with_a_relative_position_bias(ops):
    _run_layer(ops, "gelu", True, 0.5, biased=True)


# ---- models -------------------------------------------------------------------------------------------------------------------
def _tiny_model(rate=0.0, dropout=0.0, seed=11, name="hilbert32_1d", **kw):
    cfg, batch = MODEL_CASES[name]
    torch.manual_seed(seed)
    model = build_with(cfg, dropout_p=dropout, head_dropout_p=dropout, drop_path_rate=rate, **kw)
    x = formula.image_batch(batch, 3, cfg.img_size, cfg.img_size).cuda()
    tgt = formula.soft_targets(batch, cfg.num_classes).cuda()
    return model.to("cuda", dtype=BF16), x, tgt, cfg


def test_eval_logits_against_the_torch_module_tree():
    """A norm_first GELU model with lam = 1 in eval: its encoder replaced by torch's own nn.TransformerEncoder(norm_first layers,
    norm=LayerNorm) in fp32 on the CPU, loaded with the same weights and fed the HIP model's own encoder input; logits within
    3e-2 of the largest reference logit, the eval bar of the post-norm model."""
    from test_parity_gpu import LOGIT_TOL
    model, x, _, cfg = _tiny_model(norm_first=True, activation="gelu", layer_scale=1.0)
    with torch.no_grad():
        for k, prm in model.encoder.transformer.named_parameters():               # norms and biases away from ones and zeros
            if prm.dim() == 1:
                prm.add_((0.1 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(len(k)))).to(prm))
    model.eval()
    tree = prenorm_ref.torch_encoder(cfg.embed_dim, cfg.n_heads, cfg.mlp_dim, cfg.depth, "gelu").eval()
    tree.load_state_dict({k: v.float().cpu() for k, v in model.encoder.transformer.state_dict().items()}, strict=True)
    with torch.no_grad():
        got = model(x).float().cpu()
        t = model.mlp_mixer(model.patch_embed(x))
        want_tokens = tree(t.float().cpu())
        want = model.mlp_head(want_tokens.to("cuda", dtype=BF16)).float().cpu()
        enc = model.encoder(t).float().cpu()
    scale = float(want.abs().max())
    err, tok_err = float((got - want).abs().max()), float((enc - want_tokens).abs().max() / want_tokens.abs().max())
    print(f"logits max err {err:.3e} of {scale:.3e}; encoder output max err {tok_err:.3e} of its largest value")
    assert err <= LOGIT_TOL * scale and tok_err <= LOGIT_TOL


def test_post_norm_is_unchanged(ops):
    """norm_first=False gives the bits of a model constructed without the keyword: logits, every gradient, and the same launches."""
    import sfcvit.functional as F
    runs = []
    for kw in ({}, dict(norm_first=False, activation="relu", layer_scale=None)):
        model, x, tgt, _ = _tiny_model(0.1, dropout=0.1, **kw)
        model.train()
        torch.manual_seed(5)
        ops.KERNEL_LOG = []
        try:
            logits = model(x)
            F.soft_target_cross_entropy(logits, tgt).backward()
            runs.append((logits.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, list(ops.KERNEL_LOG)))
        finally:
            ops.KERNEL_LOG = None
    (l0, g0, log0), (l1, g1, log1) = runs
    assert torch.equal(bits(l0), bits(l1)) and log0 == log1 and not any("scale" in k for k in log1)
    assert list(g0) == list(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)


def test_training_gradients_reach_layer_scale_and_the_final_norm(ops):
    import sfcvit.functional as F
    model, x, tgt, cfg = _tiny_model(0.1, dropout=0.1, norm_first=True, activation="gelu", layer_scale=0.1)
    model.train()
    ops.KERNEL_LOG = []
    try:
        torch.manual_seed(5)
        F.soft_target_cross_entropy(model(x), tgt).backward()
        log = list(ops.KERNEL_LOG)
    finally:
        ops.KERNEL_LOG = None
    assert log.count("add_ln_scale_kernel<1>") == 2 * cfg.depth and sum(k.startswith("ln_bwd_scale_kernel<1") for k in log) == 2 * cfg.depth, log
    for k, prm in model.named_parameters():
        if not k.startswith("mlp_mixer.token_mix"):
            assert prm.grad is not None and torch.isfinite(prm.grad.float()).all(), k
    for k in ["encoder.transformer.norm.weight", "encoder.transformer.norm.bias"] + [f"encoder.layer_scale.{l}" for l in range(cfg.depth)]:
        g = dict(model.named_parameters())[k].grad
        assert float(g.float().abs().max()) > 0, k
    assert all(float(prm.grad[r].float().abs().max()) > 0 for prm in model.encoder.layer_scale for r in (0, 1))


def test_flat_gradient_buffer_receives_layer_scale_rows():
    """FusedAdamW's flat gradient buffer: both rows of every layer's LayerScale gradient are written into the parameter's slot, and
    equal the gradients of a run without slots."""
    import sfcvit.functional as F
    from sfcvit.training import FusedAdamW
    grads = []
    for slots in (False, True):
        model, x, tgt, cfg = _tiny_model(0.0, norm_first=True, activation="gelu", layer_scale=0.1)
        model.train()
        if slots:
            opt = FusedAdamW(model.parameters(), lr=0.0, weight_decay=0.0)     # noqa: F841  (attaches the slots)
        F.soft_target_cross_entropy(model(x), tgt).backward()
        torch.cuda.synchronize()
        grads.append({k: p.grad.float().clone() for k, p in model.named_parameters() if p.grad is not None})
    for k in grads[0]:
        if "layer_scale" in k or "transformer.norm" in k:
            a, b = grads[0][k], grads[1][k]
            assert float((a - b).abs().max()) <= 2.0 ** -7 * float(a.abs().max()) + 1e-12, k


def test_graphed_step_draws_new_flags_every_replay():
    """Dropout 0, rate 0.5, learning rate 0, pre-norm with LayerScale: the parameters stand still, so four replays on one batch
    differ only by the flags the device seed offset gives them."""
    from sfcvit import ops
    from sfcvit.training import FusedAdamW, GraphedTrainStep
    try:
        model, x, tgt, _ = _tiny_model(0.5, norm_first=True, activation="gelu", layer_scale=0.5)
        model.train()
        opt = FusedAdamW(model.parameters(), lr=0.0, weight_decay=0.0)
        opt.use_device_state(seed_base=4242)
        step = GraphedTrainStep(model, x.clone(), tgt.clone(), opt, warmup=2, preserve_state=False)
        losses = [float(step()) for _ in range(4)]
        print(losses)
        assert all(np.isfinite(losses)) and len(set(losses)) > 1, losses
        step.close()
    finally:
        ops.STEP_STATE = None


def _main_py(tmp_path, *extra):
    main = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd", "main.py")
    return [sys.executable, main, "--synthetic", "--tokenizer", "hilbert", "--img-size", "32", "--patch-size", "16", "--embed-dim", "64",
            "--depth", "2", "--heads", "1", "--mlp-dim", "128", "--batch-size", "64", "--train-size", "256", "--test-size", "128",
            "--warmup-epochs", "0", "--pre-norm", "--activation", "gelu", "--layer-scale", "--drop-path", "0.1",
            "--checkpoint-dir", str(tmp_path), *extra]


@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
def test_main_py_trains_and_resumes(tmp_path, graph):
    g = ["--graph"] if graph else []
    out = subprocess.run(_main_py(tmp_path, "--epochs", "1", *g), capture_output=True, text=True, timeout=300)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stderr[-3000:]
    assert "Epoch 1/1" in out.stdout, out.stdout[-1000:]
    ck = os.path.join(str(tmp_path), "checkpoint_hilbert.pt")
    sd = torch.load(ck, map_location="cpu", weights_only=True)["model_state_dict"]
    assert {"encoder.layer_scale.0", "encoder.layer_scale.1", "encoder.transformer.norm.weight", "encoder.transformer.norm.bias"} <= set(sd)
    assert tuple(sd["encoder.layer_scale.1"].shape) == (2, 64) and not any("drop" in k for k in sd)
    out = subprocess.run(_main_py(tmp_path, "--epochs", "2", "--resume", ck, *g), capture_output=True, text=True, timeout=300)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stderr[-3000:]
    assert "Epoch 2/2" in out.stdout and "Epoch 1/2" not in out.stdout, out.stdout[-1000:]


def test_torch_compile_refuses_a_pre_norm_model():
    import sfcvit.library  # noqa: F401  (registers the ops)
    model, x, _, _ = _tiny_model(norm_first=True)
    try:
        model.eval()
        with pytest.raises(NotImplementedError, match="the pre-norm layer has no traced form"):
            with torch.no_grad():
                torch.compile(model)(x)
    finally:
        torch._dynamo.reset()


def test_attention_report_on_a_pre_norm_model():
    """sfcvit.analysis on a 2-layer pre-norm GELU model with LayerScale: the logits are the model's own eval bits, and the attention
    distance and entropy per layer and head agree with an fp32 restatement on the same weights within the tolerance the post-norm
    report is held to."""
    from sfcvit.analysis import attention_report, token_positions
    from test_attention_probe_gpu import TOL_F32, TOL_MODEL
    model, x, _, cfg = _tiny_model(norm_first=True, activation="gelu", layer_scale=0.5)
    assert cfg.depth == 2
    model.train()
    rep = attention_report(model, x, maps=True, head_mean=False)
    assert model.training
    with torch.no_grad():
        want = model.eval()(x)
    assert torch.equal(rep["logits"], want)
    f = lambda t: t.detach().float().cpu()                                         # noqa: E731
    pos = token_positions(model.patch_embed)
    dmat = (pos[:, None] - pos[None]).norm(dim=-1)
    with torch.no_grad():
        s = f(model.mlp_mixer(model.patch_embed(x)))
    enc, H = model.encoder, model.encoder.n_head
    B, N, D = s.shape
    layers, final = prenorm_ref.layers_of(enc.transformer)
    ref = []
    n = torch.nn.functional.layer_norm(s, (D,), f(layers[0]["n1_w"]), f(layers[0]["n1_b"]))
    for l, L in enumerate(layers):
        qkv = (n @ f(L["in_w"]).T + f(L["in_b"])).reshape(B, N, 3, H, D // H)
        q, k = (qkv[:, :, i].transpose(1, 2) for i in range(2))
        P = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(D // H), dim=-1)
        ref.append(((P * dmat).sum(-1).mean(-1), -(P * torch.log(P.clamp_min(1e-30))).sum(-1).mean(-1)))
        nxt = (layers[l + 1]["n1_w"], layers[l + 1]["n1_b"]) if l + 1 < len(layers) else final
        Pf = {k_: f(v) for k_, v in dict(L, next_w=nxt[0], next_b=nxt[1]).items()}
        s, n = prenorm_ref.pre_norm_layer(s, n, Pf, H, lam=(f(enc.layer_scale[l][0]), f(enc.layer_scale[l][1])), act="gelu")
    dscale, escale = float(dmat.max()), max(math.log(N), 1.0)
    assert [e["layer"] for e in rep["layers"]] == [0, 1]
    for e, (dref, eref) in zip(rep["layers"], ref):
        assert tuple(e["map"].shape) == (B, H, N, N) and e["mass_error"] <= TOL_F32
        fd = float((e["distance"].cpu() - dref).abs().max()) / dscale
        fe = float((e["entropy"].cpu() - eref).abs().max()) / escale
        print(f"FIGURE pre-norm model layer {e['layer']}: distance={fd:.3e} entropy={fe:.3e} mass={e['mass_error']:.3e}")
        assert fd <= TOL_MODEL and fe <= TOL_MODEL, (fd, fe)
