"""Stochastic depth (DropPath) on the HIP encoder path: the keep flags against their numpy restatement, the fused scaled-residual +
LayerNorm forward kernel and the PATH LayerNorm backward bit for bit where the arithmetic is exact (dropped rows, rate 0.5) and at
the layer's store-point bar elsewhere, the encoder layer against an fp32 reference with the same masks and flags, and the models,
the captured step, main.py and torch.compile."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from drop_path_ref import encoder_layer as ref_layer, keep_flags, layernorm_of
from oracle import formula
from oracle.cases import MODEL_CASES
from token_pool_ref import build_with

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
# (B, N, D): one row; two images of one row; odd everything; more than one block; two vectors per lane with a tail; four vectors
# per lane; the backward's width limit; the two widths with kernels of their own at M >= 4096, N odd (a grid-stride walk and the
# rows of one workgroup cross image boundaries)
SHAPES = [(1, 1, 8), (2, 1, 8), (5, 3, 72), (2, 65, 200), (3, 7, 520), (2, 9, 1536), (2, 3, 2048), (22, 197, 768), (8, 577, 1024)]
LISTED_SEEDS = (44, 66, 1234, 1235, 77, 4242, 11, 22)


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int16)


def seeds_for(B, rate):
    """Seeds whose numpy flags hold both values (B >= 2: one seed, a listed one where there is one) or, for one image, a seed that
    drops it and a seed that keeps it."""
    order = list(LISTED_SEEDS) + list(range(1, 4000))
    if B == 1:
        return [next(s for s in order if not keep_flags(s, rate, 1)[0]), next(s for s in order if keep_flags(s, rate, 1)[0])]
    return [next(s for s in order if 0 < keep_flags(s, rate, B).sum() < B)]


def rows_of(flags, N):
    return torch.from_numpy(np.repeat(flags, N)).cuda()


@functools.lru_cache(maxsize=None)
def inputs(B, N, D):
    """bf16-rounded randn inputs of a shape, made once and left unchanged: x (a -0.0 planted in the first element of every image),
    branch, dy, dx_add, gamma, beta, and LayerNorm's statistics of x for the backward."""
    from sfcvit import ops
    g = torch.Generator(device="cuda").manual_seed(1000 * B + 10 * N + D)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g).to(BF16)          # noqa: E731
    x, a, dy, add = r(B * N, D), r(B * N, D), r(B * N, D), r(B * N, D)
    x.view(B, N * D)[:, 0] = -0.0
    gamma, beta = (1 + 0.1 * torch.randn(D, device="cuda", generator=g)).to(BF16), (0.1 * torch.randn(D, device="cuda", generator=g)).to(BF16)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
    return x, a, dy, add, gamma, beta, mean, rstd


def fwd_kernel(D):
    return f"add_ln_path_kernel<{1 if D <= 512 else 2 if D <= 1024 else 4 if D <= 2048 else 8}>"


def bwd_kernel(D, add):
    tf = "true" if add else "false"
    if D in (768, 1024):
        return f"ln_bwd_cols_path_kernel<{D // 256}, {tf}>"
    return f"ln_bwd_path_kernel<{1 if D <= 512 else 2 if D <= 1024 else 4}, {tf}>"


# ---- 1. flags -----------------------------------------------------------------------------------------------------------------
def test_flags_equal_the_numpy_restatement(ops):
    n = 0
    for B in sorted({s[0] for s in SHAPES} | {4096}):
        for seed in LISTED_SEEDS:
            for rate in (0.1, 0.25, 0.5):
                got = ops.drop_path_keep(B, rate, seed).cpu().numpy()
                assert got.dtype == np.bool_ and got.shape == (B,)
                assert np.array_equal(got, keep_flags(seed, rate, B)), (B, seed, rate)
                n += 1
    print(f"{n} (B, seed, rate) flag vectors equal")


# ---- 2-5, 10. the forward kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.5, 0.1])
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_forward_kernel(ops, B, N, D, rate):
    """Dropped rows: s has the bits of x (a planted -0.0 included).  Kept rows: s = bf16(x + c * branch) -- bit for bit at rate 0.5
    (c = 2 is an exact multiply), at the store-point bar (1e-3 of the elements one bf16 step away) at rate 0.1.  y, mean and rstd
    are LayerNorm (fp64) of the kernel's own stored s."""
    from test_parity_gpu import _store_point
    x, a, _, _, gamma, beta, _, _ = inputs(B, N, D)
    for seed in seeds_for(B, rate):
        flags = keep_flags(seed, rate, B)
        kept = rows_of(flags, N)
        s, y, mean, rstd = ops.add_layernorm_path_fwd(a, x, gamma, beta, B, rate, seed)
        name = ops.last_rowwise_kernel()
        torch.cuda.synchronize()
        assert name == fwd_kernel(D), name
        assert torch.equal(bits(s[~kept]), bits(x[~kept])), "a dropped image's rows of s are not the bits of x"
        if (~kept).any():
            assert int(bits(s.view(B, N * D)[~torch.from_numpy(flags).cuda(), 0]).unique().item()) == -32768     # -0.0 stays -0.0
        c = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(rate, dtype=torch.float32))
        want = (x[kept].float() + float(c) * a[kept].float()).to(BF16)
        rep = []
        if rate == 0.5:
            differing = int((bits(s[kept]) != bits(want)).sum())
            print(f"{(B, N, D)} rate {rate} seed {seed} flags {flags.astype(int).tolist()}: kept rows of s differ in {differing} elements")
            assert differing == 0
        elif kept.any():
            _store_point("s", s[kept], want.float().cpu(), rep, 1e-3)
        y64, mean64, rstd64 = layernorm_of(s, gamma, beta)
        _store_point("y", y, y64.to(BF16).float().cpu(), rep, 1e-3)
        em, er = float((mean.double() - mean64).abs().max()), float(((rstd.double() - rstd64).abs() / rstd64).max())
        print(f"{(B, N, D)} rate {rate} seed {seed}: " + ", ".join(f"{t} {f:.1e} (worst {w:.2f} of a step)" for t, f, w in rep)
              + f"; mean abs err {em:.1e}, rstd rel err {er:.1e}")
        assert torch.allclose(mean.double(), mean64, atol=1e-5, rtol=0) and torch.allclose(rstd.double(), rstd64, atol=0, rtol=1e-5)


# ---- 6-8, 10. the backward kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,add", [(0.1, True), (0.0, False)], ids=["dropout0.1+dx_add", "dropout0"])
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_backward_kernel(ops, B, N, D, p, add):
    """dx, dgamma, dbeta: the bits of ops.layernorm_bwd without a path.  dx_drop at path rate 0.5: zeros for dropped images, twice
    the existing dropout variant's dx_drop (twice dx at p = 0) for kept ones, bit for bit.  dcol: the fp64 column sum of the stored
    dx_drop, as fp32 and as bf16 (grad_out)."""
    from test_dropout_gpu import close
    x, _, dy, dx_add, gamma, _, mean, rstd = inputs(B, N, D)
    dx_add = dx_add if add else None
    rate, dseed = 0.5, 5
    if p > 0:
        dx0, dg0, db0, dxd0 = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dx_add=dx_add, drop_p=p, drop_seed=dseed)
    else:
        dx0, dg0, db0 = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dx_add=dx_add)
        dxd0 = dx0
    for seed in seeds_for(B, rate):
        flags = keep_flags(seed, rate, B)
        kept = rows_of(flags, N)
        dx, dg, db, dxd, dcol = ops.layernorm_bwd_path(dy, x, mean, rstd, gamma, N, rate, seed, dx_add=dx_add, drop_p=p, drop_seed=dseed,
                                                       want_colsum=True)
        name = ops.last_rowwise_kernel()
        torch.cuda.synchronize()
        assert name == bwd_kernel(D, add), name
        same = [int((bits(u) != bits(v)).sum()) if u.dtype == BF16 else int((u != v).sum()) for u, v in ((dx, dx0), (dg, dg0), (db, db0))]
        twice = (2 * dxd0[kept].float()).to(BF16)
        differing = int((bits(dxd[kept]) != bits(twice)).sum())
        nonzero = int((bits(dxd[~kept]) != 0).sum())
        ref = dxd.double().sum(0)
        print(f"{(B, N, D)} p {p} seed {seed} flags {flags.astype(int).tolist()}: dx / dgamma / dbeta differ in {same}; dropped rows of "
              f"dx_drop non-zero in {nonzero}; kept rows differ from twice the dropout variant's in {differing}; "
              f"dcol max err {float((dcol.double() - ref).abs().max()):.2e} of rms {float(ref.pow(2).mean().sqrt()):.2e}")
        assert same == [0, 0, 0]
        assert nonzero == 0 and differing == 0
        close(dcol, ref, rel=5e-3, abs_scale=5e-3)
        go = tuple(torch.empty(D, device="cuda", dtype=BF16) for _ in range(3))
        out = ops.layernorm_bwd_path(dy, x, mean, rstd, gamma, N, rate, seed, dx_add=dx_add, drop_p=p, drop_seed=dseed,
                                     want_colsum=True, grad_out=go)
        assert out[1] is go[0] and out[2] is go[1] and out[4] is go[2] and torch.equal(bits(out[3]), bits(dxd))
        print(f"    grads_bf16: dcol max err {float((go[2].double() - ref).abs().max()):.2e}")
        close(go[2], ref, rel=5e-3, abs_scale=5e-3)
        close(go[0], dg0, rel=5e-3, abs_scale=5e-3)
        close(go[1], db0, rel=5e-3, abs_scale=5e-3)


def test_backward_deferred_reduction(ops):
    """With sfcvit_reduce_defer on, the call queues its three reductions; after the flush dgamma, dbeta and dcol are those of the
    direct call."""
    from sfcvit._lib import lib
    B, N, D = 3, 7, 520
    x, _, dy, _, gamma, _, mean, rstd = inputs(B, N, D)
    seed = seeds_for(B, 0.5)[0]
    _, dg0, db0, dxd0, dcol0 = ops.layernorm_bwd_path(dy, x, mean, rstd, gamma, N, 0.5, seed, drop_p=0.1, drop_seed=5, want_colsum=True)
    dx, dxd = torch.empty_like(x), torch.empty_like(x)
    dg, db, dcol = (torch.full((D,), float("nan"), device="cuda") for _ in range(3))
    ws = torch.empty(lib.sfcvit_layernorm_bwd_ws(B * N, D), device="cuda", dtype=torch.uint8)      # alive until the flush
    p_ = lambda t: ctypes.c_void_p(t.data_ptr())                                                  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sfcvit_reduce_pending() == 0
    lib.sfcvit_reduce_defer(1)
    try:
        rc = lib.sfcvit_layernorm_bwd_path(p_(dy), p_(x), p_(mean), p_(rstd), p_(gamma), None, p_(dx), p_(dxd), 0.1, 5, None, p_(dg),
                                           p_(db), p_(dcol), 0, B, N, D, p_(ws), 0.5, seed, stream)
    finally:
        lib.sfcvit_reduce_defer(0)
    pending = lib.sfcvit_reduce_pending()
    torch.cuda.synchronize()
    untouched = bool(torch.isnan(dg).all() and torch.isnan(db).all() and torch.isnan(dcol).all())
    ops.flush_deferred()
    torch.cuda.synchronize()
    print(f"rc {rc}, {pending} reductions queued, outputs untouched before the flush: {untouched}")
    assert rc == 0 and pending == 3 and untouched and lib.sfcvit_reduce_pending() == 0
    assert torch.equal(dg, dg0) and torch.equal(db, db0) and torch.equal(dcol, dcol0) and torch.equal(bits(dxd), bits(dxd0))


def test_backward_all_kept_doubles_the_column_sums(ops):
    """Seed 11 at rate 0.5 keeps both of two images; at dropout 0 the outgoing gradient is then 2 dx everywhere, and its column
    sums -- taken from the rounded values, in the order of the kernel without a path -- are the fp32 sums of bf16(2 dx)."""
    B, seed = 2, 11
    assert keep_flags(seed, 0.5, B).all()
    for N, D in ((65, 200), (2048, 768)):
        x, _, dy, _, gamma, _, mean, rstd = inputs(B, N, D)
        dx0, _, _ = ops.layernorm_bwd(dy, x, mean, rstd, gamma)
        dx, _, _, dxd, dcol = ops.layernorm_bwd_path(dy, x, mean, rstd, gamma, N, 0.5, seed, want_colsum=True)
        ref = (2 * dx0.double()).sum(0)
        err = float((dcol.double() - ref).abs().max() / ref.abs().max())
        print((B, N, D), "dx_drop == 2 dx:", bool(torch.equal(bits(dxd), bits((2 * dx0.float()).to(BF16)))), f"dcol rel err {err:.1e}")
        assert torch.equal(bits(dxd), bits((2 * dx0.float()).to(BF16))) and torch.equal(bits(dx), bits(dx0))
        assert err <= 1e-5            # fp32 accumulation of B * N exactly representable addends: 2^-24 sqrt(B N) at the worst


# ---- 9. everything dropped ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(1, 8), (65, 200), (2048, 768)])
def test_all_dropped(ops, N, D):
    """Seed 22 at rate 0.5 drops both of two images: s == x, dx_drop == 0, dcol == 0; the branch is not read (NaNs in it reach
    nothing)."""
    B, seed = 2, 22
    assert not keep_flags(seed, 0.5, B).any()
    x, _, dy, _, gamma, beta, mean, rstd = inputs(B, N, D)
    poison = torch.full_like(x, float("nan"))
    s, y, mean_s, rstd_s = ops.add_layernorm_path_fwd(poison, x, gamma, beta, B, 0.5, seed)
    y0, mean0, rstd0 = ops.layernorm_fwd(x, gamma, beta)
    dx, dg, db, dxd, dcol = ops.layernorm_bwd_path(dy, x, mean, rstd, gamma, N, 0.5, seed, drop_p=0.1, drop_seed=5, want_colsum=True)
    torch.cuda.synchronize()
    figures = (int((bits(s) != bits(x)).sum()), int((bits(dxd) != 0).sum()), float(dcol.abs().max()))
    print((B, N, D), "s != x, dx_drop != 0, max |dcol|:", figures)
    assert figures == (0, 0, 0.0)
    assert bool(torch.isfinite(y.float()).all()) and torch.allclose(mean_s, mean0, atol=1e-5, rtol=0) and torch.allclose(rstd_s, rstd0, atol=0, rtol=1e-5)
    dx0, dg0, db0 = ops.layernorm_bwd(dy, x, mean, rstd, gamma)
    assert torch.equal(bits(dx), bits(dx0)) and torch.equal(dg, dg0) and torch.equal(db, db0)


# ---- 11. the encoder layer ----------------------------------------------------------------------------------------------------
def _layer_params(B, N, D, H, Fd):
    g = torch.Generator(device="cuda").manual_seed(5)
    r = lambda *s, sc=1.0: (torch.randn(*s, device="cuda", generator=g) * sc)     # noqa: E731
    bf = lambda t: t.to(BF16)                                                       # noqa: E731
    x = bf(r(B, N, D))
    P = dict(in_w=bf(r(3 * D, D, sc=D ** -0.5)), in_b=bf(r(3 * D, sc=0.1)), out_w=bf(r(D, D, sc=D ** -0.5)),
             out_b=bf(r(D, sc=0.1)), n1_w=bf(1 + r(D, sc=0.1)), n1_b=bf(r(D, sc=0.1)),
             w1=bf(r(Fd, D, sc=D ** -0.5)), b1=bf(r(Fd, sc=0.1)), w2=bf(r(D, Fd, sc=Fd ** -0.5)), b2=bf(r(D, sc=0.1)),
             n2_w=bf(1 + r(D, sc=0.1)), n2_b=bf(r(D, sc=0.1)))
    return x, P, bf(r(B, N, D))


ORDER = ["in_w", "in_b", "out_w", "out_b", "n1_w", "n1_b", "w1", "b1", "w2", "b2", "n2_w", "n2_b"]


@pytest.mark.parametrize("masked", [False, True], ids=["full", "curve_window"])
def test_encoder_layer_against_the_masked_reference(ops, masked):
    """(B, N, D, H, F) = (5, 68, 128, 2, 256), dropout 0.1, drop_path 0.5 with fixed seeds, against fp32 torch autograd with the
    same masks and flags at the bars of the training-mode layer test; the branch stores, s1, s2, LN1 and LN2 at the store-point
    bar against fp32 math on the HIP path's own inputs to each store."""
    import sfcvit.functional as F
    from sfcvit import masks
    from test_dropout_gpu import close
    from test_parity_gpu import _store_point
    B, N, D, H, Fd, p, rate = 5, 68, 128, 2, 256, 0.1, 0.5
    seeds, pseeds = (11, 22, 33, 44), (66, 1234)
    k1, k2 = keep_flags(pseeds[0], rate, B), keep_flags(pseeds[1], rate, B)
    assert 0 < k1.sum() < B and 0 < k2.sum() < B and not np.array_equal(k1, k2)
    x, P, dy = _layer_params(B, N, D, H, Fd)
    window = masks.curve_window(N, 8) if masked else None
    am = ops.as_attention_mask(window, N) if masked else None
    leaves = [x.clone().requires_grad_(True)] + [P[k].clone().requires_grad_(True) for k in ORDER]
    ops.KERNEL_LOG = []
    try:
        y = F._EncoderLayer.apply(*leaves, None, F._LayerCfg(H, 1e-5, p, seeds, None, "relu", am, (rate, pseeds)))
        kept = [t.detach() for t in y.grad_fn.saved_tensors[:10]]
        y.backward(dy)
        ran = list(ops.KERNEL_LOG)
    finally:
        ops.KERNEL_LOG = None
    assert ran.count("add_ln_path_kernel<1>") == 2 and ran.count("ln_bwd_path_kernel<1, false>") == 2, ran
    assert masked == any("masked" in k for k in ran)

    M = B * N
    ma = ops.dropout_mask(B * H * N, N, p, seeds[0]).float().view(B, H, N, N)
    m1 = ops.dropout_mask(M, D, p, seeds[1]).float().view(B, N, D)
    mf = ops.dropout_mask(M, Fd, p, seeds[2]).float().view(B, N, Fd)
    m2 = ops.dropout_mask(M, D, p, seeds[3]).float().view(B, N, D)
    c1, c2 = (torch.from_numpy(k).cuda().float() / (1 - rate) for k in (k1, k2))
    xr = x.float().requires_grad_(True)
    R = {k: v.float().requires_grad_(True) for k, v in P.items()}
    yr = ref_layer(xr, R, H, (ma, m1, mf, m2), c1, c2, attn_mask=window.cuda() if masked else None)
    yr.backward(dy.float())
    print(f"flags {k1.astype(int).tolist()} {k2.astype(int).tolist()}: y max err {float((y.float() - yr.detach()).abs().max()):.3e}")
    close(y, yr.detach(), rel=1 / 32, abs_scale=1 / 24)
    for name, got, ref in zip(["x"] + ORDER, leaves, [xr] + [R[k] for k in ORDER]):
        gg, rr = got.grad.float().flatten(), ref.grad.flatten()
        cos, ratio = float(torch.dot(gg, rr) / (gg.norm() * rr.norm() + 1e-30)), float(gg.norm() / rr.norm())
        print(f"    d{name}: cosine {cos:.5f}, norm ratio {ratio:.4f}")
        assert cos > 0.99, (name, cos)
        assert abs(ratio - 1) < 5e-2, (name, ratio)

    # the new stores, each against fp32 math on the HIP path's own inputs to it
    rb = lambda t: t.to(BF16).float()                                              # noqa: E731
    cpu = lambda t: t.detach().float().cpu()                                       # noqa: E731
    x2, _, o_s, _, s1_s, _, _, x1_s, h_s, s2_s = kept
    W = {k: cpu(v) for k, v in P.items()}
    ks = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)))
    keep = lambda m: (cpu(m) > 0).float() * ks                                     # noqa: E731
    a_s = ops.gemm(o_s.view(M, D), P["out_w"], bias=P["out_b"], dropout_p=p, dropout_seed=seeds[1])       # the branch stores, again
    f_s = ops.gemm(h_s, P["w2"], bias=P["b2"], dropout_p=p, dropout_seed=seeds[3])
    rep = []
    _store_point("out_proj, dropout1", a_s, rb((cpu(o_s).view(M, D) @ W["out_w"].t() + W["out_b"]) * keep(m1).view(M, D)), rep, 1e-3)
    _store_point("linear2, dropout2", f_s, rb((cpu(h_s) @ W["w2"].t() + W["b2"]) * keep(m2).view(M, D)), rep, 1e-3)
    r1, r2 = (cpu(c).repeat_interleave(N)[:, None] for c in (c1, c2))
    _store_point("s1 = x + c1 a", s1_s, rb(cpu(x2) + r1 * cpu(a_s)), rep, 1e-3)
    _store_point("s2 = x1 + c2 f", s2_s, rb(cpu(x1_s) + r2 * cpu(f_s)), rep, 1e-3)
    ln = lambda t, w_, b_: torch.nn.functional.layer_norm(t, (D,), w_, b_, 1e-5)    # noqa: E731
    _store_point("LN1", x1_s, rb(ln(cpu(s1_s), W["n1_w"], W["n1_b"])), rep, 1e-3)
    _store_point("LN2", y.view(M, D), rb(ln(cpu(s2_s), W["n2_w"], W["n2_b"])), rep, 1e-3)
    print("[drop-path store points] " + ", ".join(f"{t} {f:.1e}" for t, f, _ in rep))
    d1, d2 = (torch.from_numpy(np.repeat(~k, N)) for k in (k1, k2))
    assert torch.equal(bits(s1_s.cpu()[d1]), bits(x2.cpu()[d1])) and torch.equal(bits(s2_s.cpu()[d2]), bits(x1_s.cpu()[d2]))


def test_drop_path_zero_is_the_call_without_the_keyword(ops):
    import sfcvit.functional as F
    x, P, _ = _layer_params(5, 68, 128, 2, 256)
    args = [x] + [P[k] for k in ORDER]
    runs = []
    for kw in ({}, {"drop_path": 0.0}):
        torch.manual_seed(3)
        ops.KERNEL_LOG = []
        try:
            y = F.encoder_layer(*[t.clone().requires_grad_(True) for t in args], 2, dropout_p=0.1, **kw)
            runs.append((y.detach(), [t.detach() for t in y.grad_fn.saved_tensors], list(ops.KERNEL_LOG)))
        finally:
            ops.KERNEL_LOG = None
    (y0, saved0, log0), (y1, saved1, log1) = runs
    print(len(saved0), "saved tensors;", len(log0), "logged launches")
    assert log0 == log1 and not any("path" in k for k in log1)
    assert torch.equal(bits(y0), bits(y1)) and len(saved0) == len(saved1)
    assert all(torch.equal(u, v) for u, v in zip(saved0, saved1))


# ---- 12. models ---------------------------------------------------------------------------------------------------------------
def _tiny_model(rate, dropout=0.0, seed=11, name="hilbert32_1d"):
    cfg, batch = MODEL_CASES[name]
    torch.manual_seed(seed)
    model = build_with(cfg, dropout_p=dropout, head_dropout_p=dropout, drop_path_rate=rate)
    x = formula.image_batch(batch, 3, cfg.img_size, cfg.img_size).cuda()
    tgt = formula.soft_targets(batch, cfg.num_classes).cuda()
    return model.to("cuda", dtype=BF16), x, tgt


def test_model_eval_bits_and_training_gradients(ops):
    import sfcvit.functional as F
    plain, x, tgt = _tiny_model(0.0, dropout=0.1)
    model, _, _ = _tiny_model(0.1, dropout=0.1)
    model.load_state_dict(plain.state_dict())
    plain.eval()
    model.eval()
    with torch.no_grad():
        assert torch.equal(bits(model(x)), bits(plain(x)))
    model.train()
    depth = len(model.encoder.transformer.layers)
    ops.KERNEL_LOG = []
    try:
        torch.manual_seed(5)
        logits = model(x)
        fwd = [k for k in ops.KERNEL_LOG if "path" in k]
        F.soft_target_cross_entropy(logits, tgt).backward()
        log = [k for k in ops.KERNEL_LOG if "path" in k]
    finally:
        ops.KERNEL_LOG = None
    print(model.encoder.drop_path_rates, log)
    # layer 0 has rate 0 and runs the launches of a model without the feature; every later layer runs the two sites' kernels
    assert model.encoder.drop_path_rates[0] == 0.0 and depth >= 2
    assert fwd == ["add_ln_path_kernel<1>"] * (2 * (depth - 1)) and log[len(fwd):] == ["ln_bwd_path_kernel<1, false>"] * (2 * (depth - 1))
    for k, prm in model.named_parameters():
        if not k.startswith("mlp_mixer.token_mix"):
            assert prm.grad is not None and torch.isfinite(prm.grad.float()).all(), k
    # the first layer alone logs nothing of the feature, the last one does
    enc = model.encoder
    h = torch.randn(x.shape[0], enc.max_len, 128, device="cuda", dtype=BF16)
    for idx, expect in ((0, 0), (depth - 1, 2)):
        one = type(enc)(128, enc.max_len, enc.n_head, 256, None, dropout_p=0.1, n_layers=1, drop_path_rate=enc.drop_path_rates[idx]).to("cuda", dtype=BF16)
        one.train()
        ops.KERNEL_LOG = []
        try:
            one(h)
            assert sum("path" in k for k in ops.KERNEL_LOG) == expect, (idx, ops.KERNEL_LOG)
        finally:
            ops.KERNEL_LOG = None


def test_graphed_step_draws_new_flags_every_replay():
    """Dropout 0, rate 0.5, learning rate 0: the parameters stand still, so four replays on one batch differ only by the flags the
    device seed offset gives them."""
    from sfcvit import ops
    from sfcvit.training import FusedAdamW, GraphedTrainStep
    try:
        model, x, tgt = _tiny_model(0.5)
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
            "--warmup-epochs", "0", "--epochs", "1", "--drop-path", "0.1", "--checkpoint-dir", str(tmp_path), *extra]


@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
def test_main_py_trains_with_drop_path(tmp_path, graph):
    out = subprocess.run(_main_py(tmp_path, *(["--graph"] if graph else [])), capture_output=True, text=True, timeout=300)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stderr[-3000:]
    assert "Epoch 1/1" in out.stdout, out.stdout[-1000:]
    sd = torch.load(os.path.join(str(tmp_path), "checkpoint_hilbert.pt"), map_location="cpu", weights_only=True)["model_state_dict"]
    assert not any("drop" in k for k in sd)


def test_torch_compile_refuses_training_and_runs_eval():
    import sfcvit.library  # noqa: F401  (registers the ops)
    model, x, _ = _tiny_model(0.1)
    try:
        model.eval()
        with torch.no_grad():
            want = model(x)
            got = torch.compile(model)(x)
        assert torch.equal(bits(got), bits(want))
        torch._dynamo.reset()
        model.train()
        with pytest.raises(NotImplementedError, match="drop_path > 0 has no traced form"):
            torch.compile(model)(x)
    finally:
        torch._dynamo.reset()
