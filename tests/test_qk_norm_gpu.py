"""The QK-norm kernels on the GPU: exact answers on Walsh rows, fp64-referenced general inputs at the store-point bar, padding,
the untouched v third, determinism, and F.qk_norm under autograd.  Shapes (B, N, H, hd) are the smallest at which the geometry
can go wrong: a full 8-slot group, 6 of 8 slots, three groups with an odd N, padded head dims that are no multiple of 8, every
kernel head dim, and a row count read from the plan that is no multiple of a workgroup's rows and more than twice that."""
import pytest
import torch

import qk_norm_ref
from test_qk_norm_cpu import SHAPES, _hp

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPS = 1e-6


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int16)


def plan_shape(ops):
    """(B, N, H, hd) with M = B * N no multiple of the plan's rows per workgroup and more than twice that number."""
    rows = ops.qk_norm_plan(1, 4, 64)["rows_per_wg"]
    N = 2 * rows + 7
    assert N % rows and N > 2 * rows
    return (1, N, 4, 64)


def all_shapes(ops):
    return SHAPES + [plan_shape(ops)]


def pack(x, v, H, hd, hp):
    """x [M, 2 H, hd] (q slots then k slots), v [M, H, hd] -> packed padded qkv [M, 3 H hp] bf16 on the GPU."""
    M = x.shape[0]
    t = torch.zeros(M, 3, H, hp)
    t[:, :2, :, :hd] = x.reshape(M, 2, H, hd)
    t[:, 2, :, :hd] = v
    return t.reshape(M, 3 * H * hp).to("cuda", dtype=BF16)


def general(B, N, H, hd, seed=0):
    """randn, offset and scaled per head slot so that the means are not near zero -> (qkv, params, dy) on the GPU."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + N + 31 * H + hd)
    M, hp = B * N, _hp(hd)
    slots = torch.arange(2 * H).float()
    x = torch.randn(M, 2 * H, hd, generator=g) * (0.5 + 0.25 * slots)[None, :, None] + (slots - H)[None, :, None] * 0.7
    v = torch.randn(M, H, hd, generator=g)
    P = torch.stack([1 + 0.3 * torch.randn(hd, generator=g), 0.3 * torch.randn(hd, generator=g),
                     1 + 0.3 * torch.randn(hd, generator=g), 0.3 * torch.randn(hd, generator=g)]).to("cuda", dtype=BF16)
    dy = torch.zeros(M, 3, H, hp)
    dy[..., :hd] = torch.randn(M, 3, H, hd, generator=g)
    return pack(x, v, H, hd, hp), P, dy.reshape(M, 3 * H * hp).to("cuda", dtype=BF16)


# ---- (1) forward, exact answer -------------------------------------------------------------------------------------------------
def test_forward_exact_answer(ops):
    ran = 0
    for B, N, H, hd in all_shapes(ops):
        if hd not in (64, 128, 256):
            continue
        M = B * N
        x, _, _, _, sx, _, gamma, beta = qk_norm_ref.exact_inputs(M, H, hd)
        v = torch.randn(M, H, hd, generator=torch.Generator().manual_seed(M))
        qkv = pack(x, v, H, hd, hd)
        before = qkv.clone()
        P = torch.stack([gamma, beta, -gamma, beta + 0.25]).to("cuda", dtype=BF16)
        assert torch.equal(P.float().cpu(), torch.stack([gamma, beta, -gamma, beta + 0.25]))
        raw = ops.qk_norm_fwd(qkv, P, H, hd, EPS)
        torch.cuda.synchronize()
        assert ops.last_rowwise_kernel() == f"qk_norm_fwd_kernel<{hd}>"
        want = torch.cat([(gamma * sx[:, :H] + beta), (-gamma * sx[:, H:] + beta + 0.25)], 1).reshape(M, 2 * H * hd).to(BF16)
        assert bool((want != 0).all())
        got = qkv[:, :2 * H * hd].cpu()
        diff = int((bits(got) != bits(want)).sum())
        print(f"{(B, N, H, hd)}: {diff} of {got.numel()} elements differ from gamma * sign + beta")
        assert diff == 0
        assert torch.equal(bits(raw), bits(before[:, :2 * H * hd])), "raw is not the original q | k"
        assert torch.equal(bits(qkv[:, 2 * H * hd:]), bits(before[:, 2 * H * hd:])), "v was touched"
        ran += 1
    assert ran >= 6


# ---- (2) forward, general inputs -----------------------------------------------------------------------------------------------
def _forward_general(ops, B, N, H, hd, eps=EPS):
    from test_parity_gpu import _store_point
    hp, M = _hp(hd), B * N
    qkv, P, _ = general(B, N, H, hd)
    before = qkv.clone()
    raw = ops.qk_norm_fwd(qkv, P, H, hd, eps)
    torch.cuda.synchronize()
    ref = qk_norm_ref.forward64(before, P, H, hd, hp, eps)
    rep = []
    got = qk_norm_ref.heads(qkv, H, hp, 3)
    _store_point("q | k", got[:, :2, :, :hd], ref[:, :2, :, :hd].float().to(BF16).float().cpu(), rep, 1e-3)
    print(f"{(B, N, H, hd)} eps {eps}: " + ", ".join(f"{t} {f:.1e} (worst {w:.2f})" for t, f, w in rep))
    assert torch.equal(bits(raw), bits(before[:, :2 * H * hp]))
    assert torch.equal(bits(got[:, 2]), bits(qk_norm_ref.heads(before, H, hp, 3)[:, 2])), "v was touched"
    if hp > hd:
        assert int((bits(got[:, :2, :, hd:]) != 0).sum()) == 0, "padded columns are not +0"
    return before, raw, qkv, P


def test_forward_general(ops):
    for shape in all_shapes(ops):
        _forward_general(ops, *shape)
    _forward_general(ops, 2, 5, 4, 48, eps=0.0)
    _forward_general(ops, 2, 5, 3, 64, eps=1e-5)
    _forward_general(ops, 1, 3, 1, 1, eps=1e-3)                # hd = 1: every output is the bias


def test_forward_padded_columns_hold_no_bias_and_stay_out_of_the_statistics(ops):
    """Garbage in the padded columns of the input changes nothing in the real ones and comes out +0."""
    B, N, H, hd = 2, 5, 4, 20
    hp = _hp(hd)
    qkv, P, _ = general(B, N, H, hd)
    dirty = qk_norm_ref.heads(qkv.clone(), H, hp, 3)
    dirty[:, :2, :, hd:] = 37.0
    dirty = dirty.reshape(B * N, 3 * H * hp).contiguous()
    ops.qk_norm_fwd(qkv, P, H, hd, EPS)
    ops.qk_norm_fwd(dirty, P, H, hd, EPS)
    torch.cuda.synchronize()
    assert torch.equal(bits(qkv), bits(dirty))


# ---- (3) backward, exact answer ------------------------------------------------------------------------------------------------
def test_backward_exact_answer(ops):
    for B, N, H, hd in all_shapes(ops):
        if hd not in (64, 128, 256):
            continue
        M = B * N
        x, gy, k, m, _, sg, gamma, beta = qk_norm_ref.exact_inputs(M, H, hd)
        P = torch.stack([gamma, beta, gamma, beta]).to("cuda", dtype=BF16)
        dy = gy / gamma
        v = torch.randn(M, H, hd, generator=torch.Generator().manual_seed(M + 1))
        raw = x.reshape(M, 2 * H * hd).to("cuda", dtype=BF16)
        dqkv = pack(dy, v, H, hd, hd)
        before = dqkv.clone()
        _, dP, cs = ops.qk_norm_bwd(dqkv, raw, P, H, hd, EPS, colsum=True)
        torch.cuda.synchronize()
        assert ops.last_rowwise_kernel() == f"qk_norm_bwd_kernel<{hd}>"
        want = (sg * torch.pow(2.0, (m - k).float())[..., None]).reshape(M, 2 * H * hd)
        got = dqkv[:, :2 * H * hd].float().cpu()
        diff = int((got != want).sum())
        assert torch.equal(bits(dqkv[:, 2 * H * hd:]), bits(before[:, 2 * H * hd:])), "v was touched"
        ref_dx, ref_dP, abs_g, abs_b = qk_norm_ref.backward64(before, raw, P, H, hd, hd, EPS)
        err_p = (dP.double() - ref_dP).abs().cpu()
        bound_p = 1e-5 * torch.stack([abs_g[0], abs_b[0], abs_g[1], abs_b[1]]).cpu()
        err_c = (cs.double().cpu() - want.double().sum(0)).abs()
        bound_c = 1e-5 * want.double().abs().sum(0)
        print(f"{(B, N, H, hd)}: {diff} of {got.numel()} dx differ; dP worst err/bound {float((err_p / bound_p).max()):.3f}, "
              f"colsum worst err/bound {float((err_c / bound_c).max()):.3f}")
        assert diff == 0
        assert bool((err_p <= bound_p).all()) and bool((err_c <= bound_c).all())


# ---- (4) backward, general inputs ----------------------------------------------------------------------------------------------
def _backward_general(ops, B, N, H, hd, eps=EPS):
    from test_dropout_gpu import close
    from test_parity_gpu import _store_point
    hp, M = _hp(hd), B * N
    Da = H * hp
    qkv, P, dy = general(B, N, H, hd)
    raw = ops.qk_norm_fwd(qkv, P, H, hd, eps)
    if hp > hd:                                                # the padded columns of the incoming gradient hold NaN
        t = qk_norm_ref.heads(dy, H, hp, 3)
        t[:, :2, :, hd:] = float("nan")
    before = dy.clone()
    ref_dx, ref_dP, _, _ = qk_norm_ref.backward64(torch.nan_to_num(before), raw, P, H, hd, hp, eps)
    dq, dP, cs = ops.qk_norm_bwd(dy, raw, P, H, hd, eps, colsum=True)
    torch.cuda.synchronize()
    assert dq is dy and dP.dtype == torch.float32 and cs.dtype == torch.float32 and tuple(dP.shape) == (4, hd) and cs.numel() == 2 * Da
    got = qk_norm_ref.heads(dy, H, hp, 3)
    rep = []
    _store_point("dq | dk", got[:, :2], ref_dx.float().to(BF16).float().cpu(), rep, 1e-3)
    assert torch.equal(bits(got[:, 2]), bits(qk_norm_ref.heads(before, H, hp, 3)[:, 2])), "v was touched"
    if hp > hd:
        assert int((bits(got[:, :2, :, hd:]) != 0).sum()) == 0, "padded columns of dq | dk are not +0"
    cs64 = dy[:, :2 * Da].double().sum(0)
    close(dP, ref_dP, rel=5e-3, abs_scale=5e-3)
    close(cs, cs64, rel=5e-3, abs_scale=5e-3)
    print(f"{(B, N, H, hd)} eps {eps}: " + ", ".join(f"{t} {f:.1e} (worst {w:.2f})" for t, f, w in rep)
          + f"; dP max err {float((dP.double() - ref_dP).abs().max()):.2e}, colsum max err {float((cs.double() - cs64).abs().max()):.2e}")
    # the bf16 grad_out / colsum form, with the v sums carried over
    again = before.clone()
    go = torch.full((4, hd), float("nan"), device="cuda", dtype=BF16)
    slot = torch.full((3 * Da,), float("nan"), device="cuda", dtype=BF16)
    vs = torch.randn(Da, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    _, dP2, cs2 = ops.qk_norm_bwd(again, raw, P, H, hd, eps, colsum=slot, grad_out=go, vsum=vs)
    torch.cuda.synchronize()
    assert dP2 is go and cs2 is slot and torch.equal(bits(again), bits(dy))
    close(go, ref_dP, rel=5e-3, abs_scale=5e-3)
    close(slot[:2 * Da], cs64, rel=5e-3, abs_scale=5e-3)
    assert torch.equal(slot[:2 * Da], cs.to(BF16)) and torch.equal(go, dP.to(BF16)) and torch.equal(slot[2 * Da:], vs.to(BF16))
    return before, raw, P, dy, dP, cs


def test_backward_general(ops):
    for shape in all_shapes(ops):
        _backward_general(ops, *shape)
    _backward_general(ops, 2, 5, 4, 48, eps=1e-5)


# ---- (5) determinism -----------------------------------------------------------------------------------------------------------
def test_backward_is_deterministic(ops):
    for B, N, H, hd in ((2, 197, 12, 64), (2, 5, 4, 20), plan_shape(ops)):
        hp = _hp(hd)
        qkv, P, dy = general(B, N, H, hd, seed=2)
        raw = ops.qk_norm_fwd(qkv, P, H, hd, EPS)
        runs = []
        for _ in range(2):
            d = dy.clone()
            _, dP, cs = ops.qk_norm_bwd(d, raw, P, H, hd, EPS, colsum=True)
            torch.cuda.synchronize()
            runs.append((bits(d[:, :2 * H * hp]), dP.view(torch.int32), cs.view(torch.int32)))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), (B, N, H, hd)


# ---- (6) F.qk_norm under autograd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,H,hd", [(2, 5, 3, 64), (2, 5, 4, 20), (1, 7, 2, 96)])
def test_functional_qk_norm(ops, B, N, H, hd):
    import sfcvit.functional as F
    hp = _hp(hd)
    qkv, P, dy = general(B, N, H, hd)
    x = qkv.view(B, N, -1).clone().requires_grad_(True)
    keep = x.detach().clone()
    Pl = P.clone().requires_grad_(True)
    y = F.qk_norm(x, H, Pl, EPS, head_dim=hd)
    y.backward(dy.view(B, N, -1))
    torch.cuda.synchronize()
    assert torch.equal(bits(x.detach()), bits(keep)), "the input was modified"
    k_in, k_dy = qkv.clone(), dy.clone()
    raw = ops.qk_norm_fwd(k_in, P, H, hd, EPS)
    _, dP, _ = ops.qk_norm_bwd(k_dy, raw, P, H, hd, EPS)
    torch.cuda.synchronize()
    assert torch.equal(bits(y.detach().view(B * N, -1)), bits(k_in))
    assert torch.equal(bits(x.grad.view(B * N, -1)), bits(k_dy)) and torch.equal(Pl.grad, dP.to(BF16))
    assert tuple(Pl.grad.shape) == (4, hd) and y.shape == x.shape and hp * 3 * H == x.shape[-1]
