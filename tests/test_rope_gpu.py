"""The RoPE kernels on the GPU: exact answers (integers through maps that are no rotations) bit for bit with their exact column sums,
fp64-referenced general inputs at the store-point bar, column sums against the fp64 sum of the stored values, padding, the
untouched v third, determinism, the no-sums form, and F.rope under autograd.  Shapes (B, N, H, hd) are the smallest at which the
geometry can go wrong (test_rope_cpu.SHAPES), plus a row count read from the plan that is no multiple of a workgroup's rows and
more than twice that."""
import pytest
import torch

import rope_ref
from test_rope_cpu import SHAPES, STORE_CAP, _hp, general as general_cpu

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int16)


def plan_shape(ops):
    """(B, N, H, hd): a workgroup holds tokens_per_wg tokens of batch_per_wg images; B and N are no multiples of those, and M = B * N
    is no multiple of a workgroup's rows and more than twice that number."""
    plan = ops.rope_plan(1, 1, 4, 64)
    B, N = plan["batch_per_wg"] + 3, 2 * plan["tokens_per_wg"] + 1
    rows = plan["rows_per_wg"]
    assert (B * N) % rows and B * N > 2 * rows and B % plan["batch_per_wg"] and N % plan["tokens_per_wg"]
    return (B, N, 4, 64)


def all_shapes(ops):
    return SHAPES + [plan_shape(ops)]


def pack(x, v, H, hd, hp):
    """x [M, 2 H, hd] (q slots then k slots), v [M, H, hd] -> packed padded qkv [M, 3 H hp] bf16 on the GPU."""
    M = x.shape[0]
    t = torch.zeros(M, 3, H, hp)
    t[:, :2, :, :hd] = x.reshape(M, 2, H, hd)
    t[:, 2, :, :hd] = v
    return t.reshape(M, 3 * H * hp).to("cuda", dtype=BF16)


def general(ops, B, N, H, hd, seed=0):
    qkv, table, dy = general_cpu(B, N, H, hd, seed)
    return qkv.cuda(), ops.RopeTable(table), dy.cuda()


# ---- (1) exact answers, both directions, with the exact column sums --------------------------------------------------------------
def test_exact_answers(ops):
    ran = 0
    for B, N, H, hd in all_shapes(ops):
        if _hp(hd) != hd:
            continue
        M, Da = B * N, H * hd
        x, dy, table = rope_ref.exact_inputs(B, N, H, hd)
        want_y, want_dx = rope_ref.exact_answers(x, dy, table)
        rt = ops.RopeTable(table)
        v = torch.randn(M, H, hd, generator=torch.Generator().manual_seed(M))
        qkv = pack(x, v, H, hd, hd)
        before = qkv.clone()
        assert ops.rope_fwd(qkv, rt, H) is qkv
        torch.cuda.synchronize()
        assert ops.last_rowwise_kernel() == f"rope_fwd_kernel<{hd}>"
        d_fwd = int((bits(qkv[:, :2 * Da].cpu()) != bits(want_y.reshape(M, 2 * Da).to(BF16))).sum())
        assert torch.equal(bits(qkv[:, 2 * Da:]), bits(before[:, 2 * Da:])), "v was touched"
        dqkv = pack(dy, v, H, hd, hd)
        before = dqkv.clone()
        _, cs = ops.rope_bwd(dqkv, rt, H, colsum=True)
        torch.cuda.synchronize()
        assert ops.last_rowwise_kernel() == f"rope_bwd_kernel<{hd}>"
        d_bwd = int((bits(dqkv[:, :2 * Da].cpu()) != bits(want_dx.reshape(M, 2 * Da).to(BF16))).sum())
        assert torch.equal(bits(dqkv[:, 2 * Da:]), bits(before[:, 2 * Da:])), "v was touched"
        sums = want_dx.reshape(M, 2 * Da).double().sum(0)
        assert torch.equal(sums.float().double(), sums)        # exact in fp32
        d_cs = int((cs.cpu() != sums.float()).sum())
        # the bf16 form, with the v sums carried over: the bf16 rounding of the exact sum
        again = before.clone()
        slot = torch.full((3 * Da,), float("nan"), device="cuda", dtype=BF16)
        vs = torch.randn(Da, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        _, cs2 = ops.rope_bwd(again, rt, H, colsum=slot, vsum=vs)
        torch.cuda.synchronize()
        d_cs16 = int((bits(slot[:2 * Da].cpu()) != bits(sums.float().to(BF16))).sum())
        print(f"{(B, N, H, hd)}: forward {d_fwd}, backward {d_bwd} of {M * 2 * Da} elements differ from the exact answer; "
              f"{d_cs} fp32 and {d_cs16} bf16 column sums of {2 * Da} differ from the exact sum")
        assert d_fwd == 0 and d_bwd == 0 and d_cs == 0 and d_cs16 == 0
        assert cs2 is slot and torch.equal(bits(again), bits(dqkv)) and torch.equal(bits(slot[2 * Da:]), bits(vs.to(BF16)))
        assert cs.dtype == torch.float32 and cs.numel() == 2 * Da
        ran += 1
    assert ran >= 10


# ---- (2) general inputs ------------------------------------------------------------------------------------------------------------
def _forward_general(ops, B, N, H, hd):
    from test_parity_gpu import _store_point
    hp, M = _hp(hd), B * N
    qkv, rt, _ = general(ops, B, N, H, hd)
    before = qkv.clone()
    ops.rope_fwd(qkv, rt, H)
    torch.cuda.synchronize()
    ref = rope_ref.forward64(before, rt.on("cuda"), H, hd, hp)
    rep = []
    got = rope_ref.heads(qkv, H, hp, 3)
    _store_point("q | k", got[:, :2, :, :hd], ref[:, :2, :, :hd].float().to(BF16).float().cpu(), rep, STORE_CAP)
    print(f"{(B, N, H, hd)} forward: " + ", ".join(f"{t} {f:.1e} (worst {w:.2f})" for t, f, w in rep))
    assert torch.equal(bits(got[:, 2]), bits(rope_ref.heads(before, H, hp, 3)[:, 2])), "v was touched"
    if hp > hd:
        assert int((bits(got[:, :2, :, hd:]) != 0).sum()) == 0, "padded columns are not +0"


def test_forward_general(ops):
    for shape in all_shapes(ops):
        _forward_general(ops, *shape)


def test_forward_garbage_in_the_padding_changes_nothing(ops):
    """Garbage, NaN included, in the padded columns of the input changes nothing in the real ones and comes out +0."""
    for B, N, H, hd in ((2, 5, 4, 20), (2, 5, 4, 48), (1, 7, 2, 96), (1, 3, 1, 2)):
        hp = _hp(hd)
        qkv, rt, _ = general(ops, B, N, H, hd)
        dirty = rope_ref.heads(qkv.clone(), H, hp, 3)
        dirty[:, :2, :, hd:] = 37.0
        dirty[:, 0, :, hd] = float("nan")
        dirty = dirty.reshape(B * N, 3 * H * hp).contiguous()
        ops.rope_fwd(qkv, rt, H)
        ops.rope_fwd(dirty, rt, H)
        torch.cuda.synchronize()
        assert torch.equal(bits(qkv), bits(dirty)), (B, N, H, hd)


def _sum_bound(stored, M, bf16_out):
    """|sum in any fixed order - exact sum| <= M * 2^-24 * sum |addends| (M - 1 fp32 additions, each within 2^-24 of a partial sum
    that is at most sum |addends|), plus one bf16 rounding, 2^-8 relative, when the output is bf16."""
    abs_sum = stored.double().abs().sum(0)
    bound = M * 2.0 ** -24 * abs_sum
    return bound + 2.0 ** -8 * (stored.double().sum(0).abs() + bound) if bf16_out else bound


def _backward_general(ops, B, N, H, hd):
    from test_parity_gpu import _store_point
    hp, M = _hp(hd), B * N
    Da = H * hp
    _, rt, dy = general(ops, B, N, H, hd)
    if hp > hd:                                                # the padded columns of the incoming gradient hold NaN
        t = rope_ref.heads(dy, H, hp, 3)
        t[:, :2, :, hd:] = float("nan")
    before = dy.clone()
    ref_dx = rope_ref.backward64(torch.nan_to_num(before), rt.on("cuda"), H, hd, hp)
    dq, cs = ops.rope_bwd(dy, rt, H, colsum=True)
    torch.cuda.synchronize()
    assert dq is dy and cs.dtype == torch.float32 and cs.numel() == 2 * Da
    got = rope_ref.heads(dy, H, hp, 3)
    rep = []
    _store_point("dq | dk", got[:, :2], ref_dx.float().to(BF16).float().cpu(), rep, STORE_CAP)
    assert torch.equal(bits(got[:, 2]), bits(rope_ref.heads(before, H, hp, 3)[:, 2])), "v was touched"
    if hp > hd:
        assert int((bits(got[:, :2, :, hd:]) != 0).sum()) == 0, "padded columns of dq | dk are not +0"
    stored = dy[:, :2 * Da]
    cs64 = stored.double().sum(0)
    err, bound = (cs.double() - cs64).abs(), _sum_bound(stored, M, False)
    assert bool((err <= bound).all()), float((err - bound).max())
    # the bf16 colsum form, with the v sums carried over
    again = before.clone()
    slot = torch.full((3 * Da,), float("nan"), device="cuda", dtype=BF16)
    vs = torch.randn(Da, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    _, cs2 = ops.rope_bwd(again, rt, H, colsum=slot, vsum=vs)
    # and the no-sums form: one launch, the same dq | dk bits
    plain = before.clone()
    ops.KERNEL_LOG = []
    try:
        _, none = ops.rope_bwd(plain, rt, H)
        log = list(ops.KERNEL_LOG)
    finally:
        ops.KERNEL_LOG = None
    torch.cuda.synchronize()
    assert none is None and log == [f"rope_bwd_kernel<{hp}>"]
    assert cs2 is slot and torch.equal(bits(again), bits(dy)) and torch.equal(bits(plain), bits(dy))
    err16, bound16 = (slot[:2 * Da].double() - cs64).abs(), _sum_bound(stored, M, True)
    assert bool((err16 <= bound16).all()), float((err16 - bound16).max())
    assert torch.equal(bits(slot[:2 * Da]), bits(cs.to(BF16))) and torch.equal(bits(slot[2 * Da:]), bits(vs.to(BF16)))
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{(B, N, H, hd)} backward: " + ", ".join(f"{t} {f:.1e} (worst {w:.2f})" for t, f, w in rep)
          + f"; colsum worst err/bound {worst:.3f} (fp32), {float((err16 / bound16.clamp_min(1e-300)).max()):.3f} (bf16)")


def test_backward_general(ops):
    for shape in all_shapes(ops):
        _backward_general(ops, *shape)


# ---- (3) determinism ---------------------------------------------------------------------------------------------------------------
def test_backward_is_deterministic(ops):
    for B, N, H, hd in ((2, 197, 12, 64), (67, 3, 1, 64), (2, 5, 4, 20), plan_shape(ops)):
        hp = _hp(hd)
        _, rt, dy = general(ops, B, N, H, hd, seed=2)
        runs = []
        for _ in range(2):
            d = dy.clone()
            _, cs = ops.rope_bwd(d, rt, H, colsum=True)
            torch.cuda.synchronize()
            runs.append((bits(d), cs.view(torch.int32)))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), (B, N, H, hd)


# ---- (4) F.rope under autograd -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,H,hd", [(2, 5, 3, 64), (2, 5, 4, 20), (1, 7, 2, 96)])
def test_functional_rope(ops, B, N, H, hd):
    import sfcvit.functional as F
    from test_parity_gpu import _store_point
    hp = _hp(hd)
    qkv, rt, dy = general(ops, B, N, H, hd)
    x = qkv.view(B, N, -1).clone().requires_grad_(True)
    keep = x.detach().clone()
    y = F.rope(x, rt, H)
    y.backward(dy.view(B, N, -1))
    torch.cuda.synchronize()
    assert torch.equal(bits(x.detach()), bits(keep)), "the input was modified"
    assert y.shape == x.shape and x.grad.shape == x.shape and hp * 3 * H == x.shape[-1]
    rep = []
    ref_y = rope_ref.forward64(qkv, rt.on("cuda"), H, hd, hp)
    ref_dx = rope_ref.backward64(dy, rt.on("cuda"), H, hd, hp)
    _store_point("y", rope_ref.heads(y.detach().view(B * N, -1), H, hp, 3)[:, :2], ref_y[:, :2].float().to(BF16).float().cpu(), rep, STORE_CAP)
    _store_point("dx", rope_ref.heads(x.grad.view(B * N, -1), H, hp, 3)[:, :2], ref_dx.float().to(BF16).float().cpu(), rep, STORE_CAP)
    # v passes through in both directions
    assert torch.equal(bits(y.detach()[..., 2 * H * hp:]), bits(keep[..., 2 * H * hp:]))
    assert torch.equal(bits(x.grad[..., 2 * H * hp:]), bits(dy.view(B, N, -1)[..., 2 * H * hp:]))
    # a CPU table is taken too, and gives the same bits
    y2 = F.rope(keep, rt.table, H)
    assert torch.equal(bits(y2), bits(y.detach()))
