"""Qualifies tests/rowwise_ref.py without a GPU: (1) the fp64 references agree with torch double autograd to 1e-12; (2) an fp32
restatement of every kernel formula (numpy float32, sums in the kernels' lane / butterfly / partial-row order) passes every bar
at every input family of tests/test_rowwise_edges_gpu.py, worst ratio printed; (3) every bar has teeth: each fp32 mutant fails
at least one bar at those inputs; (4) the launch geometry rowwise_ref restates is the library's."""
import numpy as np
import pytest
import torch

import rowwise_ref as R

F = np.float32


def f32(t):
    return t.detach().cpu().to(torch.float32).numpy()


# ---- fp32 restatements (csrc/layernorm.hip, rowwise.hip), with their mutants -------------------------------------------------
def lane_sum(v, skip_vec=None):
    """Row sums of v [M, D] as a wave forms them: lane l adds its 8-column vectors l, l + 64, ... in turn, then the xor butterfly."""
    M, D = v.shape
    vpl = -(-(D // 8) // 64)
    pad = np.zeros((M, vpl * 512), F)
    pad[:, :D] = v
    if skip_vec is not None:
        pad[:, 8 * skip_vec:8 * skip_vec + 8] = 0
    a = pad.reshape(M, vpl, 64, 8)
    s = np.zeros((M, 64), F)
    for i in range(vpl):
        for j in range(8):
            s = s + a[:, i, :, j]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return s[:, 0]


def reduce16(part):
    """reduce_partials16: thread row g adds partial rows g, g + 64, ...; 4 thread rows add 16 of those each; (a + b) + (c + d)."""
    nb, n = part.shape
    k = -(-nb // 64)
    pad = np.zeros((k * 64, n), F)
    pad[:nb] = part
    pad = pad.reshape(k, 64, n)
    r = np.zeros((64, n), F)
    for i in range(k):
        r = r + pad[i]
    r = r.reshape(4, 16, n)
    t = np.zeros((4, n), F)
    for i in range(16):
        t = t + r[:, i]
    return (t[0] + t[1]) + (t[2] + t[3])


def rows_sum(terms, blocks, drop_row=None):
    """Column sums of terms [M, n] as ln_bwd_* forms them: wave w of block b adds rows 4 b + w, + 4 blocks, ...; the block adds its
    4 waves; reduce16 adds the blocks."""
    M, n = terms.shape
    stride = 4 * blocks
    k = -(-M // stride)
    pad = np.zeros((k * stride, n), F)
    pad[:M] = terms
    if drop_row is not None:
        pad[drop_row] = 0
    pad = pad.reshape(k, blocks, 4, n)
    acc = np.zeros((blocks, 4, n), F)
    for i in range(k):
        acc = acc + pad[i]
    return reduce16(((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3])


def ln_fwd32(x, gamma, beta, eps=R.EPS, mutant=None):
    x, g, b = f32(x), f32(gamma), f32(beta)
    D = x.shape[1]
    skip = min(1, D // 8 - 1) if mutant == "skipvec" else None
    with np.errstate(all="ignore"):
        mu = lane_sum(x, skip) / F(D)
        d = x - mu[:, None]
        if mutant == "onepass":
            var = lane_sum(x * x) / F(D) - mu * mu
        else:
            var = lane_sum(d * d, skip) / F(D - 1 if mutant == "dm1" else D)
        rs = F(1) / np.sqrt(var + F(0 if mutant == "noeps" else eps), dtype=F)
        y = d * rs[:, None] * g + b
    return R.bf(torch.from_numpy(y)), mu, rs


def ln_bwd32(dy, x, mean, rstd, gamma, add, mutant=None):
    dy, x, g = f32(dy), f32(x), f32(gamma)
    mu, rs = f32(mean)[:, None], f32(rstd)[:, None]
    M, D = x.shape
    if mutant == "gshift":
        g = np.roll(g, 8)
    xh = (x - mu) * rs
    gy = dy * g
    c1 = (lane_sum(gy) / F(D - 1 if mutant == "c1dm1" else D))[:, None]
    c2 = (lane_sum(gy * xh) / F(D))[:, None]
    if mutant == "noc2":
        c2 = c2 * F(0)
    o = rs * (gy - c1 - xh * c2)
    if add is not None:
        o = o + f32(add)
    blocks = R.ln_bwd_blocks(M, D)
    drop = M - 1 if mutant == "droprow" else None
    return (R.bf(torch.from_numpy(o)), rows_sum(dy * xh, blocks, drop), rows_sum(dy, blocks, drop), rows_sum(o, blocks, drop))


def ce32(logits, targets, C, gscale, mutant=None):
    z, t = f32(logits)[:, :C], f32(targets)
    B = z.shape[0]
    gs = F(gscale)
    with np.errstate(all="ignore"):
        mx = z.max(axis=1, keepdims=True)
        am = z.argmax(axis=1)[:, None]                       # the first maximum
        if mutant == "nomax":
            mx = mx * F(0)
        e = np.exp(z - mx, dtype=F)
        first = np.arange(C)[None, :] == am
        se = e.sum(axis=1, keepdims=True, dtype=F)
        so = np.where(first, F(0), e).sum(axis=1, keepdims=True, dtype=F)
        st = np.ones((B, 1), F) if mutant == "st1" else t.sum(axis=1, keepdims=True, dtype=F)
        stl = (t * z).sum(axis=1, keepdims=True, dtype=F)
        lse = mx + np.log(se, dtype=F)
        loss = (lse * st - stl)[:, 0]
        p = np.exp(z - lse, dtype=F)
        if mutant == "old":
            gr = (p * st - t) * gs
        else:
            gr = (p * (st - t) - t * np.where(first, so / se, F(1) - p)) * gs
    return loss, R.bf(torch.from_numpy(gr.astype(F)))


def gelu32(x, bwd, mutant=None):
    xf = x.float()
    if mutant == "tanh":
        xd = xf.clone().requires_grad_(True)
        y = torch.nn.functional.gelu(xd, approximate="tanh")
        if bwd:
            y.sum().backward()
            return R.bf(xd.grad)
        return R.bf(y.detach())
    cdf2 = 1 + torch.erf(xf * 0.70710678118654752)
    if bwd:
        return R.bf(0.5 * cdf2 + xf * 0.3989422804014327 * torch.exp(-0.5 * xf * xf))
    return R.bf(0.5 * xf * cdf2)


# ---- 1. the references against torch double autograd --------------------------------------------------------------------
def test_references_agree_with_torch_double_autograd():
    g = torch.Generator().manual_seed(1)
    M, D = 11, 200
    x, gamma, beta, dy, add = R.ln_random_inputs(M, D)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = torch.nn.functional.layer_norm(xd, (D,), gd, bd, R.EPS)
    y.backward(dy.double())
    yr, mean, rstd, _ = R.ln_fwd_ref(x, gamma, beta)
    r = R.ln_bwd_ref(dy, x, torch.from_numpy(mean), torch.from_numpy(rstd), gamma, add)
    scale = lambda a: max(1.0, float(np.abs(a).max()))      # noqa: E731
    figs = dict(y=np.abs(yr - y.detach().numpy()).max() / scale(yr), dx=np.abs(r["dx"] - xd.grad.numpy()).max() / scale(r["dx"]),
                dxa=np.abs(r["dxa"] - (xd.grad + add.double()).numpy()).max() / scale(r["dxa"]),
                dgamma=np.abs(r["dgamma"] - gd.grad.numpy()).max() / scale(r["dgamma"]),
                dbeta=np.abs(r["dbeta"] - bd.grad.numpy()).max() / scale(r["dbeta"]),
                dcol=np.abs(r["dcol"] - (xd.grad + add.double()).sum(0).numpy()).max() / scale(r["dcol"]))
    xs = (torch.randn(4096, generator=g) * 3).double().requires_grad_(True)
    ge = torch.nn.functional.gelu(xs)
    ge.sum().backward()
    figs["gelu"] = np.abs(R.gelu_ref(xs) - ge.detach().numpy()).max()
    figs["gelu_grad"] = np.abs(R.gelu_grad_ref(xs) - xs.grad.numpy()).max()
    logits, targets, _ = R.ce_inputs(37, 10, 16)
    zd = logits[:, :10].double().requires_grad_(True)
    loss = -(targets.double() * torch.log_softmax(zd, -1)).sum(-1)
    (loss.sum() / 37).backward()
    lr, dr, _, _ = R.soft_ce_ref(logits, targets, 10, 1.0 / 37)
    figs["ce_loss"] = np.abs(lr - loss.detach().numpy()).max() / scale(lr)
    figs["ce_grad"] = np.abs(dr - zd.grad.numpy()).max()
    print("references vs torch double autograd:", " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    assert max(figs.values()) <= 1e-12, figs


def test_bf16_bookkeeping():
    v = np.array([1.0, 1.5, 2.0, 255.0, 256.0, -0.75, 3e-39, 0.0])
    assert np.array_equal(R.bf16_step(v), [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133])
    a = torch.tensor([1.0, -1.0, 0.0, -0.0, 257.0, 259.0]).to(torch.bfloat16)
    assert R.ordered(a).tolist()[2] == R.ordered(a).tolist()[3] == 0
    assert a.float().tolist()[4:] == [256.0, 260.0]                      # the ties of the exact families round to even
    assert R.steps_off(a, np.array([1.0 + 2.0 ** -7, -1.0, 0.0, 0.0, 256.0, 262.0])).tolist() == [1, 0, 0, 0, 0, 1]


# ---- 2. + 3. LayerNorm forward ---------------------------------------------------------------------------------------------
FWD_MUTANTS = ("dm1", "noeps", "skipvec", "onepass")


@pytest.mark.parametrize("M,D", R.LN_FWD_EXACT)
def test_ln_fwd_exact_family(M, D):
    x, gamma, beta, mean, q = R.ln_exact_fwd_inputs(M, D)
    _, mr, rr, var = R.ln_fwd_ref(x, gamma, beta)
    assert np.array_equal(mr, mean) and np.allclose(var, q / D, rtol=1e-15)
    rat = R.ln_fwd_ratios(x, gamma, beta, ln_fwd32(x, gamma, beta), exact=mean)
    print(f"ln_fwd exact ({M}, {D}) fp32 restatement:", rat)
    assert R.passes(rat)
    if M <= 16:
        caught = {m: not R.passes(R.ln_fwd_ratios(x, gamma, beta, ln_fwd32(x, gamma, beta, mutant=m), exact=mean)) for m in ("dm1", "skipvec")}
        print("   mutants rejected:", caught)
        assert all(caught.values())


@pytest.mark.parametrize("M,D", R.LN_RANDOM)
def test_ln_fwd_random_family_and_mutants(M, D):
    x, gamma, beta, _, _ = R.ln_random_inputs(M, D)
    rat = R.ln_fwd_ratios(x, gamma, beta, ln_fwd32(x, gamma, beta))
    print(f"ln_fwd random ({M}, {D}) fp32 restatement:", rat)
    assert R.passes(rat)
    caught = {m: not R.passes(R.ln_fwd_ratios(x, gamma, beta, ln_fwd32(x, gamma, beta, mutant=m))) for m in FWD_MUTANTS
              if D > 8 or m != "onepass"}          # D = 8: the eight squares near 900 of row 0 add up exactly
    print("   mutants rejected:", caught)
    assert all(caught.values())


# ---- LayerNorm backward ----------------------------------------------------------------------------------------------------
BWD_MUTANTS = ("noc2", "c1dm1", "gshift", "droprow")


@pytest.mark.parametrize("M,D", R.LN_BWD_EXACT)
def test_ln_bwd_exact_family(M, D):
    inp = R.ln_exact_bwd_inputs(M, D)
    for with_add in (False, True):
        add = inp["add"] if with_add else None
        got = ln_bwd32(inp["dy"], inp["x"], inp["mean"], inp["rstd"], inp["gamma"], add)
        assert R.ln_bwd_exact_ok(inp, got, with_add), (M, D, with_add)
    w = inp["want"]
    if M * D <= 1 << 20:                                                                           # the fp64 reference says the same
        r = R.ln_bwd_ref(inp["dy"], inp["x"], inp["mean"], inp["rstd"], inp["gamma"], inp["add"])
        assert np.array_equal(r["dxa"], w["dxa"].numpy()) and np.array_equal(r["dgamma"], w["dgamma"].numpy())
        assert np.array_equal(r["dcol"], w["dcol_add"].numpy()) and float(np.abs(r["c1"]).max()) == 0 == float(np.abs(r["c2"]).max())
    if M >= 259:
        assert w["dbeta"][:2].tolist() == [257, 259]
    caught = {m: not R.ln_bwd_exact_ok(inp, ln_bwd32(inp["dy"], inp["x"], inp["mean"], inp["rstd"], inp["gamma"], None, mutant=m), False)
              for m in ("gshift", "droprow") if (D > 8 and M * D <= 1 << 20) or m != "gshift"}     # D = 8 is one vector: no shift
    print(f"ln_bwd exact ({M}, {D}): fp32 restatement exact; mutants rejected: {caught}")
    assert all(caught.values())


@pytest.mark.parametrize("M,D", [s for s in R.LN_RANDOM if s[1] <= R.LN_BWD_MAX_D])
def test_ln_bwd_random_family_and_mutants(M, D):
    x, gamma, beta, dy, add = R.ln_random_inputs(M, D)
    _, mean, rstd = ln_fwd32(x, gamma, beta)                       # backward takes a forward's own fp32 mean / rstd
    mean, rstd = torch.from_numpy(mean), torch.from_numpy(rstd)
    for with_add in (False, True):
        a = add if with_add else None
        r = R.ln_bwd_ref(dy, x, mean, rstd, gamma, a)
        rat = R.ln_bwd_ratios(r, ln_bwd32(dy, x, mean, rstd, gamma, a), M, D, with_add)
        print(f"ln_bwd random ({M}, {D}) add={with_add} fp32 restatement:", rat)
        assert R.passes(rat)
    caught = {m: not R.passes(R.ln_bwd_ratios(r, ln_bwd32(dy, x, mean, rstd, gamma, add, mutant=m), M, D, True)) for m in BWD_MUTANTS
              if D > 8 or m != "gshift"}                                  # D = 8 is one vector: no shift
    print("   mutants rejected:", caught)
    assert all(caught.values())


# ---- soft-target cross entropy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,ld", list(R.CE_CASES))
def test_soft_ce_family_and_mutants(B, C, ld):
    logits, targets, kinds = R.ce_inputs(B, C, ld)
    gscale = 1.0 / B
    v = R.ce_verdict(logits, targets, C, gscale, ce32(logits, targets, C, gscale))
    print(f"soft_ce ({B}, {C}, {ld}) fp32 restatement: loss {v['loss']:.3f} of its bar, dlogits worst {int(v['steps'].max())} steps, "
          f"{v['floor_share']:.2e} on the floor (worst {v['floor_worst']:.3f} of it)")
    assert v["loss"] <= 1 and v["grad_ok"] and v["floor_share"] == 0       # the rewritten formula needs no floor at these inputs
    if any(k == "spread" for k in kinds) and C > 1:
        m = R.ce_verdict(logits, targets, C, gscale, ce32(logits, targets, C, gscale, mutant="nomax"))
        assert not (m["loss"] <= 1 and m["grad_ok"]), "maximum not subtracted"
    if any(k.startswith("sum") for k in kinds):
        m = R.ce_verdict(logits, targets, C, gscale, ce32(logits, targets, C, gscale, mutant="st1"))
        assert not (m["loss"] <= 1 and m["grad_ok"]), "sum(t) assumed 1"
    rows = [i for i, k in enumerate(kinds) if k in R.CE_CONFIDENT]
    if rows:
        m = R.ce_verdict(logits, targets, C, gscale, ce32(logits, targets, C, gscale, mutant="old"))
        per_kind = {kinds[i]: (int(m["steps"][i].max()), int(v["steps"][i].max())) for i in rows}
        print("   bf16 steps on the confident rows, exp(z - lse) st - t against the rewritten formula:", per_kind)
        assert not m["grad_ok"], "the former gradient formula"
        assert max(old for old, _ in per_kind.values()) > 1 and max(new for _, new in per_kind.values()) <= 1


# ---- GELU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bwd", [False, True])
def test_gelu_exhaustive_and_the_tanh_mutant(bwd):
    x = R.gelu_all_finite()
    ref = R.gelu_grad_ref(x) if bwd else R.gelu_ref(x)
    got = gelu32(x, bwd)
    ok, on_floor, worst = R.elementwise_verdict(got, ref, R.gelu_floor(x))
    xs = x.float().numpy()[on_floor]
    print(f"gelu {'bwd' if bwd else 'fwd'} fp32 restatement: {on_floor.mean():.4%} on the floor (x in [{xs.min()}, {xs.max()}]), "
          f"worst {worst:.3f} of it")
    assert torch.isfinite(got.float()).all() and ok.all() and on_floor.mean() <= 0.01
    ok_t, on_t, _ = R.elementwise_verdict(gelu32(x, bwd, "tanh"), ref, R.gelu_floor(x))
    print(f"   tanh approximation: {(~ok_t).sum()} elements outside, {on_t.mean():.2%} off by more than a step")
    assert not ok_t.all() or on_t.mean() > 0.01


# ---- column sums / sum of squares: the premise of the exact families ----------------------------------------------------
def test_exact_sum_premise():
    """Every partial sum of the exact families is an fp32 value in any order: sum|terms| stays below 2^24 units."""
    for M, N in R.COLSUM_EXACT:
        x, want = R.colsum_exact_inputs(M, N)
        assert float(x.float().abs().sum(0).max()) < 2 ** 24 and torch.equal(x.double().sum(0).long(), want)
        assert np.array_equal(reduce16(rows_sum(f32(x), 64)[None, :]), want.double().numpy())
    for n in R.SUMSQ_N:
        v, s = R.sumsq_exact_inputs(n)
        assert torch.equal(v, v.to(torch.bfloat16).float()) and float((v * v).sum()) == s
    for M, D in R.LN_BWD_EXACT:
        w = R.ln_exact_bwd_inputs(M, D)
        assert float((w["dy"].double().abs() * 12 * 16).sum(0).max()) < 2 ** 24


# ---- 4. the geometry the shapes were chosen from ------------------------------------------------------------------------
def test_shapes_meet_the_library_geometry():
    """ln_bwd_geometry / colsum_geometry through the library's workspace queries (host code, no GPU), and what the shapes are
    for: a second row per wave past the workgroup cap, 257 partial rows, the two-row forward form with an odd last wave."""
    from sfcvit._lib import lib
    for M, D in R.LN_BWD_EXACT + [s for s in R.LN_RANDOM if s[1] <= R.LN_BWD_MAX_D]:
        assert lib.sfcvit_layernorm_bwd_ws(M, D) == R.ln_bwd_blocks(M, D) * 3 * D * 4, (M, D)
    for M, N in R.COLSUM_EXACT:
        assert lib.sfcvit_colsum_workspace(M, N) == R.colsum_parts(M, N)[1] * N * 4, (M, N)
    two_rows = {s: R.ln_bwd_blocks(*s) * 4 < s[0] for s in R.LN_BWD_EXACT}
    assert two_rows == {(9, 8): False, (37, 200): False, (2053, 192): True, (1025, 520): False, (70, 1536): False, (33, 2048): False,
                        (2053, 2048): True, (300, 768): False, (3077, 768): True, (2053, 1024): True}
    assert R.ln_bwd_blocks(1025, 520) == 257 and R.ln_bwd_blocks(3077, 768) == 768 and R.ln_bwd_blocks(2053, 192) == 512
    assert [R.ln_fwd_form(*s) for s in R.LN_FWD_EXACT] == [("ln_fwd_kernel", 1)] * 3 + [("ln_fwd_kernel", 2)] * 2 + [("ln_fwd_kernel", 4)] * 2 \
        + [("ln_fwd_kernel", 8)] * 2 + [("ln_fwd2_kernel", 3), ("ln_fwd2_kernel", 4)]
    assert [R.colsum_parts(*s)[1] for s in R.COLSUM_EXACT] == [1, 256, 129, 209, 125]
    assert [R.sumsq_parts(n) for n in R.SUMSQ_N] == [1, 1, 2, 1024] and -(-(R.SUMSQ_N[-1] // 8) // 256) > 1024
    assert 4 * 3 * 2048 * 4 == 96 * 1024                      # ln_bwd_kernel<4> at D = 2048: 96 KiB of dynamic LDS
