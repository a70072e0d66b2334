"""References, bars and input families of the row-wise edge tests (tests/test_rowwise_ref_cpu.py qualifies them without a GPU,
tests/test_rowwise_edges_gpu.py holds the kernels of layernorm.hip / rowwise.hip / optim.hip to them).

References are plain fp64 (numpy; torch double for erfc and log_softmax) of the bf16 / fp32 values the kernel reads.

Bars are derived, not tuned.  u = 2^-24 is half an fp32 ulp, relative.  A sum of n terms added along chains of at most L
additions (a lane's serial part plus the levels of the butterfly or tree above it) is off by at most L u sum|terms|.  A bf16
output is the rounding of an fp32 value v with |v - ref| <= floor, and half a bf16 step of v is at most one step of ref, so a
bf16 output is held to  step(ref) + floor  with the floor counting the fp32 roundings of the kernel's documented evaluation.

    chain lengths
      LayerNorm row sums     ln_chain(D) = 8 VPL + 6, VPL = ceil(D / 512): a lane adds 8 VPL values, the butterfly has 6 levels
                             (the two-row and the column-chunk forms add fewer values per lane)
      column sums over rows  rows_chain: a wave's rows one after the other, 4 waves, ceil(parts / 64) partial rows per thread,
                             then 16 and 2 more (reduce_partials16)
    mean   = fl(sum x) / D                     |err| <= (L + 2) u sum|x| / D
    rstd   = rsqrt(sum (x - mean)^2 / D + eps) relative: the terms are positive, so the sum is relatively off by (L + 3) u (three
             roundings a term), the division and the addition by u each, and rsqrt halves all that; rsqrtf itself 2 ulp = 4 u; a
             mean off by d adds d^2 to the variance:   ((L + 5) / 2 + 4) u + d^2 / (2 (var + eps)),  d = the mean's bar
    y      = (x - mean) rstd gamma + beta      floor = |rstd gamma| d + |y - beta| (rho + 4 u) + u |y|, rho = rstd's bar
    dx     = rstd (gy - c1 - xh c2) [+ add]    floor = rstd (3 u |gy| + dc1 + |xh| dc2 + 5 u |xh c2| + 3 u |c1|) + u |add| + u |dx|,
             dc1 = (L + 2) u sum|gy| / D, dc2 = (L + 6) u sum|gy xh| / D   (xh carries two roundings, gy one)
    dgamma, dbeta, dcol                        (rows_chain + 4) u sum|terms| (+ for dcol the floors of the dx it adds)
    GELU   0.5 x (1 + erf(x / sqrt 2))         1 + erf is off by at most 6 u absolutely (argument 1 u, erff 4 ulp = 4 u just
             below 1, the addition 1 u and exact where it cancels), so the product by 3 u |x|:  floor = 3 u max(1, |x|), times
             |dy| backward (0.5 (1 + erf) carries the same 3 u; the density term has a relative error only)
    soft CE loss = lse sum(t) - sum(t z)       (2 Lc + 10 + 2 E|z - max|) u (|lse| + max|z|) sum(t), Lc = ceil(C / 64) + 6: the
             exponentials (2 u each plus u |z - max| of their argument, softmax-weighted: E|z - max|) and their sum give lse an
             absolute error, the logarithm 2 u, mx + log one rounding of |lse|, the two target sums Lc u each, two more
             roundings for the product and the difference
    soft CE dlogits                            one bf16 step of the rounded oracle, or 4 u gscale max(p sum(t), t) where two
             like-sized terms cancel (at most 1e-3 of the elements may need it).  Of p (sum(t) - t) - t (1 - p) one term is
             exactly 0 on a one-hot row (and when C = 1), so nothing cancels there and the floor is 0: without that the label
             column of a confident row, where the former formula is 12 and more steps off, would rest on a floor of 4 u
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
BF16 = torch.bfloat16
EPS = 1e-5


# ---- bf16 bookkeeping ------------------------------------------------------------------------------------------------------
def ordered(bf16):
    """bf16 tensor -> int32 keys in which neighbouring representable values differ by one (+0 and -0 coincide)."""
    b = bf16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def round_bf16(ref64):
    """fp64 numpy array -> the nearest bf16 (through fp32, as the kernels round)."""
    return torch.from_numpy(np.asarray(ref64, dtype=np.float64)).to(torch.float32).to(BF16)


def steps_off(got_bf16, ref64):
    """bf16 steps between a kernel's output and the rounded reference (int32 numpy array)."""
    return (ordered(got_bf16.cpu()) - ordered(round_bf16(ref64))).abs().numpy()


def bf16_step(ref64):
    """The spacing of bf16 at |ref|: 2^(floor(log2 |ref|) - 7), the subnormal spacing 2^-133 below 2^-126."""
    m, e = np.frexp(np.abs(np.asarray(ref64, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(np.where(m == 0, -125, e), -125) - 8)


def f64(t):
    return t.detach().cpu().to(torch.float64).numpy()


def bf(t):
    return t.to(BF16)


# ---- references ------------------------------------------------------------------------------------------------------------
def ln_fwd_ref(x, gamma, beta, eps=EPS):
    """-> y, mean, rstd, var (fp64) of bf16 inputs."""
    x, g, b = f64(x), f64(gamma), f64(beta)
    mean = x.mean(axis=1)
    var = ((x - mean[:, None]) ** 2).mean(axis=1)
    rstd = 1.0 / np.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * g + b, mean, rstd, var


def ln_bwd_ref(dy, x, mean, rstd, gamma, add=None):
    """mean / rstd are inputs (the fp32 values the kernel is given).  -> dict of dx, dxa (dx + add), dgamma, dbeta, dcol (column
    sums of dxa) and the intermediate quantities the bars need."""
    dy, x, g = f64(dy), f64(x), f64(gamma)
    mu, rs = f64(mean)[:, None], f64(rstd)[:, None]
    D = x.shape[1]
    xh = (x - mu) * rs
    gy = dy * g
    c1 = gy.sum(axis=1, keepdims=True) / D
    c2 = (gy * xh).sum(axis=1, keepdims=True) / D
    dx = rs * (gy - c1 - xh * c2)
    a = f64(add) if add is not None else np.zeros_like(dx)
    dxa = dx + a
    return dict(dx=dx, dxa=dxa, dgamma=(dy * xh).sum(axis=0), dbeta=dy.sum(axis=0), dcol=dxa.sum(axis=0),
                xh=xh, gy=gy, c1=c1, c2=c2, rs=rs, add=a, dy=dy)


def soft_ce_ref(logits, targets, C, gscale):
    """-> loss rows, dlogits [B, C], softmax p, lse (fp64), from log_softmax in double."""
    z = logits[:, :C].detach().cpu().double()
    t = targets.detach().cpu().double()
    lsm = torch.log_softmax(z, dim=-1)
    loss = -(t * lsm).sum(-1)
    p = lsm.exp()
    dl = (p * t.sum(-1, keepdim=True) - t) * gscale
    return loss.numpy(), dl.numpy(), p.numpy(), torch.logsumexp(z, dim=-1).numpy()


def gelu_ref(x):
    """0.5 x erfc(-x / sqrt 2): free of the 1 + erf cancellation."""
    xd = x.detach().cpu().double()
    return (0.5 * xd * torch.special.erfc(-xd / math.sqrt(2.0))).numpy()


def gelu_grad_ref(x):
    xd = x.detach().cpu().double()
    return (0.5 * torch.special.erfc(-xd / math.sqrt(2.0)) + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2.0 * math.pi)).numpy()


# ---- launch geometry restated (csrc/rowwise.cpp; tests/test_rowwise_ref_cpu.py checks it against the library) ---------------
def ln_fwd_form(M, D):
    """-> kernel, vectors per lane."""
    if D in (768, 1024) and M >= 4096:
        return "ln_fwd2_kernel", 3 if D == 768 else 4
    return "ln_fwd_kernel", 1 if D <= 512 else 2 if D <= 1024 else 4 if D <= 2048 else 8


def ln_bwd_blocks(M, D):
    return min(-(-M // 4), 768 if D == 768 else 512)


def ln_bwd_form(M, D, add):
    cols = D in (768, 1024)
    inst = D // 256 if cols else 1 if D <= 512 else 2 if D <= 1024 else 4
    return "ln_bwd%s_kernel<%d, %s>" % ("_cols" if cols else "", inst, "true" if add else "false")


def colsum_parts(M, N):
    """-> rows per block, partial rows."""
    col_blocks = -(-N // 256)
    row_blocks = max(1, min(256, 1024 // col_blocks))
    rpb = -(-(-(-M // row_blocks)) // 8) * 8
    return rpb, -(-M // rpb)


def sumsq_parts(n):
    return min(-(-((n - 1) // 8 + 1) // 256), 2048, 1024)


def ln_chain(D):
    return 8 * -(-D // 512) + 6


def reduce16_chain(parts):
    return -(-parts // 64) + 16 + 2


def ln_rows_chain(M, D):
    blocks = ln_bwd_blocks(M, D)
    return -(-M // (4 * blocks)) + 4 + reduce16_chain(blocks)


# ---- bars ------------------------------------------------------------------------------------------------------------------
def mean_bar(x, exact=False):
    """fp32 mean against the fp64 mean; exact: every partial sum is an fp32 value, so is the quotient -> 0."""
    x = f64(x)
    if exact:
        return np.zeros(x.shape[0])
    return (ln_chain(x.shape[1]) + 2) * U * np.abs(x).sum(axis=1) / x.shape[1]


def rstd_bar(x, var, eps=EPS, exact=False):
    """RELATIVE bar of the fp32 rstd against (var + eps)^-1/2."""
    D = x.shape[1]
    if exact:            # exact sum: the division, the addition of eps (half each) and rsqrtf's 2 ulp
        return np.full(x.shape[0], 5 * U)
    d = mean_bar(x)
    return ((ln_chain(D) + 5) / 2 + 4) * U + d * d / (2 * (var + eps))


def ln_y_bar(x, gamma, beta, eps=EPS):
    y, _, rstd, var = ln_fwd_ref(x, gamma, beta, eps)
    g, b = f64(gamma), f64(beta)
    floor = np.abs(rstd[:, None] * g) * mean_bar(x)[:, None] + np.abs(y - b) * (rstd_bar(x, var, eps)[:, None] + 4 * U) + U * np.abs(y)
    return bf16_step(y) + floor


def ln_dx_floor(r):
    """fp32 floor of dx + add (before the bf16 rounding) from ln_bwd_ref's dict."""
    D = r["gy"].shape[1]
    L = ln_chain(D)
    dc1 = (L + 2) * U * np.abs(r["gy"]).sum(axis=1, keepdims=True) / D
    dc2 = (L + 6) * U * np.abs(r["gy"] * r["xh"]).sum(axis=1, keepdims=True) / D
    xh = np.abs(r["xh"])
    return (np.abs(r["rs"]) * (3 * U * np.abs(r["gy"]) + dc1 + xh * dc2 + 5 * U * xh * np.abs(r["c2"]) + 3 * U * np.abs(r["c1"]))
            + U * np.abs(r["add"]) + U * np.abs(r["dxa"]))


def ln_dx_bar(r, with_add):
    return bf16_step(r["dxa"] if with_add else r["dx"]) + ln_dx_floor(r)


def ln_colgrad_bars(r, M, D, as_bf16=False):
    """-> bars of dgamma, dbeta, dcol (fp32 outputs; as_bf16 adds a bf16 step of the reference)."""
    k = (ln_rows_chain(M, D) + 4) * U
    bars = dict(dgamma=k * np.abs(r["dy"] * r["xh"]).sum(axis=0), dbeta=k * np.abs(r["dy"]).sum(axis=0),
                dcol=k * np.abs(r["dxa"]).sum(axis=0) + ln_dx_floor(r).sum(axis=0))
    if as_bf16:
        bars = {n: b + bf16_step(r[n]) for n, b in bars.items()}
    return bars


GELU_K = 3


def gelu_floor(x, dy=None):
    xd = np.abs(f64(x))
    fl = GELU_K * U * np.maximum(1.0, xd)
    return fl if dy is None else fl * np.abs(f64(dy))


def elementwise_verdict(got_bf16, ref64, floor):
    """-> (ok mask, on-floor mask, worst |err| / floor among the elements resting on the floor): an element passes within one
    bf16 step of the rounded reference, or within the floor."""
    st = steps_off(got_bf16, ref64).reshape(-1)
    err = np.abs(f64(got_bf16).reshape(-1) - np.asarray(ref64).reshape(-1))
    fl = np.asarray(floor).reshape(-1)
    on_floor = st > 1
    ok = ~on_floor | (err <= fl)
    with np.errstate(divide="ignore"):
        worst = float((err[on_floor] / fl[on_floor]).max()) if on_floor.any() else 0.0
    return ok, on_floor, worst


def ce_loss_bar(logits, targets, C):
    z = logits[:, :C].detach().cpu().double().numpy()
    t = targets.detach().cpu().double().numpy()
    _, _, p, lse = soft_ce_ref(logits, targets, C, 1.0)
    mx = z.max(axis=1)
    spread = (p * np.abs(z - mx[:, None])).sum(axis=1)
    k = 2 * (-(-C // 64) + 6) + 10 + 2 * spread
    return k * U * (np.abs(lse) + np.abs(z).max(axis=1)) * np.abs(t).sum(axis=1)


def ce_grad_floor(logits, targets, C, gscale):
    t = targets.detach().cpu().double().numpy()
    _, _, p, _ = soft_ce_ref(logits, targets, C, gscale)
    st = t.sum(axis=1, keepdims=True)
    cancels = (p * (st - t) != 0) & (t * (1 - p) != 0)       # one-hot rows: one of the two terms is exactly 0, nothing cancels
    return np.where(cancels, 4 * U * gscale * np.maximum(p * st, t), 0.0)


# ---- verdicts: worst |err| / bar per output ------------------------------------------------------------------------------
def ratio(err, bar):
    err, bar = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bar, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def ln_fwd_ratios(x, gamma, beta, got, exact=None):
    y, mean, rstd = got
    yr, mr, rr, var = ln_fwd_ref(x, gamma, beta)
    if exact is not None:                                                      # the exact family: mean bit for bit, y not asserted
        out = {}
        out["mean"] = 0.0 if np.array_equal(np.asarray(mean, dtype=np.float64), exact) else np.inf
        out["rstd"] = ratio(np.asarray(rstd, dtype=np.float64) / rr - 1, rstd_bar(x, var, exact=True))
    else:
        out = dict(y=ratio(f64(y) - yr, ln_y_bar(x, gamma, beta)))
        out["mean"] = ratio(np.asarray(mean, dtype=np.float64) - mr, mean_bar(x))
        out["rstd"] = ratio(np.asarray(rstd, dtype=np.float64) / rr - 1, rstd_bar(x, var))
    return out


def ln_bwd_ratios(ref, got, M, D, with_add):
    dx, dg, db, dc = got
    bars = ln_colgrad_bars(ref, M, D)
    return dict(dx=ratio(f64(dx) - (ref["dxa"] if with_add else ref["dx"]), ln_dx_bar(ref, with_add)),
                dgamma=ratio(dg - ref["dgamma"], bars["dgamma"]), dbeta=ratio(db - ref["dbeta"], bars["dbeta"]),
                dcol=ratio(dc - ref["dcol"], bars["dcol"]))


def ln_bwd_exact_ok(inp, got, with_add):
    """The exact family's assertion: everything equal to the integer-arithmetic answer."""
    w = inp["want"]
    dx, dg, db, dc = got
    return (np.array_equal(f64(dx), (w["dxa"] if with_add else w["dx"]).numpy()) and np.array_equal(dg, w["dgamma"].numpy())
            and np.array_equal(db, w["dbeta"].numpy()) and np.array_equal(dc, (w["dcol_add"] if with_add else w["dcol"]).numpy()))


def ce_verdict(logits, targets, C, gscale, got):
    """got = (loss rows fp64, dlogits bf16 [B, C]) -> loss: worst |err| / bar; grad_ok: every element within a step or its floor
    and at most 1e-3 of them more than a step off; steps: bf16 steps from the rounded oracle, per element."""
    loss, dl = got
    lr, dr, _, _ = soft_ce_ref(logits, targets, C, gscale)
    ok, on_floor, worst = elementwise_verdict(dl, dr, ce_grad_floor(logits, targets, C, gscale))
    return dict(loss=ratio(loss - lr, ce_loss_bar(logits, targets, C)), grad_ok=bool(ok.all() and on_floor.mean() <= 1e-3),
                floor_share=float(on_floor.mean()), floor_worst=worst, steps=steps_off(dl, dr))


def passes(ratios):
    return all(v <= 1 for v in ratios.values())


# ---- input families --------------------------------------------------------------------------------------------------------
LN_FWD_EXACT = [(5, 8), (7, 200), (9, 512), (6, 520), (1023, 1024), (5, 1032), (6, 2048), (5, 2056), (5, 4096), (4097, 768), (4099, 1024)]
LN_BWD_EXACT = [(9, 8), (37, 200), (2053, 192), (1025, 520), (70, 1536), (33, 2048), (2053, 2048), (300, 768), (3077, 768), (2053, 1024)]
LN_RANDOM = [(64, 8), (64, 200), (64, 520), (64, 1536), (33, 2048), (33, 2056), (17, 4096), (300, 768), (300, 1024)]
LN_BWD_MAX_D = 2048
COLSUM_EXACT = [(7, 8), (2048, 256), (2056, 256), (5000, 328), (1000, 1032)]
SUMSQ_N = [3, 8, 2051, 256 * 8 * 1024 + 2048 + 5]
CE_CASES = {(5, 1, 8): ["random", "sum0.5", "sum2", "equal", "spread"],
            (37, 10, 16): ["random", "lead8", "lead12", "lead16", "lead20", "smooth8", "smooth12", "smooth16", "smooth20", "twohot",
                           "sum0.5", "sum2", "equal", "spread"],
            (6, 64, 64): ["lead8", "lead12", "lead16", "lead20", "twohot", "random"],
            (6, 65, 72): ["smooth16", "smooth20", "lead20", "sum0.5", "sum2", "spread"],
            (5, 77, 80): ["lead16", "smooth12", "equal", "spread", "twohot"],
            (7, 1000, 1000): ["random", "lead8", "lead12", "lead16", "lead20", "smooth20", "spread"]}
CE_CONFIDENT = ("lead12", "lead16", "lead20")      # the rows the former gradient formula loses


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1000003, 10007, 101, 1))))


def ln_exact_fwd_inputs(M, D):
    """x: integers in [-4, 4]; row r sums to k_r D / 8 with k_r = 7 r mod 33 - 16, so its mean is k_r / 8 exactly and
    neighbouring rows differ.  -> x bf16, gamma, beta, mean (fp64, exact), sum of (x - mean)^2 (fp64, exact)."""
    g = _gen(1, M, D)
    r = torch.arange(M)
    k = (7 * r) % 33 - 16
    base = torch.div(k, 8, rounding_mode="floor")                          # -2 .. 1
    ones = (k - 8 * base) * (D // 8)                                       # columns that carry base + 1
    x = base[:, None] + (torch.arange(D)[None, :] < ones[:, None]).long()  # -2 .. 2
    d = torch.randint(-2, 3, (M, D // 2), generator=g)                     # zero-sum perturbation on pairs (j, j + D / 2)
    x = x + torch.cat([d, -d], dim=1)
    perm = torch.argsort(torch.rand(M, D, generator=g), dim=1)             # the pairs and the +1 columns land anywhere
    x = torch.gather(x, 1, perm)
    assert int(x.abs().max()) <= 4 and torch.equal(x.sum(1) * 8, k * D)
    mean = k.double() / 8
    q = ((x.double() - mean[:, None]) ** 2).sum(1)
    gamma = bf(1 + 0.25 * torch.randint(-2, 3, (D,), generator=g).float())
    beta = bf(0.5 * torch.randint(-2, 3, (D,), generator=g).float())
    return bf(x.float()), gamma, beta, mean.numpy(), q.numpy()


def ln_exact_bwd_inputs(M, D):
    """Columns j and j + D / 2 carry equal x and gamma and opposite dy, so both row sums are exactly 0 and dx = rstd dy gamma.
    mean = k / 8, rstd in {0.5, 1, 2} per row, x in [-4, 4], dy in [-3, 3], gamma in {+-0.5, +-1, 2}, add in [-3, 3].  With 259 rows
    or more, dy's columns 0 and 1 sum to 257 and 259: ties of the bf16 dbeta.  -> dict of tensors and the integer-arithmetic
    answers (fp64 holding exact values)."""
    g = _gen(2, M, D)
    h = D // 2
    xi = torch.randint(-4, 5, (M, h), generator=g)
    dyi = torch.randint(-3, 4, (M, h), generator=g)
    if M >= 259:
        dyi[:, 0] = (torch.arange(M) < 257).long()
        dyi[:, 1] = (torch.arange(M) < 259).long()
    g2 = torch.tensor([-1, 1, -2, 2, 4])[torch.randint(0, 5, (h,), generator=g)]        # 2 gamma
    xi, dyi, g2 = torch.cat([xi, xi], 1), torch.cat([dyi, -dyi], 1), torch.cat([g2, g2])
    mu8 = torch.randint(-16, 17, (M,), generator=g)                                        # 8 mean
    rs2 = torch.tensor([1, 2, 4])[torch.randint(0, 3, (M,), generator=g)]                  # 2 rstd
    add = torch.randint(-3, 4, (M, D), generator=g)
    xh16 = (8 * xi - mu8[:, None]) * rs2[:, None]                                          # 16 x_hat
    dx4 = rs2[:, None] * dyi * g2[None, :]                                                 # 4 dx
    want = dict(dx=dx4.double() / 4, dxa=dx4.double() / 4 + add, dgamma=(dyi * xh16).sum(0).double() / 16, dbeta=dyi.sum(0).double(),
                dcol=dx4.sum(0).double() / 4, dcol_add=(dx4 + 4 * add).sum(0).double() / 4)
    assert float(want["dxa"].abs().max()) <= 15 and float(want["dgamma"].abs().max()) * 16 < 2 ** 24
    return dict(x=bf(xi.float()), dy=bf(dyi.float()), gamma=bf(g2.float() / 2), mean=mu8.float() / 8, rstd=rs2.float() / 2,
                add=bf(add.float()), want=want)


def ln_random_inputs(M, D):
    """Rows 0..3 are edges (mean 30 with spread 0.05; constant; spread 1e-3, where eps dominates; zeros with one entry of 100), the
    rest randn * 1.5 + 0.3.  dy has a mean of its own (c1 counts).  -> x, gamma, beta, dy, add (bf16)."""
    g = _gen(3, M, D)
    x = torch.randn(M, D, generator=g) * 1.5 + 0.3
    x[0] = torch.randn(D, generator=g) * 0.05 + 30
    x[1] = 2.5
    x[2] = torch.randn(D, generator=g) * 1e-3
    x[3] = 0
    x[3, 5] = 100.0
    gamma = 1 + 0.2 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g) + 0.5
    add = torch.randn(M, D, generator=g)
    return bf(x), bf(gamma), bf(beta), bf(dy), bf(add)


def colsum_exact_inputs(M, N):
    """Integers in [-8, 8]; with 259 rows or more columns 0 and 1 sum to 257 and 259 (bf16 ties).  -> x bf16, int64 sums."""
    x = torch.randint(-8, 9, (M, N), generator=_gen(4, M, N))
    if M >= 259:
        x[:, 0] = (torch.arange(M) < 257).long()
        x[:, 1] = (torch.arange(M) < 259).long()
    return bf(x.float()), x.sum(0)


def sumsq_exact_inputs(n):
    """Entries in {0, +-1, +-2}; the sum of squares stays below 2^24.  -> fp32 tensor (bf16-exact), the integer sum."""
    v = torch.randint(-2, 3, (n,), generator=_gen(5, n)).float()
    s = int((v.double() ** 2).sum())
    assert s + 1000 < 2 ** 24
    return v, s


def ce_inputs(B, C, ld):
    """The rows of CE_CASES[(B, C, ld)], cycled over B rows.  -> logits bf16 [B, ld] (padding columns hold 7.0, which the kernel
    must not read into the row), targets fp32 [B, C], the kind of every row."""
    g = _gen(6, B, C, ld)
    kinds = [CE_CASES[(B, C, ld)][i % len(CE_CASES[(B, C, ld)])] for i in range(B)]
    z = torch.full((B, ld), 7.0)
    t = torch.zeros(B, C)
    for i, kind in enumerate(kinds):
        zi = torch.randn(C, generator=g) * 3
        ti = torch.softmax(torch.randn(C, generator=g), -1)
        k = (3 + 5 * i) % C
        if kind.startswith("lead") or kind.startswith("smooth"):
            gap = float("".join(ch for ch in kind if ch.isdigit()))
            zi = torch.randn(C, generator=g)
            zi[k] = -100.0
            zi[k] = float(bf(zi.max())) + gap
            ti = torch.zeros(C)
            ti[k] = 1.0
            if kind.startswith("smooth"):
                ti = 0.9 * ti + 0.1 / C
        elif kind == "twohot":
            ti = torch.zeros(C)
            ti[k] = 0.6
            ti[(k + 7) % C] += 0.4
        elif kind == "sum0.5":
            ti = ti * 0.5
        elif kind == "sum2":
            ti = ti * 2.0
        elif kind == "equal":
            zi = torch.full((C,), -3.25)
        elif kind == "spread":
            zi = torch.linspace(-1500.0, 1500.0, C)[torch.randperm(C, generator=g)] if C > 1 else torch.tensor([1500.0])
        z[i, :C] = zi
        t[i] = ti
    return bf(z), t.float().contiguous(), kinds


def gelu_all_finite():
    """All 65 280 finite bf16 patterns."""
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    x = allb[torch.isfinite(allb.float())]
    assert x.numel() == 65280
    return x.contiguous()
