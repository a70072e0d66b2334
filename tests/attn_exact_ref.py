"""Exact-answer inputs for the unmasked attention kernels (csrc/attention_seq.hip, attention_bwd_fused.hip, attention_long.hip,
attention.hip, attention_wide.hip, attention_wide_stream.hip) and their fp64 expectations.  CPU only; the claims made here are
proven by tests/test_attn_exact_ref_cpu.py and asserted on the GPU by tests/test_attention_exact_gpu.py.

All values are small integers or dyadic numbers bf16 holds exactly, and every (batch, head) item has data of its own.

uniform   q = 0, k arbitrary, v[j, d] = a_d + sign_d s_j with integer a_d in -3 .. 3 and integer |s_j| >= 8 summing to 0 over the
          keys.  Every score is 0, so lse = log N and out[., d] = a_d: the forward's sum N a_d is an exact integer, and bf16 takes
          it back to a_d however the kernel divides by l = N.  One key too few or too many moves lse by about 1 / N and out by at
          least 8 / N -- visible in the columns with a_d = 0 (any non-zero is) and |a_d| = 1.  Backward: dK = 0 (q = 0); every
          dV row is P colsum(dO) with P = bf16(fp32(1 / N)), exact in fp32 -- unless 1 / N lies within 2^-16 (relative) of a bf16
          rounding midpoint, where the kernel's exp2(-lse log2 e) may land on the other side (uniform_dv_exact); dQ rounds dS to
          bf16 and gets the bound of the kernel-roundings test.
one-hot   k_j distinct +-1 codes, q_i = g k_pi(i) with pi(i) = (a i + c) mod N, a coprime to N (it crosses every block and
          chunk boundary), g a power of two.  out_i = v_pi(i), lse_i = g hd scale, dV the scatter of dO, dQ = dK = 0.
ties      q_i = g (k_a(i) + k_b(i)), b(i) = a(i) + max(1, N / 2): both scores are the same integer whatever the kernel does with
          it, so P = 1/2, 1/2; every key serves two queries.  out = (v_a + v_b) / 2, dS = +-(dP_a - dP_b) / 4 scale, all short
          dyadic numbers.  With dropout p = 0.5 the factor 1 / (1 - p) = 2 is exact as well.  At N = 1 there is one key (P = 1).

Gain: the smallest power of two for which the probability outside the selected keys is below 2^-30, in fp64 for the codes used.
What that leaves: the selected probabilities round to exactly 1 or 1/2 in fp32 and bf16, so every output whose expectation is
NOT zero is exact -- the leak, bounded here in fp64 (`leak`), is below 2^-12 of the smallest non-zero expectation and the final
bf16 rounding removes it.  An output whose expectation IS zero (dQ and dK of one-hot, the zeros of a sparse dO scatter) holds
the leak itself, about 2^-30 times the size of the terms: not zero, so `wrong` asks |got| <= `allow` there (the leak, plus an fp32
ulp of the terms per accumulation step: see `allow`), and bit equality everywhere else.  (A gain at which fp32 exp underflows would make them zero; it would also put lse in the hundreds.)
A zero padding key with score 0 is invisible to one-hot and ties for the same reason -- exp(-g hd scale) -- and is what the
uniform design is for."""
import math

import torch

F64 = torch.float64
MASS = 2.0 ** -30
CHUNK = 64                                                      # items per slab of the [items, N, N] fp64 work


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(int(sum((i + 1) * 1000003 * (int(k) + 17) for i, k in enumerate(key)) % (2 ** 31)))
    return g


def rb(t):
    """Round to bf16 (through fp32, as the kernels do), back in fp64."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def ints(lo, hi, shape, g, nonzero=False):
    t = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    if nonzero:
        t = torch.where(t == 0, torch.full_like(t, float(hi)), t)
    return t


def uniform_dv_exact(N):
    """False where bf16(1 / N) is not safely decided: 1 / N within 2^-16 (relative) of a bf16 rounding midpoint."""
    x = 1.0 / N
    m, e = math.frexp(x)                                        # x = m 2^e, m in [0.5, 1): bf16 keeps 8 bits of m
    t = m * 256.0
    return abs((t - math.floor(t)) - 0.5) / t >= 2.0 ** -16


def _perm(N, item):
    a = 37 + 2 * item
    while math.gcd(a, N) != 1:
        a += 2
    c = 11 + 5 * item
    return (a * torch.arange(N) + c) % N


def _zero_sum(N, g):
    """Integers |s_j| >= 8 summing to 0 (N = 1: the single 0)."""
    if N == 1:
        return torch.zeros(1, dtype=F64)
    t = ints(8, 60, (N,), g)
    s = torch.zeros(N, dtype=F64)
    n2 = N - 3 if N % 2 else N
    s[0:n2:2], s[1:n2:2] = t[0:n2:2], -t[0:n2:2]
    if N % 2:
        s[N - 3], s[N - 2], s[N - 1] = t[N - 3], t[N - 2], -(t[N - 3] + t[N - 2])
    return s[torch.randperm(N, generator=g)]


def build(design, B, H, N, hd, scale=None, tag=0):
    """-> dict: q, k, v, do [items, N, hd] fp64 (items = B * H, item = b * H + h), sel [items, N, N] bool (None for uniform),
    gain, scale (the fp32 value the kernel receives, as a Python float), and the shape."""
    scale = float(torch.tensor(hd ** -0.5 if scale is None else scale, dtype=torch.float32))
    I = B * H
    c = dict(design=design, B=B, H=H, N=N, hd=hd, scale=scale, pow2=math.frexp(scale)[0] == 0.5, gain=1.0, sel=None)
    g = _gen(N, hd, I, tag, len(design))
    if design == "uniform":
        a = ints(-3, 3, (I, 1, hd), g)
        a[:, :, 0], a[:, :, 1] = 0.0, 1.0                        # the two most sensitive columns are always there
        sgn = ints(0, 1, (I, 1, hd), g) * 2 - 1
        s = torch.stack([_zero_sum(N, g) for _ in range(I)])
        c.update(q=torch.zeros(I, N, hd, dtype=F64), k=ints(-3, 3, (I, N, hd), g, nonzero=True), v=a + sgn * s[:, :, None],
                 do=ints(-4, 4, (I, N, hd), g, nonzero=True), a=a)
        return c
    k = ints(0, 1, (I, N, hd), g) * 2 - 1
    gram = k @ k.transpose(1, 2)
    assert bool((gram - hd * torch.eye(N, dtype=F64) < hd).all()), "sign codes are not distinct"
    sel = torch.zeros(I, N, N, dtype=torch.bool)
    rows = torch.arange(N)
    for i in range(I):
        pi = _perm(N, i)
        sel[i, rows, pi] = True
        if design == "ties":
            sel[i, rows, (pi + max(1, N // 2)) % N] = True       # N = 1: the same key
    qs = sel.to(F64) @ k                                         # q / gain
    gain = 1.0
    while _off_mass(qs, k, sel, gain, scale) >= MASS:
        gain *= 2.0
        assert gain <= 64.0, "no gain up to 64 isolates the selected keys"
    if design == "onehot":
        v, do = ints(-8, 8, (I, N, hd), g, nonzero=True), ints(-3, 3, (I, N, hd), g, nonzero=True)
    else:
        v = ints(1, 7, (I, N, hd), g)
        do = torch.zeros(I, N, hd, dtype=F64)
        cols = torch.rand(I, N, hd, generator=g).argsort(-1)[..., :3]
        do.scatter_(-1, cols, ints(-2, 2, (I, N, 3), g, nonzero=True))     # |dO . v| <= 42: dK, two queries per key, stays in 8 bits
    c.update(q=gain * qs, k=k, v=v, do=do, sel=sel, gain=gain)
    return c


def _off_mass(qs, k, sel, gain, scale, term=None):
    """Largest total softmax probability outside the selected keys at this gain, fp64.  term: an additive [items, N, N] term of
    the scores (tests/attn_masked_exact_ref.py), finite or -inf."""
    worst = 0.0
    for lo in range(0, qs.shape[0], CHUNK):
        s = gain * scale * (qs[lo:lo + CHUNK] @ k[lo:lo + CHUNK].transpose(1, 2))
        if term is not None:
            s = s + term[lo:lo + CHUNK]
        sl = sel[lo:lo + CHUNK]
        top = torch.where(sl, s, torch.full_like(s, -math.inf)).amax(-1, keepdim=True)
        assert bool((torch.where(sl, s, top) == top).all()), "the selected keys of a row do not tie"
        worst = max(worst, float(torch.where(sl, torch.zeros_like(s), torch.exp(s - top)).sum(-1).max()))
    return worst


def pack(c):
    """q | k | v as the bf16 [B, N, 3 H hd] tensor the kernels read, dO as [B, N, H hd]."""
    B, H, N, hd = c["B"], c["H"], c["N"], c["hd"]
    un = lambda t: t.reshape(B, H, N, hd).permute(0, 2, 1, 3).reshape(B, N, H * hd)       # noqa: E731
    qkv = torch.cat([un(c["q"]), un(c["k"]), un(c["v"])], -1).to(torch.float32).to(torch.bfloat16)
    return qkv, un(c["do"]).to(torch.float32).to(torch.bfloat16)


def unpack(c, t):
    """[B, N, H hd] (any dtype) -> fp64 [items, N, hd]."""
    B, H, N, hd = c["B"], c["H"], c["N"], c["hd"]
    return t.to(F64).reshape(B, N, H, hd).permute(0, 2, 1, 3).reshape(B * H, N, hd)


def ideal_p(c, rounded=True):
    """The probabilities the design stands for: 1 / selected keys of the row, or 1 / N (rounded: as bf16(fp32(1 / N)), what the
    backward kernels multiply dO by)."""
    if c["sel"] is None:
        p = torch.tensor(1.0 / c["N"], dtype=F64)
        return (rb(p) if rounded else p).expand(c["B"] * c["H"], c["N"], c["N"])
    return c["sel"].to(F64) / c["sel"].sum(-1, keepdim=True)


def expect(c, keep=None, p=0.0, rounded=True):
    """fp64 expectations from the ideal probabilities.  keep: bool [items, N, N], the keys dropout keeps (p > 0).
    c["term"] (optional, [items, N, N], finite or -inf; tests/attn_masked_exact_ref.py): an additive term of the scores -- it moves
    lse and the leak, the ideal probabilities come from c["sel"] as ever; with c["table_terms"] the un-scaled P (keep dP - delta)
    of every pair is kept as well (g, and g_leak: what the off-selection probability can add to it).
    -> out, lse, delta, dq, dk, dv [items, N, hd] (lse, delta [items, N]); ds (what the kernels round to bf16, scale included),
    pm (P keep / (1 - p)); terms_dq, terms_dk, terms_dv (sum of |terms| of each output); leak (per output, see the docstring)."""
    q, k, v, do, scale = c["q"], c["k"], c["v"], c["do"], c["scale"]
    P = ideal_p(c, rounded)
    I, N, hd = q.shape
    ks = 1.0 / (1.0 - p)
    r = {n: torch.empty(I, N, hd, dtype=F64) for n in ("out", "dq", "dk", "dv", "terms_out", "terms_dq", "terms_dk", "terms_dv", "gross_dq", "gross_dk")}
    r.update(lse=torch.empty(I, N, dtype=F64), delta=torch.empty(I, N, dtype=F64), ds_exact=True, sums_exact=True)
    leak = dict(out=0.0, dq=0.0, dk=0.0, dv=0.0)
    for lo in range(0, I, CHUNK):
        sl = slice(lo, lo + CHUNK)
        kk = keep[sl].to(F64) * ks if keep is not None else torch.ones(1, dtype=F64)
        s = scale * (q[sl] @ k[sl].transpose(1, 2))
        if c.get("term") is not None:
            s = s + c["term"][sl]
        pm = P[sl] * kk
        # the forward sums the un-normalised exp (1 on the ideal keys) times keep / (1 - p), then divides by l = their number
        unn = (c["sel"][sl].to(F64) if c["sel"] is not None else torch.ones(N, N, dtype=F64).expand(s.shape)) * kk
        out = (unn @ v[sl]) / (float(N) if c["sel"] is None else c["sel"][sl].sum(-1, keepdim=True).to(F64))
        dp = do[sl] @ v[sl].transpose(1, 2)
        delta = (do[sl] * out).sum(-1)
        x = dp * kk - delta[..., None]
        ds0 = P[sl] * x
        ds = ds0 * scale
        r["out"][sl], r["delta"][sl], r["lse"][sl] = out, delta, torch.logsumexp(s, -1)
        r["dq"][sl], r["dk"][sl], r["dv"][sl] = ds @ k[sl], ds.transpose(1, 2) @ q[sl], pm.transpose(1, 2) @ do[sl]
        r["terms_dq"][sl], r["terms_dk"][sl] = ds.abs() @ k[sl].abs(), ds.abs().transpose(1, 2) @ q[sl].abs()
        r["terms_dv"][sl] = pm.transpose(1, 2) @ do[sl].abs()
        r["terms_out"][sl] = (unn @ v[sl].abs()) / (float(N) if c["sel"] is None else c["sel"][sl].sum(-1, keepdim=True).to(F64))
        gross = P[sl] * (dp.abs() * kk + delta.abs()[..., None]) * scale              # |dS| without the cancellation in dP - delta
        r["gross_dq"][sl], r["gross_dk"][sl] = gross @ k[sl].abs(), gross.transpose(1, 2) @ q[sl].abs()
        if c["sel"] is not None:
            # fp32 sums of the kernels: products of integers and of P in {1, 1/2}, keep / (1 - p) in {0, 1, 2}
            r["sums_exact"] &= all(_sum_exact(a, b) for a, b in ((unn, v[sl]), (do[sl], v[sl].transpose(1, 2)), (ds0, k[sl]),
                                                                 (ds0.transpose(1, 2), q[sl]), (pm.transpose(1, 2), do[sl])))
            r["sums_exact"] &= _sum_exact(do[sl], rb(out).transpose(1, 2))
            r["ds_exact"] &= bool((rb(ds0) == ds0).all()) and bool((rb(pm) == pm).all())
            if c["pow2"]:
                r["ds_exact"] &= bool((rb(ds) == ds).all())
            pt = torch.softmax(s, -1)
            raw = torch.where(c["sel"][sl], torch.zeros_like(pt), pt)
            off = raw * kk
            l_out = off @ v[sl].abs()
            d_delta = (do[sl].abs() * l_out).sum(-1, keepdim=True)
            e = (raw * (dp.abs() * kk + delta.abs()[..., None] + d_delta) + P[sl] * d_delta) * scale   # a dropped key still has -P delta
            for name, val in (("out", l_out), ("dq", e @ k[sl].abs()), ("dk", e.transpose(1, 2) @ q[sl].abs()),
                              ("dv", off.transpose(1, 2) @ do[sl].abs())):
                leak[name] = max(leak[name], 2.0 * float(val.max()))            # x 2: the bf16 and fp32 roundings on the way
            if c.get("table_terms"):
                r.setdefault("g", torch.empty(I, N, N, dtype=F64))[sl] = ds0
                r.setdefault("g_leak", torch.empty(I, N, N, dtype=F64))[sl] = 2.0 * e / scale
        else:
            r["sums_exact"] &= _sum_exact(unn, v[sl]) and _sum_exact(do[sl], v[sl].transpose(1, 2)) and (not rounded or _sum_exact(pm.transpose(1, 2), do[sl]))
            r["sums_exact"] &= _sum_exact(do[sl], rb(out).transpose(1, 2))
    r["leak"] = leak
    return r


def _unit(t):
    """The largest power of two (at most 1) every entry is a multiple of."""
    u = 1.0
    while not bool((t / u == torch.round(t / u)).all()):
        u /= 2.0
        assert u > 2.0 ** -40, "not dyadic"
    return u


def _sum_exact(a, b):
    """Whether sum_k a[.., i, k] b[.., k, j] is exact in fp32 in every order: all products are integers times one factor and even
    the sum of their magnitudes stays under 2^24 of it."""
    u = _unit(a) * _unit(b)
    return float((a.abs() @ b.abs()).max()) / u < 2.0 ** 24


def truth(c, keep=None, p=0.0):
    """Plain fp64 softmax attention and its autograd gradient, with the keep mask applied to the probabilities."""
    q, k, v = (c[n].clone().requires_grad_(True) for n in "qkv")
    s = c["scale"] * (q @ k.transpose(1, 2))
    if c.get("term") is not None:
        s = s + c["term"]
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep.to(F64) / (1.0 - p)
    out = pr @ v
    out.backward(c["do"])
    return dict(out=out.detach(), lse=torch.logsumexp(s.detach(), -1), dq=q.grad, dk=k.grad, dv=v.grad)


def lse_fp32_error(c):
    """Worst |error| against fp64 of the fp32 restatements of the kernels' lse = mx * scale + logf(l), mx the largest raw score.
    l as the kernels sum it: exp((s - mx) * scale), where the largest score contributes exactly 1 (attention.hip and
    attention_wide_stream.hip scale first and subtract after), and exp2(fma(s, c2, -fl(mx * c2))) with c2 = scale * log2(e)
    (attention_seq.hip, attention_long.hip, attention_wide.hip: the compiler contracts s * c2 - mc, so the largest score
    contributes 2^(mx c2 - fl(mx c2)), up to half an ulp of mx c2 away from 1).  The last step with and without a fused
    multiply-add."""
    sc32 = torch.tensor(c["scale"], dtype=torch.float32)
    c2 = sc32 * torch.tensor(1.4426950408889634, dtype=torch.float32)
    worst = 0.0
    for lo in range(0, c["q"].shape[0], CHUNK):
        raw = c["q"][lo:lo + CHUNK] @ c["k"][lo:lo + CHUNK].transpose(1, 2)           # integers: exact in fp32 too
        want = torch.logsumexp(c["scale"] * raw, -1)
        s32 = raw.to(torch.float32)
        mx = s32.amax(-1)
        mc = (mx * c2).to(F64)
        contracted = (raw * c2.to(F64) - mc[..., None]).to(torch.float32)              # one rounding: the fma
        for l in (torch.exp((s32 - mx[..., None]) * sc32).sum(-1), torch.exp2(contracted).sum(-1)):
            plain = mx * sc32 + torch.log(l)
            fused = (mx.to(F64) * c["scale"] + torch.log(l).to(F64)).to(torch.float32)
            worst = max(worst, float((plain.to(F64) - want).abs().max()), float((fused.to(F64) - want).abs().max()))
    return worst


def mfma_steps(N):
    """Accumulation steps behind one output element: 16- or 32-deep products over the sequence, and a few more."""
    return (N + 15) // 16 + 2


def allow(c, e, n):
    """What an element of output n whose expectation is zero may hold (a tensor like the output; 0 for the uniform design, whose
    sums are exact).  The leak -- and one fp32 ulp of sum |terms| per accumulation step.  Observed on an MI355X, not documented:
    where two terms cancel, x - x, with leak-sized addends beside them, the element came back as minus one fp32 ulp of x, never
    plus and never the leak, in every family (profiles/attn_exact/mfma_residues.txt records the counts, signs and sizes, and the
    GPU test prints them again as FIGURE lines).  That is what accumulators do that round an inexact sum x + tiny down instead
    of to nearest, and the CPU test restates the kernels that way (mm_down); no other cause was looked for.  Where the
    expectation is not zero the same error is 2^-23 of the terms against the 2^-10 that could change the bf16 result, which
    `proven` asserts element by element."""
    if c["sel"] is None:
        return torch.zeros_like(e[n])
    return e["leak"][n] + mfma_steps(c["N"]) * 2.0 ** -23 * e["terms_" + n]


def proven(c, e, p=0.0):
    """The margins behind "bit for bit", asserted on the inputs at hand (one-hot and ties; the CPU test and the GPU test both
    call this): every exact expectation survives bf16, the leak is under 2^-12 of the smallest non-zero value, and leak plus
    accumulation error stay under 2^-10 of every non-zero element (half a bf16 step just above a power of two)."""
    assert c["sel"] is not None and e["sums_exact"] and e["ds_exact"], (p, e["sums_exact"], e["ds_exact"])
    for n in ["out", "dv"] + (["dq", "dk"] if c["pow2"] else []):
        assert torch.equal(rb(e[n]), e[n]), (n, p)
        nz = e[n] != 0
        if bool(nz.any()):
            assert e["leak"][n] <= 2.0 ** -12 * float(e[n][nz].abs().min()), (n, p, e["leak"][n])
            assert bool((allow(c, e, n) <= 2.0 ** -10 * e[n].abs())[nz].all()), (n, p)


def eps_exp2(e):
    """Relative error of the backward's P = exp2(s c2 - lse log2 e) in fp32: four roundings at the size of lse, two ulp of exp2."""
    return 4 * 2.0 ** -24 * max(1.0, float(e["lse"].abs().max())) + 2.0 ** -22


def colsum_tolerance(c, e, unrounded_dq):
    """What the fp32 column sums of a ties case may differ by from the fp64 sums of the dqkv the same call stored, [3 D].
    Sums built from rounded values -- MFMA accumulators of bf16 P and dS, or a pass over the stored bf16 dqkv -- are exact up to
    what `allow` grants the rows (x 2: the sum and the stored value each carry it).  unrounded_dq: the Q third of
    attn_seq_bwd_fused_kernel with in-kernel sums, scale sum_k (sum_q dS[q, k]) K[k, :] with dS summed BEFORE it is rounded to
    bf16 (ksum += dr in attention_bwd_fused.hip): P = 1/2 (1 + eps) there, so that third is off by eps sum |terms|."""
    B, H, N, hd = c["B"], c["H"], c["N"], c["hd"]
    un = lambda t: t.reshape(B, H, N, hd).sum((0, 2)).reshape(H * hd)                      # noqa: E731
    tol = [2.0 * un(allow(c, e, n)) for n in ("dq", "dk", "dv")]
    if unrounded_dq:
        tol[0] = tol[0] + eps_exp2(e) * un(e["terms_dq"])
    return torch.cat(tol)


def off(got, want, allowed):
    """Elements that are neither the expected bits nor, where zero is expected, within what `allow` grants."""
    got, want = got.to(F64), want.to(F64)
    return (got != want) & ~((want == 0) & (got.abs() <= allowed))


def wrong(got, want, allowed):
    return int(off(got, want, allowed).sum())


def rounding_bound(got, want, terms):
    """The allowance of test_attention_backward_against_fp32_math_with_the_kernel_roundings: one bf16 step of the result plus
    every P / dS of the sum one bf16 step off."""
    return 2.0 ** -7 * torch.maximum(got.abs(), want.abs()) + 2.0 ** -8 * terms + 1e-6


def mutate(c, kind, j):
    """The fp64 (lse, out) of the same inputs with key j dropped ("drop"), counted twice ("twice"), or with one padding key of
    score 0 and value 0 appended ("pad"; j unused)."""
    q, k, v = c["q"], c["k"], c["v"]
    N = c["N"]
    if kind == "drop":
        idx = [i for i in range(N) if i != j]
    elif kind == "twice":
        idx = list(range(N)) + [j]
    else:
        idx = list(range(N))
    k2, v2 = k[:, idx], v[:, idx]
    if kind == "pad":
        k2 = torch.cat([k2, torch.zeros_like(k2[:, :1])], 1)
        v2 = torch.cat([v2, torch.zeros_like(v2[:, :1])], 1)
    s = c["scale"] * (q @ k2.transpose(1, 2))
    return torch.logsumexp(s, -1), torch.softmax(s, -1) @ v2


# ---- the cases of tests/test_attention_exact_gpu.py -----------------------------------------------------------------------------
LDS_LIMIT, SEQ_MAX_N, FUSED_MAX_N, LONG_MAX_N = 160 * 1024, 256, 224, 608


def wide_fits(hd, N, bwd):
    """csrc/dispatch.h, wide_lds: the Q | K (K | V) images of the padded sequence, + lse / delta / row key in the dK / dV kernel."""
    npad = (N + 31) // 32 * 32
    return N <= SEQ_MAX_N and 2 * (hd // 64) * npad * 128 + (3 * npad * 4 if bwd else 0) <= LDS_LIMIT


def wide_max_n(hd, bwd):
    return max(n for n in range(1, SEQ_MAX_N + 1) if wide_fits(hd, n, bwd))


def symbols(hd, N, p, env, any_length):
    """(forward symbol, backward symbol or None where the backward is refused) of one call, as csrc/dispatch.cpp plans it."""
    drop = "true" if p > 0 else "false"
    if hd != 64:
        S = hd // 64
        stream = any_length and env.get("SFCVIT_ATTN_WIDE_STREAM") == "1"
        fwd = "attn_wide_fwd_kernel<%d>" % S if wide_fits(hd, N, False) and not stream else "attn_wide_stream_fwd_kernel<%d>" % S
        if wide_fits(hd, N, True) and not stream:
            return fwd, "attn_wide_bwd_kv_kernel<%d>" % S
        return fwd, "attn_wide_stream_bwd_kv_kernel<%d>" % S if any_length else None
    inst = 13 if (N + 15) // 16 == 13 else 0
    long_ok = env.get("SFCVIT_ATTN_LONG") != "0" and SEQ_MAX_N < N <= LONG_MAX_N
    if N <= SEQ_MAX_N:
        fwd = "attn_seq_fwd_kernel<%d, %s>" % (inst, drop)
    elif long_ok:
        fwd = "attn_long_fwd_kernel<%d>" % (36 if (N + 31) // 32 * 32 == 576 else 0)
    else:
        fwd = "attn_fwd_kernel"
    if N <= FUSED_MAX_N and env.get("SFCVIT_ATTN_BWD_FUSED") != "0":
        bwd = "attn_seq_bwd_fused_kernel<%d, %s>" % (inst, drop)
    elif long_ok:
        bwd = "attn_long_bwd_kv_kernel"
    elif N <= SEQ_MAX_N:
        bwd = "attn_seq_bwd_kv_kernel<%d>" % inst
    else:
        bwd = "attn_bwd_kv_kernel"
    return fwd, bwd


def _cases():
    """(id, family, hd, N, scale or None, environment, any_length, lengths-with-dropout flag)."""
    out = []
    add = lambda fam, hd, N, scale=None, env=None, any_length=False, drop=False: out.append(      # noqa: E731
        dict(family=fam, hd=hd, N=N, scale=scale, env=env or {}, any_length=any_length, drop=drop))
    for N in (1, 5, 16, 17, 33, 70, 193, 196, 208, 209, 224):    # seq forward <0> / <13>, one-pass backward <0> / <13>
        add("seq + fused", 64, N, drop=N in (5, 70, 196, 208, 224))
    for N in (225, 256):                                         # above FUSED_MAX_N: the two-kernel backward by default
        add("seq + seq kv", 64, N, drop=True)
    for N in (5, 64, 70, 196):                                   # 64: a whole length for the dropout pair
        add("seq kv, SFCVIT_ATTN_BWD_FUSED=0", 64, N, env={"SFCVIT_ATTN_BWD_FUSED": "0"}, drop=N != 70)
    for N in (5, 70, 196, 209, 224):
        add("fused, SFCVIT_ATTN_BWD_PERSIST=0", 64, N, env={"SFCVIT_ATTN_BWD_PERSIST": "0"}, drop=N in (5, 196, 224))
        add("fused, SFCVIT_ATTN_DQSUM=pass", 64, N, env={"SFCVIT_ATTN_DQSUM": "pass"}, drop=N in (5, 196, 224))
    for N in (257, 300, 576, 577, 608):
        add("long", 64, N, drop=N in (300, 576))
    for N in (609, 640):                                         # 640: a whole length for the dropout pair
        add("tiled", 64, N, drop=True)
    for N in (257, 320):
        add("tiled, SFCVIT_ATTN_LONG=0", 64, N, env={"SFCVIT_ATTN_LONG": "0"}, drop=True)
    for hd, scale in ((128, 2.0 ** -3), (192, 2.0 ** -4), (256, None)):
        top = wide_max_n(hd, True)
        for N in sorted({n for n in (1, 5, 100, 180) if wide_fits(hd, n, True)} | {top}):
            add("wide", hd, N, scale=scale, drop=N in (5, top))
        if wide_max_n(hd, False) > top:                          # the forward alone fits longer sequences (hd 256: 160 against 128)
            add("wide, forward only", hd, wide_max_n(hd, False), scale=scale)
    for hd in (128, 192):                                        # 1 / sqrt(hd) is no power of two: one bf16 step on dQ and dK
        add("wide, default scale", hd, 100)
    add("stream", 128, 257, scale=2.0 ** -3, any_length=True, drop=True)
    add("stream", 256, 161, any_length=True, drop=True)
    add("stream, default scale", 128, 257, any_length=True)
    for hd, scale in ((128, 2.0 ** -3), (256, None)):
        for N in (1, 5, 64, 70):                                 # 64: a whole length for the dropout pair
            add("stream, SFCVIT_ATTN_WIDE_STREAM=1", hd, N, scale=scale, env={"SFCVIT_ATTN_WIDE_STREAM": "1"}, any_length=True, drop=N in (5, 64))
    return out


CASES = _cases()
DESIGNS = ("uniform", "onehot", "ties")
DROP_P = 0.5
MANY_ITEMS = ((33, (1, 2, 3)), (196, (1, 2, 3)), (224, (3,)))    # N, which of B = cus + 1, 2 cus, 2 cus + 37
MAX_ITEMS = 2048


def many_items_b(cus, which):
    return {1: cus + 1, 2: 2 * cus, 3: 2 * cus + 37}[which]


def case_id(c):
    return "%s-hd%d-N%d" % (c["family"].replace(", ", "-").replace(" ", "_"), c["hd"], c["N"])


def shape_of(c):
    """B, H of a case: 2, 2, and one head at head dims 192 and 256."""
    return 2, (1 if c["hd"] >= 192 else 2)


def lse_bar(built):
    """uniform: 1e-5 against log N; one-hot and ties: 4 x the fp32 restatement's worst error on the same inputs."""
    return 1e-5 if built["design"] == "uniform" else 4.0 * lse_fp32_error(built)
