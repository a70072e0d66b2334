"""Reference, exact designs and error bar for the fused clip + AdamW step (csrc/optim.hip: adamw_one, adamw_kernel,
adamw_ema_kernel, step_advance_kernel).  Used by tests/test_adamw_ref_cpu.py (which qualifies all of it without a GPU) and
tests/test_adamw_edges_gpu.py.

The step, as the kernel defines it (every hyperparameter is the float32 value the kernel receives):

    gmul  = grad_scale * min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6))        (grad_scale alone without sumsq)
    g     = bf16 gradient * gmul
    w1    = w * (1 - lr * wd)
    m'    = beta1 * m + (1 - beta1) * g
    v'    = beta2 * v + (1 - beta2) * g * g
    D     = sqrt(v') * rbc2 + eps
    w'    = w1 - (lr / bc1) * (m' / D)
    param = bf16(w'), round to nearest even

bc1 = 1 - beta1^t and rbc2 = 1 / sqrt(1 - beta2^t) are INPUTS of `step64` / `step32`.  On the host path the reference gets
them in float64 from the float32 betas and the bar carries the error of the launcher's float32 evaluation (below); on the
dev_state path they, and lr, are the three floats the test reads back from the state buffer: the kernel's inputs there.

`step64`    the step in float64 (numpy arrays, or torch tensors for the one size that is compared on the device).
`step32`    the step restated in numpy float32 in the kernel's order of operations.  contract=False rounds every multiply
            and every add; contract=True rounds a multiply feeding an add once, fusing what LLVM's combiner fuses under
            -ffp-contract=fast: in a sum of two products the LEFT one -- fma(beta1, m, fl((1 - beta1) g)), and, since
            w1 - U is the sum w * decay - c * q, fma(decay, w, -fl(c q)); contract="right" fuses the other product of
            those three sums instead.  A dict chooses per site (SITES; `all_contractions` lists all 216 combinations).  A
            fused multiply-add is emulated as the float64 product (exact: 24 x 24 bits) plus the addend in float64, rounded
            once to float32.
`bar`       the bound below.

The bar (derived, not tuned).  u = 2^-24: an fp32 operation in round-to-nearest is off by at most u times the magnitude
of its result, or by 2^-150 (half the subnormal spacing) where the result is subnormal; `f` below stands for that floor.
sqrtf and the fp32 division are correctly rounded (one rounding each).  Errors are carried to first order, except through
the square root, where the bound is rigorous (v' may be as small as its own error).

    gmul    with sumsq: sqrt, * grad_scale, + 1e-6, the division, * grad_scale: 5 roundings, min() is 1-Lipschitz: 5 u
            relative.  Without sumsq it is an input.  g = gradient * gmul: one more.  So  |dg| <= eg u |g|,  eg = 6 or 1.
    m'      A = beta1 m: 1 rounding.  B = (1 - beta1) g: the subtraction, the product, g's eg.  The sum: u |m'| <= u (|A| + |B|).
            |dm| <= u (2 |A| + (3 + eg) |B|) + 4 f
    v'      A = beta2 v: 1.  B = ((1 - beta2) g) g: the subtraction, two products, g twice.  The sum as above.
            |dv| <= u (2 |A| + (4 + 2 eg) |B|) + 5 f
    s       = sqrt(v'):  |sqrt(v' + d) - sqrt(v')| = |d| / (sqrt(v' + d) + sqrt(v')) <= dv / (sqrt(v') + sqrt(max(v' - dv, 0)))
            (sqrt(dv) where that denominator is 0), plus the rounding u s.
    D       = s rbc2 + eps:  dD <= rbc2 ds + s rbc2 (u + r_r) + u D      (product, r_r = relative error of rbc2, sum)
    q       = m' / D:        dq <= dm / D + |q| dD / D + u |q| + f
    U       = c q, c = lr / bc1 with relative error r_c = u + r_1:   dU <= c dq + |U| (r_c + u) + f
    w1      = w (1 - lr wd): lr wd is off by u lr wd, the subtraction by u, the product by u:  dw1 <= u (2 + lr wd) |w1| + f
    w'      = w1 - U:        dw <= dw1 + dU + u (|w1| + |U|) + f

With a multiply and an add contracted into one FMA there is one rounding fewer, so the bound holds for every contraction.

The margin.  The counted bound is nearly attained (the clip's five roundings are common to all elements, and among a few
thousand elements some round the same way in every remaining step: the float32 restatement reaches 0.94 of it).  `bar`
returns MARGIN = 2 times the counted bound: tests/test_adamw_ref_cpu.py holds the restatement, in every contraction variant,
to half the bar, i.e. to the counted bound itself, and the other half is left to the device for what numpy cannot restate:
which multiply-adds it fuses, and a sqrtf or division that is not the correctly rounded one.  The factor is not fitted to
any kernel output.

On the dev_state path r_1 = r_r = 0.  On the host path the launcher evaluates bc = 1.f - powf(beta, t) in float32
(`host_rho`): the subtraction rounds once (u bc), powf is off by P ulp of beta^t <= 2 P u beta^t -- the GNU C library manual's
table of known maximum errors lists powf at 1 ulp, P = 1 -- and both are divided by the bc they feed:
r = u + 2 P u beta^t / bc.  At t = 1, beta2 = 0.999 that is 2000 u = 1.2e-4: the cancellation the issue speaks of, and it is
the launcher's, not the kernel's.  r_1 = r(beta1); rbc2 = 1.f / sqrtf(bc2) adds a square root and a division:
r_r = r(beta2) / 2 (1 + r(beta2)) + 2 u.

The EMA in the same kernel, e' = e + omd (w' - e), is held to model_ema_ref's bar for one update, plus the error of w'
that enters it multiplied by omd <= 1:  6 u max(|w'|, |e|) + dw.

param is held to the bf16 rounding of the kernel's own stored master bit for bit, and to the bf16 rounding of the
reference master wherever [w' - dw, w' + dw] rounds to one bf16 value (`bf16_unambiguous`).

step_advance (`advance_ref`, `advance_bar`): counter + 1, seed offset mix32(seed_base ^ step * 0x9E3779B1) in uint32, and
    state[3] = 1 - beta1^t:           the subtraction (u bc1) + P_dev ulp of beta1^t (2 P_dev u beta1^t)
    state[4] = 1 / sqrt(1 - beta2^t): relative ((u bc2 + 2 P_dev u beta2^t) / bc2) / 2 (1 + that), + u (sqrt) + u (reciprocal)
P_dev is the device powf's error.  The ROCm installation this was written against documents no bound for it, so
DEVICE_POWF_ULPS is the OpenCL full-profile bound for pow, 16 ulp; the GPU test prints the observed error.

Exact designs (`design`): inputs on which every operation of the step is exact in fp32, fused or not, so the answer is
known bit for bit and a dropped, doubled or misplaced element changes it.
    "first"      m = v = 0, beta1 = 0.5, beta2 = 0.75, eps = 0, step 1 on the host path (bc1 = 0.5, rbc2 = 2; powf(x, 1) = x),
                 lr = 2^-3, wd = 2^-2 (decay factor 31/32).  w_i = 32 j_i 2^-10 with j_i a hash of i in +-1023,
                 g_i = +- k_i 2^e_i with k_i in 1..7, e_i in -8..8.  Then m' = g / 2, v' = g^2 / 4, D = |g|, q = sign(g) / 2,
                 c = 2^-2:  w' = 31 j 2^-10 - 2^-3 sign(g).  Planted: w = 0, and w = +-32 j 2^-11 that make w' an odd 9-bit
                 integer times 2^-11, a bf16 tie, rounding up and rounding down.
    "running"    through dev_state = (lr 2^-4, bc1 0.5, rbc2 2.0), beta1 = 0.5, beta2 = 0.75, eps = 0, wd = 0.5 (31/32 again).
                 s_i = k_i 2^e_i (k in 1..15, e in -6..6), v = s^2, g = +-s, m = a s with a in -4..4.  Then v' = s^2,
                 m' = (a +- 1) s / 2, D = 2 s, q = (a +- 1) / 4, c = 2^-3:  w' = 31 j 2^-10 - (a +- 1) 2^-5.
    "running-clip"  the same with the gradient doubled, grad_scale = 0.5, sumsq = 4, max_norm = 4: the norm is 1, the
                 coefficient fminf(1, 4 / (1 + 1e-6)) must be exactly 1 and gmul 0.5.
For adamw_ema_step the average starts at e = 0 with decay 0.5: e' = 0 + 0.5 (w' - 0) = w' / 2 exactly."""
import functools

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -150
MARGIN = 2.0                  # bar = MARGIN x the counted bound (module docstring, "The margin")
HOST_POWF_ULPS = 1.0          # the GNU C library manual, "Known Maximum Errors in Math Functions": powf 1 ulp
DEVICE_POWF_ULPS = 16.0       # OpenCL full profile, pow: <= 16 ulp (no bound documented for the ROCm device library's powf)
F32 = np.float32


def f32(x):
    """The float32 the kernel receives for a Python float, widened to float64."""
    return float(F32(x))


# ---- bf16 -------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """Round-to-nearest-even bf16 bit patterns (uint16) of a float32 array; NaN stays NaN (quiet, sign kept)."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, ((b >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def bf16_round(x):
    """The float32 values of bf16_bits(x)."""
    return (bf16_bits(x).astype(np.uint32) << np.uint32(16)).view(F32)


def bf16_unambiguous(w, dw):
    """Where every value of [w - dw, w + dw] (float64) rounds to the same bf16 value."""
    with np.errstate(over="ignore", invalid="ignore"):
        return bf16_bits((w - dw).astype(F32)) == bf16_bits((w + dw).astype(F32))


# ---- the step in float64 ------------------------------------------------------------------------------------------------------
def _xp(x):
    if isinstance(x, np.ndarray):
        return np
    import torch
    return torch


def _f64(x):
    if isinstance(x, np.ndarray):
        return x.astype(np.float64)
    return x.double()


def gmul64(grad_scale, max_norm, sumsq):
    gs = f32(grad_scale)
    if sumsq is None:
        return gs
    return gs * min(1.0, f32(max_norm) / (float(np.sqrt(np.float64(f32(sumsq)))) * gs + f32(1e-6)))


def step64(w, m, v, g, *, lr, beta1, beta2, eps, weight_decay, bc1, rbc2, grad_scale=1.0, max_norm=0.0, sumsq=None):
    """One clip + AdamW step in float64 on numpy arrays or torch tensors.  -> (w', m', v', terms); terms holds the
    intermediate magnitudes `bar` needs, among them the sum of the absolute values of each output's terms (S_w, S_m, S_v)."""
    xp = _xp(w)
    w, m, v, g = _f64(w), _f64(m), _f64(v), _f64(g)
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, beta1, beta2, eps, weight_decay))
    bc1, rbc2 = float(bc1), float(rbc2)
    gh = g * gmul64(grad_scale, max_norm, sumsq)
    w1 = w * (1.0 - lr * wd)
    ma, mb = b1 * m, (1.0 - b1) * gh
    va, vb = b2 * v, (1.0 - b2) * gh * gh
    m2, v2 = ma + mb, va + vb
    s = xp.sqrt(v2)
    D = s * rbc2 + eps
    c = lr / bc1
    q = m2 / D
    Uu = c * q
    w2 = w1 - Uu
    terms = dict(ma=abs(ma), mb=abs(mb), va=abs(va), vb=abs(vb), v=v2, s=s, D=D, q=abs(q), c=c, U=abs(Uu), w1=abs(w1), rbc2=rbc2,
                 lrwd=lr * wd, S_m=abs(ma) + abs(mb), S_v=abs(va) + abs(vb), S_w=abs(w1) + abs(Uu))
    return w2, m2, v2, terms


def host_bc(beta1, beta2, t):
    """The host path's reference corrections: float64 of the float32 betas.  -> (bc1, rbc2)"""
    return 1.0 - f32(beta1) ** t, 1.0 / float(np.sqrt(1.0 - f32(beta2) ** t))


def _rho(beta, t, ulps):
    bt = f32(beta) ** t
    return U + 2.0 * ulps * U * bt / (1.0 - bt)


def host_rho(beta1, beta2, t, ulps=HOST_POWF_ULPS):
    """Relative error of the launcher's float32 bc1 and rbc2 against host_bc (module docstring).  -> (r_1, r_r)"""
    r2 = _rho(beta2, t, ulps)
    return _rho(beta1, t, ulps), 0.5 * r2 * (1.0 + r2) + 2.0 * U


def bar(terms, *, clip, rho_bc1=0.0, rho_rbc2=0.0):
    """(bar_w, bar_m, bar_v) of the module docstring from step64's terms; clip = a sumsq was given."""
    t = terms
    xp = _xp(t["s"])
    eg = 6.0 if clip else 1.0
    dm = U * (2.0 * t["ma"] + (3.0 + eg) * t["mb"]) + 4 * FLOOR
    dv = U * (2.0 * t["va"] + (4.0 + 2.0 * eg) * t["vb"]) + 5 * FLOOR
    lo = xp.sqrt((t["v"] - dv).clip(min=0.0))
    den = t["s"] + lo
    ds = xp.where(den > 0, dv / xp.where(den > 0, den, den + 1.0), xp.sqrt(dv)) + U * t["s"]
    dD = t["rbc2"] * ds + t["s"] * t["rbc2"] * (U + rho_rbc2) + U * t["D"]
    dq = dm / t["D"] + t["q"] * dD / t["D"] + U * t["q"] + FLOOR
    dU = t["c"] * dq + t["U"] * (U + rho_bc1 + U) + FLOOR
    dw1 = U * (2.0 + t["lrwd"]) * t["w1"] + FLOOR
    dw = dw1 + dU + U * (t["w1"] + t["U"]) + FLOOR
    return MARGIN * dw, MARGIN * dm, MARGIN * dv


def ema_bar(w2, e, dw):
    """One update e' = e + omd (w' - e): model_ema_ref's three roundings of quantities <= 2 max(|w'|, |e|), plus dw."""
    xp = _xp(w2)
    return 6.0 * U * xp.maximum(abs(w2), abs(_f64(e))) + dw


# ---- the step restated in float32 -----------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl(a * b + c) with one rounding (float64 product of float32 factors is exact)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


MUTANTS = ("bc_prev_step", "eps_in_sqrt", "decay_after", "decay_on_update", "no_omb1", "no_omb2", "v_unscaled", "clip_sumsq",
           "scale_grad_only", "rbc2_sqrt")


SITES = dict(norm=(0, 1), decay=(0, 1), m=(0, "left", "right"), v=(0, "left", "right"), denom=(0, 1), update=(0, "left", "right"))


def contraction(contract):
    """False / True / "right" / a dict of SITES -> the choice at every site.  True is what LLVM's combiner does under
    -ffp-contract=fast: every product feeding an add is fused, and of two products feeding one add the LEFT one."""
    if isinstance(contract, dict):
        return dict({k: 0 for k in SITES}, **contract)
    if not contract:
        return {k: 0 for k in SITES}
    side = "right" if contract == "right" else "left"
    return dict(norm=1, decay=1, m=side, v=side, denom=1, update=side)


def all_contractions():
    """Every combination of the choices of SITES (216)."""
    import itertools
    keys = list(SITES)
    return [dict(zip(keys, c)) for c in itertools.product(*(SITES[k] for k in keys))]


def step32(w, m, v, g, *, lr, beta1, beta2, eps, weight_decay, bc1, rbc2, grad_scale=1.0, max_norm=0.0, sumsq=None,
           contract=False, mutant=None, bc_prev=None):
    """The kernel's arithmetic in numpy float32, operation by operation (adamw_kernel's gmul lines and adamw_one).
    contract: False / True / "right" (module docstring) or a dict of SITES.  mutant: one of MUTANTS, a deliberate error for
    the CPU tests (bc_prev = the (bc1, rbc2) of step t - 1 for "bc_prev_step").  -> (w', m', v') float32."""
    assert mutant is None or mutant in MUTANTS, mutant
    on = contraction(contract)
    w, m, v, g = (np.asarray(x, dtype=F32) for x in (w, m, v, g))
    lr, b1, b2, eps, wd, gs, mn = (F32(x) for x in (lr, beta1, beta2, eps, weight_decay, grad_scale, max_norm))
    bc1, rbc2 = F32(bc1), F32(rbc2)
    if mutant == "bc_prev_step":
        bc1, rbc2 = F32(bc_prev[0]), F32(bc_prev[1])
    if mutant == "rbc2_sqrt":
        rbc2 = F32(1.0) / rbc2
    one = F32(1.0)

    def mul(a, b):
        return (a * b).astype(F32)

    def mad(fuse, a, b, c):                             # a * b + c
        return _fma(a, b, c) if fuse else (mul(a, b) + c).astype(F32)

    def two(side, a, b, c, d):                          # a * b + c * d
        if side == "left":
            return _fma(a, b, mul(c, d))
        if side == "right":
            return _fma(c, d, mul(a, b))
        return (mul(a, b) + mul(c, d)).astype(F32)

    with np.errstate(all="ignore"):
        gmul = gs
        if sumsq is not None:
            root = F32(sumsq) if mutant == "clip_sumsq" else np.sqrt(F32(sumsq))
            norm = F32(root + F32(1e-6)) if mutant == "scale_grad_only" else F32(mad(on["norm"], root, gs, F32(1e-6)))
            gmul = F32(gs * np.minimum(one, F32(mn / norm)))
        gr = mul(g, gmul)
        decay = F32(mad(on["decay"], -lr, wd, one))
        omb1 = one if mutant == "no_omb1" else F32(one - b1)
        omb2 = one if mutant == "no_omb2" else F32(one - b2)
        gv = g if mutant == "v_unscaled" else gr
        m2 = two(on["m"], b1, m, omb1, gr)
        v2 = two(on["v"], b2, v, mul(omb2, gv), gv)
        if mutant == "eps_in_sqrt":
            denom = mul(np.sqrt((v2 + eps).astype(F32)), rbc2)
        else:
            denom = mad(on["denom"], np.sqrt(v2), rbc2, eps)
        c = F32(lr / bc1)
        q = (m2 / denom).astype(F32)
        if mutant == "decay_on_update":
            w2 = mad(on["update"], -c, mul(q, decay), w)
        elif mutant == "decay_after":
            w2 = mul(mad(on["update"], -c, q, w), decay)
        else:
            w2 = two(on["update"], decay, w, -c, q)     # w * decay - c * q
    return w2.astype(F32), m2.astype(F32), v2.astype(F32)


def ema32(e, w2, decay, contract=False):
    """e + omd * (w' - e) in float32 (no warm-up): adamw_ema_kernel's update."""
    e, w2 = np.asarray(e, dtype=F32), np.asarray(w2, dtype=F32)
    omd = F32(F32(1.0) - F32(decay))
    d = (w2 - e).astype(F32)
    return _fma(omd, d, e) if contract else ((omd * d).astype(F32) + e).astype(F32)


# ---- step_advance ---------------------------------------------------------------------------------------------------------------
def mix32(x):
    """device_common.h's mix32 in numpy uint32."""
    x = np.asarray(x, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x85EBCA6B)
        x = x ^ (x >> np.uint32(13))
        x = x * np.uint32(0xC2B2AE35)
        x = x ^ (x >> np.uint32(16))
    return x


def advance_ref(step_before, beta1, beta2, seed_base):
    """What step_advance leaves from a counter of `step_before`.  -> (step, seed offset uint32, bc1 float64, rbc2 float64)"""
    step = step_before + 1
    with np.errstate(over="ignore"):
        off = int(mix32(np.uint32(seed_base & 0xFFFFFFFF) ^ (np.uint32(step) * np.uint32(0x9E3779B1))))
    bc1, rbc2 = host_bc(beta1, beta2, step)
    return step, off, bc1, rbc2


def advance_bar(beta1, beta2, step, ulps=DEVICE_POWF_ULPS):
    """(absolute bar on state[3], absolute bar on state[4]) of the module docstring."""
    bc1, rbc2 = host_bc(beta1, beta2, step)
    r2 = _rho(beta2, step, ulps)
    return _rho(beta1, step, ulps) * bc1, (0.5 * r2 * (1.0 + r2) + 2.0 * U) * rbc2


def advance32(beta1, beta2, step):
    """The two corrections in numpy float32, as the kernel writes them (the launcher's host-path formula is the same)."""
    return kernel_bc32(beta1, beta2, step)


def powf_ulps(got_bc, beta, step):
    """The device powf's error in ulps of beta^t, read back from a stored 1 - powf(beta, t).  Only while that subtraction
    is exact (beta^t >= 0.5, Sterbenz); NaN otherwise, where the subtraction's own rounding would be in the figure."""
    bt = f32(beta) ** step
    if bt < 0.5:
        return float("nan")
    ulp = 2.0 ** (np.floor(np.log2(bt)) - 23)
    return abs((1.0 - float(got_bc)) - bt) / ulp


# ---- exact designs --------------------------------------------------------------------------------------------------------------
def _h(i, salt):
    with np.errstate(over="ignore"):
        return mix32(i.astype(np.uint32) * np.uint32(0x9E3779B1) + np.uint32(salt))


# planted in "first": (j, sign of g, sign of w); w = sw * 32 j 2^-11, w' = sw (31 j - sg sw 256) 2^-11
_TIES = [(17, +1, +1), (19, +1, +1), (21, +1, +1), (23, +1, +1), (1, -1, +1), (3, -1, +1), (17, -1, -1), (19, -1, -1), (5, +1, -1)]

DESIGNS = ("first", "running", "running-clip")


@functools.lru_cache(maxsize=4)
def design(name, n):
    """The exact design `name` at n elements.  -> dict: w, m, v, g (float32; g is a bf16 value), hyper (the keyword
    arguments of ops.adamw_step except dev_state), state (lr, bc1, rbc2 to write into the state buffer, or None), bc (the
    bc1, rbc2 the kernel sees), want = dict(w, m, v, ema) float32, and the planted tie positions.  Read-only; shared."""
    assert name in DESIGNS, name
    i = np.arange(n, dtype=np.int64)
    j = (_h(i, 1) % np.uint32(2047)).astype(np.int64) - 1023
    sign = np.where(_h(i, 2) & np.uint32(1 << 20), -1.0, 1.0)
    w = j.astype(np.float64) / 32.0                                          # 32 j 2^-10
    ties = []
    if name == "first":
        h = _h(i, 3)
        k = 1 + (h % np.uint32(7)).astype(np.int64)
        e = ((h >> np.uint32(8)) % np.uint32(17)).astype(np.int64) - 8
        g = sign * k * 2.0 ** e
        m, v = np.zeros(n), np.zeros(n)
        want_w = 31.0 * j * 2.0 ** -10 - 2.0 ** -3 * sign
        pos = list(range(1, 1 + len(_TIES))) + ([n - 2 - 2 * p for p in range(len(_TIES))] if n >= 64 else [])
        for p, (tj, sg, sw) in zip(pos, _TIES + _TIES):
            if p < n:
                w[p], g[p] = sw * 32.0 * tj * 2.0 ** -11, sg * abs(g[p])
                want_w[p] = sw * 31.0 * tj * 2.0 ** -11 - 2.0 ** -3 * sg
                ties.append(p)
        w[0] = 0.0
        want_w[0] = -2.0 ** -3 * np.sign(g[0])
        want_m, want_v = g / 2.0, g * g / 4.0
        hyper = dict(lr=2.0 ** -3, beta1=0.5, beta2=0.75, eps=0.0, weight_decay=2.0 ** -2, max_norm=0.0, step=1, grad_scale=1.0)
        state, sumsq = None, None
    else:
        h = _h(i, 4)
        k = 1 + (h % np.uint32(15)).astype(np.int64)
        e = ((h >> np.uint32(8)) % np.uint32(13)).astype(np.int64) - 6
        a = ((h >> np.uint32(16)) % np.uint32(9)).astype(np.int64) - 4
        s = k * 2.0 ** e
        m, v = a * s, s * s
        clip = name == "running-clip"
        g = sign * s * (2.0 if clip else 1.0)
        want_w = 31.0 * j * 2.0 ** -10 - (a + sign) * 2.0 ** -5
        want_m, want_v = (a + sign) * s / 2.0, s * s
        hyper = dict(lr=123.0, beta1=0.5, beta2=0.75, eps=0.0, weight_decay=0.5, max_norm=4.0 if clip else 0.0, step=7,
                     grad_scale=0.5 if clip else 1.0)                       # lr and step: the state's are what count
        state, sumsq = (2.0 ** -4, 0.5, 2.0), (4.0 if clip else None)
    out = dict(w=w, m=m, v=v, g=g, want=dict(w=want_w, m=want_m, v=want_v, ema=want_w / 2.0))
    for d in (out, out["want"]):
        for key in list(d):
            if isinstance(d[key], np.ndarray):
                x32 = d[key].astype(F32)
                assert np.array_equal(x32.astype(np.float64), d[key]), (name, key, "is not a float32 value")
                x32.setflags(write=False)
                d[key] = x32
    assert np.array_equal(bf16_round(out["g"]), out["g"]) and bool((out["g"] != 0).all()), "the gradient must be a non-zero bf16 value"
    out.update(hyper=hyper, state=state, sumsq=sumsq, bc=(0.5, 2.0), ties=ties, name=name, n=n)
    return out


def design_step_kwargs(d):
    """step64 / step32 keyword arguments of a design: the hyperparameters the kernel ends up using."""
    h = d["hyper"]
    return dict(lr=d["state"][0] if d["state"] else h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], weight_decay=h["weight_decay"],
                bc1=d["bc"][0], rbc2=d["bc"][1], grad_scale=h["grad_scale"], max_norm=h["max_norm"], sumsq=d["sumsq"])


# ---- what each size exercises ---------------------------------------------------------------------------------------------------
def walk(n, threads, cap):
    """The kernels' walk over n elements restated: -> dict(grid, tail, paired trips of lane 0, lanes with a remainder
    group, most groups any lane sees)."""
    nq, grid = n >> 2, min(cap, -(-(-(-n // 8)) // threads))
    stride = grid * threads
    full, extra = divmod(nq, stride)                      # every lane owns `full` groups, the first `extra` lanes one more
    rem_lanes = (extra if (full + 1) % 2 else 0) + (stride - extra if full % 2 else 0)
    most = full + (1 if extra else 0)
    return dict(grid=grid, tail=n & 3, trips0=most // 2, rem_lanes=rem_lanes, max_groups=most)


# ---- the random and edge cases of the fp64-bar tests ---------------------------------------------------------------------------
BETA1, BETA2, EPS, MAX_NORM = 0.9, 0.999, 1e-8, 1.0
# (first step t, clip, grad_scale, weight_decay, lr, step state on the device).  Crossed sparingly: every step, every clip
# mode, every grad_scale, both weight decays and both step states appear; the last case (lr 0.1, wd 0.5: a decay factor of
# 0.95) is the one on which the ORDER of decay and update is visible.
CASES = [
    (1, "binds", 1.0, 5e-2, 1e-3, False),
    (2, "loose", 0.5, 0.0, 1e-3, True),
    (10, None, 1.0 / 3.0, 5e-2, 1e-3, True),
    (1000, "binds", 0.5, 0.0, 1e-3, False),
    (1, None, 1.0, 5e-2, 1e-3, True),
    (1000, "loose", 1.0 / 3.0, 5e-2, 1e-3, False),
    (2, None, 1.0, 0.5, 0.1, True),
]
CASE_IDS = [f"t{t}-clip_{c}-gs{gs:.2f}-wd{wd:g}-lr{lr:g}-{'dev' if dev else 'host'}" for t, c, gs, wd, lr, dev in CASES]


def grad_sigma(clip, n):
    """Standard deviation of the random gradient: "binds" gives a norm far above MAX_NORM even at 7 elements and
    grad_scale 1/3, "loose" one of about 0.1."""
    return {"binds": 10.0, "loose": 0.1 / float(np.sqrt(n)), None: 3.0}[clip]


def random_state(n, seed):
    """w ~ N(0, 1); m ~ +-(1e-4 + |N(0, 1e-2)|), never zero; v = 10^U(-12, 0).  float32 numpy."""
    r = np.random.default_rng(seed)
    w = r.standard_normal(n).astype(F32)
    m = (np.where(r.random(n) < 0.5, -1.0, 1.0) * (1e-4 + np.abs(r.standard_normal(n)) * 1e-2)).astype(F32)
    v = (10.0 ** r.uniform(-12.0, 0.0, n)).astype(F32)
    return w, m, v


def random_grad(n, seed, clip):
    return bf16_round((np.random.default_rng(seed).standard_normal(n) * grad_sigma(clip, n)).astype(F32))


def kernel_bc32(beta1, beta2, t):
    """bc1 and rbc2 as the launcher (host path) computes them: float32 throughout.  numpy's float32 power stands in for the
    C library's powf; host_rho's allowance covers either."""
    b1t, b2t = np.power(F32(beta1), F32(t)), np.power(F32(beta2), F32(t))
    return F32(F32(1.0) - b1t), F32(F32(1.0) / np.sqrt(F32(F32(1.0) - b2t)))


EDGE_HYPER = dict(lr=1e-3, beta1=BETA1, beta2=BETA2, eps=EPS, weight_decay=5e-2)
EDGE_STEP = 3
EDGE_NAMES = ["g0_v0", "g0_v0_negzero_w", "subnormal_v", "min_subnormal_v", "g_square_subnormal", "g_square_underflows", "g_+3e38", "g_-3e38"]


def edge_vector():
    """23 elements (five groups of four and a tail of three): ordinary random elements with the edge elements planted at
    positions 1.. and again in the tail.  -> (w, m, v, g float32, {name: [positions]})"""
    n = 23
    w, m, v = random_state(n, 77)
    g = random_grad(n, 78, None)
    rows = {                                             # name: (w, m, v, g)
        "g0_v0": (0.75, 0.0, 0.0, 0.0),
        "g0_v0_negzero_w": (-0.0, 0.0, 0.0, 0.0),
        "subnormal_v": (0.5, 1e-25, 1e-40, 0.0),
        "min_subnormal_v": (-0.5, 0.0, 1.4e-45, 1e-24),
        "g_square_subnormal": (1.25, 0.0, 0.0, 1e-20),
        "g_square_underflows": (-1.25, 0.0, 0.0, 1e-30),
        "g_+3e38": (2.0, 1e-3, 1e-4, 3e38),
        "g_-3e38": (-2.0, 1e-3, 1e-4, -3e38),
    }
    where = {k: [] for k in rows}
    for p, name in list(enumerate(EDGE_NAMES, start=1)) + [(20, "g0_v0_negzero_w"), (21, "g_+3e38"), (22, "subnormal_v")]:
        w[p], m[p], v[p] = (F32(x) for x in rows[name][:3])
        g[p] = bf16_round(np.array([rows[name][3]], dtype=F32))[0]
        where[name].append(p)
    return w, m, v, g, where


def edge_state32():
    """(lr, bc1, rbc2) float32 the edge test writes into the state buffer: the kernel's inputs."""
    bc1, rbc2 = kernel_bc32(BETA1, BETA2, EDGE_STEP)
    return F32(EDGE_HYPER["lr"]), bc1, rbc2


def case_kwargs(case, t, sumsq, state=None):
    """step64's keyword arguments for step t of a case, and the bar's.  Host path: float64 corrections, host_rho in the bar.
    dev_state path: `state` = the (lr, bc1, rbc2) floats read back from the state buffer.  -> (step kwargs, bar kwargs)"""
    _, clip, gs, wd, lr, dev = case
    kw = dict(lr=lr, beta1=BETA1, beta2=BETA2, eps=EPS, weight_decay=wd, grad_scale=gs, max_norm=MAX_NORM if clip else 0.0,
              sumsq=sumsq if clip else None)
    if dev:
        kw.update(lr=float(state[0]), bc1=float(state[1]), rbc2=float(state[2]))
        return kw, dict(clip=bool(clip))
    kw["bc1"], kw["rbc2"] = host_bc(BETA1, BETA2, t)
    r1, rr = host_rho(BETA1, BETA2, t)
    return kw, dict(clip=bool(clip), rho_bc1=r1, rho_rbc2=rr)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (numpy or torch), 0 where both the error and the bound are 0."""
    xp = _xp(ref)
    err = abs(_f64(got) - ref)
    return float((err / xp.where(bound > 0, bound, bound + 1e-300)).max())
