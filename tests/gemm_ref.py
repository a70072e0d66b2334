"""Exact-answer inputs, expectations, case tables and expected kernel symbols of the GEMM family (gemm.hip, gemm256.hip,
gemm8p.hip, the shared epilogue of gemm_core.h).  tests/test_gemm_ref_cpu.py qualifies this file without a GPU,
tests/test_gemm_exact_gpu.py holds the kernels to it bit for bit.

Why the answers do not depend on the summation order.  Operands are small integers (exactly representable in bf16), so every
product and every partial sum of a dot product is an integer; as long as the largest possible |sum| stays below 2^24 every
partial sum is an fp32 value, whatever the order, the k-tile size or the split.  The fp32 accumulator a kernel holds before its
epilogue is therefore THE integer, and the stored value is one round-to-nearest-even of what the epilogue makes of it.

    kind "unit"   A in {-1, 0, 1}, B in {-2 .. 2}: |sum| stays below 256 at the shapes of the tables (asserted on the reference,
                  bf16_exact_bound), so a bf16 C is the integer itself; 1-2 % of the outputs are exactly 0 (the ReLU / bit-mask edge)
    kind "wide"   A, B in {-4 .. 4}: |sum| <= 16 K < 2^24 (asserted); the fp32 C is the integer, the bf16 C its round-to-nearest-
                  even -- odd integers in [256, 512) are ties (count_ties)
    kind "gelu"   A in {-1, 0, 1}, B and the bias multiples of 1/8 in [-1.5, 1.5]: sums are multiples of 1/8 below 32, exact in
                  fp32 AND in bf16 (8 bits above the 1/8 place), so the stored pre-activation is known bit for bit
    side inputs   bias in {-3 .. 3}, residual in {-4 .. 4}, aux_in in {-2 .. 2} (zeros and negatives), dact_scale in {1, 2},
                  dropout p = 0.5 (keep scale exactly 2): bias -> act -> dropout -> residual -> dact stays in integers below
                  2^24, one rounding at the store

expect() follows the order documented at sfcvit_gemm (include/sfcvit.h) in fp64 and rounds once with rowwise_ref.round_bf16.

GELU bar.  The epilogue calls gelu_erf / gelu_erf_grad of device_common.h, the functions of the stand-alone GELU kernels, so y is
held to rowwise_ref.gelu_floor(pre) and dX = v gelu'(a) ds to ds gelu_floor(a, v): the kernel forms fl(v gelu'(a)) -- the one
product the stand-alone backward forms with dy in v's place -- and then multiplies by ds in {1, 2}, a power of two, which adds
no rounding and scales value and error alike.
"""
import fnmatch
import re

import numpy as np
import torch

from rowwise_ref import BF16, bf, bf16_step, elementwise_verdict, f64, gelu_floor, gelu_grad_ref, gelu_ref, round_bf16  # noqa: F401

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
P8_BITS = dict(RELU=1, DROP=2, RES=4, DACT=8, CSUM=16, BITS=32)     # csrc/dispatch.h P8_*; the CPU test reads the header
BIAS_MAX_N = 8160
DROP_P, KEEP_SCALE = 0.5, 2.0
TILE_OF_MODE = {8: 256, 9: 224, 10: 192, 0: 192}                    # force mode -> tile rows (automatic dispatch takes 192-row
                                                                    # tiles wherever all heights need one round of workgroups)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1000003, 100003, 10007, 101, 1))) + 77)


def exact_inputs(M, N, K, kind="unit", tag=0):
    """-> a [M, K], b [N, K] int64 (kind "gelu": b holds EIGHTHS).  Logical layout; a k-major operand is a.t().contiguous()."""
    g = _gen(tag, M, N, K, {"unit": 1, "wide": 2, "gelu": 3}[kind])
    if kind == "wide":
        assert 16 * K < 2 ** 24
        return torch.randint(-4, 5, (M, K), generator=g), torch.randint(-4, 5, (N, K), generator=g)
    a = torch.randint(-1, 2, (M, K), generator=g)
    if kind == "gelu":
        return a, torch.randint(-12, 13, (N, K), generator=g)
    return a, torch.randint(-2, 3, (N, K), generator=g)


def side_inputs(M, N, tag=0):
    """-> bias [N] in {-3 .. 3}, residual [M, N] in {-4 .. 4}, aux_in [M, N] in {-2 .. 2} (int64)."""
    g = _gen(tag, M, N, 0, 9)
    return torch.randint(-3, 4, (N,), generator=g), torch.randint(-4, 5, (M, N), generator=g), torch.randint(-2, 3, (M, N), generator=g)


def one_hot_a(M, K, tag=0):
    """A [M, K] with one 1 per row at a random k: C's row m is row idx[m] of B^T (catches a permuted fragment map).  -> a, idx."""
    idx = torch.randint(0, K, (M,), generator=_gen(tag, M, K, 0, 5))
    a = torch.zeros(M, K, dtype=torch.int64)
    a[torch.arange(M), idx] = 1
    return a, idx


def synthetic_keep(M, N, tag=0):
    """A keep mask for the CPU tests (the GPU test takes the library's: ops.dropout_mask)."""
    return torch.rand(M, N, generator=_gen(tag, M, N, 0, 7)) >= DROP_P


def pack_bits(pos):
    """bool [M, N] -> uint8 [M, N / 8], bit (n & 7) of byte n >> 3 (sfcvit_gemm_args.actmask)."""
    M, N = pos.shape
    w = (pos.view(M, N // 8, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(-1)
    return w.to(torch.uint8)


# ---- the expectation -----------------------------------------------------------------------------------------------------
def expect(a, b, *, bias=None, act=ACT_NONE, keep=None, residual=None, aux_in=None, dact=ACT_NONE, dact_scale=1.0, out_f32=False,
           b_scale=1.0):
    """Everything sfcvit_gemm stores for C = epilogue(a b^T), in fp64 in the documented order: v += bias; pre = bf16(v);
    v = act(v); v = keep ? 2 v : 0; v += residual; v *= dact(aux_in) dact_scale; C = v.  a, b and the side inputs hold exact values
    (any dtype; b_scale = 1/8 for the eighths of kind "gelu").  ReLU only: the GELU cases go through gelu_expect.
    -> dict  acc     fp64 [M, N] the sums
             v       fp64 the epilogue's value before the store
             c       what is stored: bf16 (one rounding of v) or fp32
             pre     bf16 pre-activation (aux_out)
             colsum  fp64 [N] column sums of v: the persistent kernel's fused sums (of the fp32 values it stores as bf16)
             colsum_c  fp64 [N] column sums of the stored C: the separate pass of the other kernels
             bits    uint8 [M, N / 8] of (C > 0) when N % 8 == 0."""
    assert act in (ACT_NONE, ACT_RELU) and dact in (ACT_NONE, ACT_RELU)
    acc = (a.double() @ b.double().t()) * b_scale
    v = acc.clone()
    if bias is not None:
        v = v + bias.double() * b_scale
    out = dict(acc=acc, pre=round_bf16(v.numpy()))
    if act == ACT_RELU:
        v = v.clamp_min(0.0)
    if keep is not None:
        v = torch.where(keep, v * KEEP_SCALE, torch.zeros_like(v))
    if residual is not None:
        v = v + residual.double()
    if dact == ACT_RELU:
        v = torch.where(aux_in.double() > 0, v * float(dact_scale), torch.zeros_like(v))
    assert float(v.abs().max()) * 8 < 2 ** 24 and float(v.abs().sum(0).max()) < 2 ** 24
    c = v.float() if out_f32 else round_bf16(v.numpy())
    assert not out_f32 or torch.equal(c.double(), v)
    out.update(v=v, c=c, colsum=v.sum(0), colsum_c=c.double().sum(0))
    if v.shape[1] % 8 == 0:
        out["bits"] = pack_bits(c > 0)
    return out


def bf16_exact_bound(want):
    """The bound of kind "unit", on the reference alone: every sum is an integer below 256, i.e. a bf16 value."""
    acc = want["acc"]
    return bool(torch.equal(acc, acc.round())) and float(acc.abs().max()) < 256


def count_ties(v):
    """How many entries of fp64 v lie exactly halfway between two bf16 values."""
    x = np.abs(np.asarray(v, dtype=np.float64))
    s = bf16_step(x)
    return int((np.mod(x, s) == s / 2).sum())


def colsum_slot(sums64, as_bf16):
    """The column sums as stored: fp32, or one bf16 rounding of the exact sum."""
    return round_bf16(sums64.numpy()) if as_bf16 else sums64.float()


def gelu_expect(a, b8, bias8):
    """kind "gelu" forward: pre = (a b8^T + bias8) / 8 exactly (bf16), y = gelu(pre) in fp64.  -> pre bf16, y fp64, floor."""
    pre = (a.double() @ b8.double().t() + bias8.double()) / 8
    assert float(pre.abs().max()) < 32                                   # eighths below 32: 8 significant bits, exact in bf16
    pre_bf = round_bf16(pre.numpy())
    assert torch.equal(pre_bf.double(), pre)
    return pre_bf, gelu_ref(pre_bf), gelu_floor(pre_bf)


def gelu_dx_expect(a, b8, aux_bf, ds):
    """kind "gelu" backward: dX = v gelu'(aux) ds with v = a b8^T / 8 exact.  -> v fp64 tensor, dX fp64, floor (see the header)."""
    v = (a.double() @ b8.double().t()) / 8
    assert ds in (1.0, 2.0)
    ref = v.numpy() * gelu_grad_ref(aux_bf) * ds
    return v, ref, ds * gelu_floor(aux_bf, v)


def stored(want, epi, fused_colsum):
    """What a launch with this epilogue leaves behind, from expect()'s dict: c; pre (want_aux); the column sums as fp32 and as a
    bf16 slot (fused_colsum: sums of the fp32 values, else of the stored C); bits (written with act = RELU)."""
    out = dict(c=want["c"])
    if epi.get("aux"):
        out["pre"] = want["pre"]
    if epi.get("colsum"):
        s = want["colsum"] if fused_colsum else want["colsum_c"]
        out["colsum"], out["colsum_bf16"] = colsum_slot(s, False), colsum_slot(s, True)
    if epi.get("bits") and epi.get("act") == ACT_RELU:
        out["bits"] = want["bits"]
    return out


# ---- the verdict both test files use -------------------------------------------------------------------------------------
def exact_verdict(got, want):
    """-> the keys of `got` that are not bit-for-bit what `want` holds (empty list: pass).  No tolerance anywhere."""
    bad = []
    for k, t in got.items():
        w = want[k]
        t = t.detach().cpu()
        if t.dtype != w.dtype or t.shape != w.shape or not torch.equal(t, w):
            bad.append(k)
    return bad


# ---- kernel symbols --------------------------------------------------------------------------------------------------------
def tf(x):
    return "true" if x else "false"


def p8_symbol(mode, mask):
    """gemm8p_kernel<NI, MASK, *>: NI = tile rows / 32, MASK = the P8_* bits of the epilogue, * = the k-tile schedule switch."""
    return "gemm8p_kernel<%d, %d, *>" % (TILE_OF_MODE[mode] // 32, mask)


def ring_symbol(akm, bkm, bn, heavy=False):
    return "gemm256_kernel<%s, %s, %d, %s>" % (tf(akm), tf(bkm), bn, tf(heavy))


def generic_symbol(akm, bkm, heavy=False):
    return "gemm_kernel<%s, %s, %s>" % (tf(akm), tf(bkm), tf(heavy))


KM_SYMBOL = "gemm8p_km_kernel<*>"
SYMBOL_RE = re.compile(r"^(gemm8p_kernel<[678], \d+, (\*|true|false)>|gemm8p_km_kernel<(\*|true|false)>|"
                       r"gemm256_kernel<(true|false), (true|false), (128|256), (true|false)>|gemm_kernel<(true|false), (true|false), (true|false)>)$")


def symbol_matches(pattern, ran):
    return fnmatch.fnmatchcase(ran, pattern.replace("*", "?*"))


def mask_of(epi):
    """The persistent kernel's MASK of an epilogue (csrc/dispatch.cpp plan_p8)."""
    m = 0
    if epi.get("act") == ACT_RELU:
        m |= P8_BITS["RELU"]
    if epi.get("drop"):
        m |= P8_BITS["DROP"]
    if epi.get("res"):
        m |= P8_BITS["RES"]
    if epi.get("dact") == ACT_RELU:
        m |= P8_BITS["DACT"]
    if epi.get("colsum"):
        m |= P8_BITS["CSUM"]
    if epi.get("bits") and (m & (P8_BITS["RELU"] | P8_BITS["DACT"])) and not m & P8_BITS["RES"]:
        m |= P8_BITS["BITS"]
    return m


# ---- case tables -----------------------------------------------------------------------------------------------------------
# An epilogue is a dict of switches: bias, act, drop, res, dact (+ ds), colsum, bits, f32, aux (want_aux).
P8_EPILOGUES = {                                  # every variant plan_p8 admits / launch_mask instantiates, by MASK
    "bias": dict(bias=True),
    "bias+res": dict(bias=True, res=True),
    "bias+drop+res": dict(bias=True, drop=True, res=True),
    "bias+relu": dict(bias=True, act=ACT_RELU),
    "bias+relu+drop": dict(bias=True, act=ACT_RELU, drop=True),
    "dact": dict(dact=ACT_RELU, ds=2.0),
    "dact+csum": dict(dact=ACT_RELU, ds=2.0, colsum=True),
    "bias+relu+bits": dict(bias=True, act=ACT_RELU, bits=True),
    "bias+relu+drop+bits": dict(bias=True, act=ACT_RELU, drop=True, bits=True),
    "dact+bits": dict(dact=ACT_RELU, ds=2.0, bits=True),
    "dact+csum+bits": dict(dact=ACT_RELU, ds=1.0, colsum=True, bits=True),
}
P8_MASKS = (0, 4, 6, 1, 3, 8, 24, 33, 35, 40, 56)
P8_MODES = (8, 9, 10, 0)
P8_KS = (256, 384, 640, 896)


def p8_rows(mode):
    """One tile; tile + 1 and 2 tile - 1 (the last tile almost all overlap / barely any); tile + 8."""
    t = TILE_OF_MODE[mode]
    return (t, t + 1, 2 * t - 1, t + 8)


def p8_shape_cases():
    """(mode, M, N, K, symbol): bias epilogue, N = 512."""
    return [(mode, M, 512, K, p8_symbol(mode, 0)) for mode in P8_MODES for K in P8_KS for M in p8_rows(mode)]


P8_WALK_CASES = [                                 # (mode, M, N, K, symbol): tile walk, queue and start-up stagger
    (8, 512, 1792, 256, p8_symbol(8, 0)),         # seven column tiles: the 6-wide window + a remainder of one
    (0, 512, 1792, 256, p8_symbol(0, 0)),         # the same through automatic dispatch (192-row tiles, ragged)
    (8, 256 * 37, 1792, 256, p8_symbol(8, 0)),    # 259 tiles for 256 workgroups: some draw a second and a third tile
    (8, 256 * 74, 1792, 256, p8_symbol(8, 0)),    # 518 tiles >= 2 x 256: the start-up stagger is on
]


def p8_epilogue_rows(mode):
    """An aligned and a ragged M per tile height (ragged: the last tile shares tile - 72 rows with the first, both wave groups)."""
    t = TILE_OF_MODE[mode]
    return (2 * t, t + 72)


def p8_epilogue_cases():
    """(mode, M, N, K, name, epilogue, symbol)."""
    return [(mode, M, 512, 256, name, epi, p8_symbol(mode, mask_of(epi)))
            for mode in (8, 9, 10) for M in p8_epilogue_rows(mode) for name, epi in P8_EPILOGUES.items()]


P8_BIAS_LIMIT_CASES = [                           # (M, N, K, symbol), automatic dispatch with a bias
    (256, 7936, 256, p8_symbol(0, 0)),            # 15 872 bytes of bias: still inside the LDS
    (256, 8192, 256, ring_symbol(False, False, 128)),   # N > BIAS_MAX_N: the ring kernel
]

KM_MN = ((256, 256), (256, 512), (512, 256))
KM_KS = (                                         # (K, splitk, symbol, what)
    (256, 2, KM_SYMBOL, "four k-tiles, the least the plan accepts"),
    (264, 2, KM_SYMBOL, "an 8-row tail slab"),
    (384, 2, KM_SYMBOL, "uneven splits of 4 + 2 k-tiles"),
    (384, 3, KM_SYMBOL, "three splits of 2"),
    (640, 4, KM_SYMBOL, "k-tiles per split rounded up to even: 4 + 4 + 2, three splits"),
    (1096, 3, KM_SYMBOL, "6 + 6 + 4 and a 72-row tail slab"),
    (4168, None, generic_symbol(True, True), "auto_splitk keeps K / s >= 512, so it does not split: the generic kernel, whole K"),
    (4168, 8, KM_SYMBOL, "the same K on the weight-gradient kernel: eight splits and a 72-row tail slab"),
)


def km_cases():
    return [(M, N, K, s, sym) for M, N in KM_MN for K, s, sym, _ in KM_KS]


RING_MODES = (4, 6, 7)
RING_KS = (32, 96, 160, 256)                      # stages of 32: 1 (less than a 64-deep k-tile), 3, 5, 8
RING_MS = (256, 512)
RING_NS = (128, 256, 384)
LAYOUTS = ((False, False), (False, True), (True, False), (True, True))


def ring_bn(mode, N):
    """plan_ring at these sizes: fewer than 200 tiles, so only mode 7 takes 256-wide tiles, and only where N allows."""
    return 256 if mode == 7 and N % 256 == 0 else 128


def ring_cases():
    """(mode, akm, bkm, M, N, K, symbol)."""
    return [(mode, akm, bkm, M, N, K, ring_symbol(akm, bkm, ring_bn(mode, N)))
            for mode in RING_MODES for akm, bkm in LAYOUTS for M in RING_MS for N in RING_NS for K in RING_KS]


RING_SPLIT_CASES = [                              # (M, N, K, splitk, what): kind "wide", fp32 and bf16 C, mode 4
    (1024, 1024, 2048, 3, "64 output tiles: three ranges of 704, 704 and 640"),
    (256, 256, 2048, 3, "4 output tiles: one set of ranges per XCD, 8 x 256"),
]
RING_EPILOGUES = {
    "bias+res": dict(bias=True, res=True),
    "dact": dict(dact=ACT_RELU, ds=2.0),
    "res+f32": dict(res=True, f32=True),
}
RING_EPILOGUE_SHAPES = ((512, 384, 160), (256, 256, 96))

GEN_KS = (8, 72, 200, 1000)
GEN_MS = (1, 7, 129, 200)
GEN_NS = (4, 12, 132, 264)                        # the 4-column half vector (N % 8 = 4) and nvalid < 4 past the end


def generic_cases():
    """(akm, bkm, M, N, K, symbol): every shape k-contiguous; the k-major layouts where M % 8 == 0 / N % 8 == 0 allow them;
    both operands k-major with K = 12 (no multiple of 8)."""
    cases = [(False, False, M, N, K) for K in GEN_KS for M in GEN_MS for N in GEN_NS]
    cases += [(akm, bkm, 200, 264, K) for K in GEN_KS for akm, bkm in LAYOUTS[1:]]
    cases += [(True, True, 200, 264, 12), (True, True, 8, 8, 12)]
    return [c + (generic_symbol(c[0], c[1]),) for c in cases]


GEN_SPLIT_CASES = [                               # (M, N, K, splitk, empty ranges): fewer than 64 tiles -> splits rounded up to 8s
    (192, 136, 192, 2, (3, 4, 5, 6, 7)),          # 3 k-tiles over 8 ranges
    (192, 136, 3000, 5, ()),                      # 47 k-tiles: 8 ranges of 6 (the last of 5)
    (192, 136, 3000, 16, ()),                     # 16 ranges of 3 k-tiles (the last of 2, 120 rows deep)
]
GEN_EPILOGUES = {
    "bias": dict(bias=True),
    "bias+relu": dict(bias=True, act=ACT_RELU),
    "bias+res": dict(bias=True, res=True),
    "relu+drop+res": dict(act=ACT_RELU, drop=True, res=True),
    "dact": dict(dact=ACT_RELU, ds=2.0),
    "res+f32": dict(res=True, f32=True),
    "relu+aux": dict(bias=True, act=ACT_RELU, aux=True),
    "bias+dact": dict(bias=True, dact=ACT_RELU, ds=2.0),     # the persistent DACT variants drop the bias: must never get this call
    "res+dact": dict(res=True, dact=ACT_RELU, ds=2.0),       # MASK 12 is no persistent variant either: dact scales the residual too
    "relu+bits": dict(bias=True, act=ACT_RELU, bits=True),   # the bit mask through the separate pass (N % 16 == 0)
}
GEN_EPILOGUE_SHAPES = ((200, 264, 200), (129, 132, 72))
GEN_BITS_SHAPE = (200, 144, 72)

GELU_CASES = [                                    # (force mode, M, N, K, symbol): HEAVY instantiations
    (1, 200, 264, 32, generic_symbol(False, False, True)),
    (1, 256, 256, 32, generic_symbol(False, False, True)),
    (4, 256, 256, 32, ring_symbol(False, False, 128, True)),
]
GELU_DS = (1.0, 2.0)

DX_EPILOGUES = {
    "plain": dict(),
    "res": dict(res=True),
    "dact": dict(dact=ACT_RELU, ds=2.0),
    "dact+csum": dict(dact=ACT_RELU, ds=2.0, colsum=True),
    "dact+bits": dict(dact=ACT_RELU, ds=2.0, bits=True),
    "dact+csum+bits": dict(dact=ACT_RELU, ds=2.0, colsum=True, bits=True),
}
DX_ROUTES = {                                     # name -> (M, out features = K, in features = N, symbol of an epilogue)
    "persistent": (328, 256, 512, lambda epi: p8_symbol(0, mask_of(epi))),
    "ring": (256, 96, 384, lambda epi: ring_symbol(False, False, 128)),
    "generic": (200, 72, 272, lambda epi: generic_symbol(False, True)),
}


def all_exact_cases():
    """Every exact case of the tables as (family, akm, bkm, M, N, K, kind, epilogue, out_f32, symbol, extra) -- what the CPU test
    walks for bounds and mutants.  extra: dict(tile=..) for the persistent kernel, dict(splitk=.., empty=..) for split-K."""
    out = []
    for mode, M, N, K, sym in p8_shape_cases() + P8_WALK_CASES:
        out.append(("p8", False, False, M, N, K, "unit", P8_EPILOGUES["bias"], False, sym, dict(tile=TILE_OF_MODE[mode])))
    for mode, M, N, K, name, epi, sym in p8_epilogue_cases():
        out.append(("p8", False, False, M, N, K, "unit", epi, False, sym, dict(tile=TILE_OF_MODE[mode])))
    for M, N, K, sym in P8_BIAS_LIMIT_CASES:
        out.append(("p8", False, False, M, N, K, "unit", P8_EPILOGUES["bias"], False, sym, dict(tile=192)))
    for M, N, K, s, sym in km_cases():
        for f32 in (True, False):
            out.append(("km", True, True, M, N, K, "wide", {}, f32, sym, dict(splitk=s, tail=K % 128 if sym == KM_SYMBOL else 0)))
    for mode, akm, bkm, M, N, K, sym in ring_cases():
        out.append(("ring", akm, bkm, M, N, K, "unit", {}, False, sym, {}))
    for M, N, K, s, _ in RING_SPLIT_CASES:
        for f32 in (True, False):
            out.append(("ring", False, False, M, N, K, "wide", {}, f32, ring_symbol(False, False, 128), dict(splitk=s)))
    for M, N, K in RING_EPILOGUE_SHAPES:
        for epi in RING_EPILOGUES.values():
            out.append(("ring", False, False, M, N, K, "unit", epi, bool(epi.get("f32")), ring_symbol(False, False, 128), {}))
    for akm, bkm, M, N, K, sym in generic_cases():
        out.append(("generic", akm, bkm, M, N, K, "unit", {}, False, sym, {}))
    for M, N, K, s, empty in GEN_SPLIT_CASES:
        for f32 in (True, False):
            out.append(("generic", True, True, M, N, K, "wide", {}, f32, generic_symbol(True, True), dict(splitk=s, empty=empty)))
    for M, N, K in GEN_EPILOGUE_SHAPES + (GEN_BITS_SHAPE,):
        for name, epi in GEN_EPILOGUES.items():
            if bool(epi.get("bits")) == ((M, N, K) == GEN_BITS_SHAPE):
                out.append(("generic", False, False, M, N, K, "unit", epi, bool(epi.get("f32")), generic_symbol(False, False), {}))
    for route, (M, K, N, sym) in DX_ROUTES.items():
        for epi in DX_EPILOGUES.values():
            out.append(("dx-" + route, False, route == "generic", M, N, K, "unit", epi, False, sym(epi), dict(tile=192)))
    return out


def build_case(M, N, K, kind, epi, out_f32, keep=None, tag=0):
    """Inputs and expectation of one exact case.  keep: the [M, N] keep flags when the epilogue has dropout (the library's own on
    the GPU, synthetic_keep on the CPU).  -> dict(a, b, bias, res, aux: int64 or None; want: expect()'s dict)."""
    a, b = exact_inputs(M, N, K, kind, tag)
    bias, res, aux = side_inputs(M, N, tag)
    use = dict(bias=bias if epi.get("bias") else None, res=res if epi.get("res") else None, aux=aux if epi.get("dact") else None)
    want = expect(a, b, bias=use["bias"], act=epi.get("act", ACT_NONE), keep=keep if epi.get("drop") else None, residual=use["res"],
                  aux_in=use["aux"], dact=epi.get("dact", ACT_NONE), dact_scale=epi.get("ds", 1.0), out_f32=out_f32)
    return dict(a=a, b=b, want=want, **use)
