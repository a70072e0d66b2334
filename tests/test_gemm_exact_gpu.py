"""The GEMM kernels (csrc/gemm.hip, gemm256.hip, gemm8p.hip, the epilogue of gemm_core.h) held bit for bit to tests/gemm_ref.py,
whose docstring says why the answers do not depend on the summation order and which tests/test_gemm_ref_cpu.py qualifies
without a GPU.

Every exact case: inputs generated on the CPU, the bounds asserted on the reference before the kernel is looked at, the result
produced twice (the runs must agree), every output torch.equal to the expectation, the kernel symbol that ran asserted.  No
tolerance anywhere on exact inputs; the GELU cases (HEAVY instantiations) carry the floor of the stand-alone GELU kernels.
The shapes are the smallest that reach each path of the kernels and of csrc/dispatch.cpp -- no workload shapes.
A summary (cases per family, symbols seen, worst GELU |err| / floor) is printed when the module is done."""
import collections

import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SEED = 1234567
SENTINEL = 0xA5
SEEN = collections.defaultdict(collections.Counter)           # family -> symbol -> cases
GELU_WORST = [0.0]


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    for fam, syms in SEEN.items():
        print(f"FIGURE gemm exact {fam}: {sum(syms.values())} cases; " + "; ".join(f"{s} x {n}" for s, n in sorted(syms.items())))
    print(f"FIGURE gemm exact gelu: worst |err| / floor {GELU_WORST[0]:.3f}")


def dev(t, scale=1.0):
    """Exact integer (or eighths) tensor -> bf16 on the GPU."""
    return None if t is None else (t.double() * scale).to(torch.float32).to(BF16).cuda()


def operand(t, kmajor):
    return t.t().contiguous() if kmajor else t


def logged(ops, fn):
    ops.KERNEL_LOG = []
    try:
        out = fn()
    finally:
        ran, ops.KERNEL_LOG = ops.KERNEL_LOG, None
    return out, ran


def keep_flags(ops, M, N, epi, seed=SEED):
    """The library's own keep flags (ops.dropout_mask) of an epilogue with dropout, on the CPU."""
    if not epi.get("drop"):
        return None
    mask = ops.dropout_mask(M, N, G.DROP_P, seed).cpu()
    assert set(mask.float().unique().tolist()) == {0.0, G.KEEP_SCALE}
    return mask > 0


def launch(ops, d, epi, mode, *, akm=False, bkm=False, f32=False, splitk=None, colsum_bf16=False, bits_from_aux=None, row_offset=0,
           seed=SEED, dx_weight=None):
    """One sfcvit_gemm call of a case (d: its device tensors).  -> (dict of what it stored, as gemm_ref.stored names it; symbols)."""
    M, N = d["M"], d["N"]
    kw = dict(force_generic=mode, out_f32=f32, row_offset=row_offset)
    if splitk is not None:
        kw["splitk"] = splitk
    if epi.get("bias"):
        kw["bias"] = d["bias"]
    if epi.get("act"):
        kw["act"] = epi["act"]
    if epi.get("drop"):
        kw.update(dropout_p=G.DROP_P, dropout_seed=seed)
    if epi.get("res"):
        kw["residual"] = d["res"]
    if epi.get("dact"):
        kw.update(aux_in=d["aux"], dact=epi["dact"], dact_scale=epi.get("ds", 1.0))
    if epi.get("aux"):
        kw["want_aux"] = True
    cs = None
    if epi.get("colsum"):
        cs = torch.full((N,), float("nan"), device="cuda", dtype=BF16) if colsum_bf16 else True
        kw["colsum"] = cs
    bits = None
    if epi.get("bits"):
        bits = torch.full((M, N // 8 + 2), SENTINEL, device="cuda", dtype=torch.uint8)      # two spare bytes per row
        if epi.get("dact"):
            bits[:, :N // 8] = bits_from_aux
        kw["actmask"] = bits
    if dx_weight is not None:
        kw.pop("force_generic")
        res, ran = logged(ops, lambda: ops.gemm_dx(d["a"], dx_weight, **kw))
    else:
        res, ran = logged(ops, lambda: ops.gemm(operand(d["a"], akm), operand(d["b"], bkm), a_kmajor=akm, b_kmajor=bkm, **kw))
    torch.cuda.synchronize()
    res = res if isinstance(res, tuple) else (res,)
    got = dict(c=res[0])
    if epi.get("aux"):
        got["pre"] = res[1]
    if epi.get("colsum"):
        got["colsum_bf16" if colsum_bf16 else "colsum"] = res[-1]
    if bits is not None:
        assert bool((bits[:, N // 8:] == SENTINEL).all()), "bytes past N / 8 of the bit mask were written"
        if epi.get("act") == G.ACT_RELU:
            got["bits"] = bits[:, :N // 8].contiguous()
    return got, ran


def check_case(ops, family, M, N, K, kind, epi, mode, symbol, *, akm=False, bkm=False, f32=False, splitk=None, tag=0, fused=False,
               dx=False):
    """Build the case, assert the bounds on the reference, run it twice, compare bit for bit, assert the symbol.  -> (inp, got, device tensors)."""
    inp = G.build_case(M, N, K, kind, epi, f32, keep=keep_flags(ops, M, N, epi), tag=tag)
    want = inp["want"]
    if kind == "unit":
        assert G.bf16_exact_bound(want)                            # max |sum| < 256, on the reference alone
    else:
        assert 16 * K < 2 ** 24
    d = dict(M=M, N=N, a=dev(inp["a"]), b=dev(inp["b"]), bias=dev(inp["bias"]), res=dev(inp["res"]), aux=dev(inp["aux"]))
    extra = dict(akm=akm, bkm=bkm, f32=f32, splitk=splitk)
    if dx:
        extra["dx_weight"] = d["b"].t().contiguous()               # W [out = K, in = N]: dX = dY W
    if epi.get("bits") and epi.get("dact"):
        extra["bits_from_aux"] = G.pack_bits(inp["aux"] > 0).cuda()
    st = G.stored(want, epi, fused)
    where = (family, M, N, K, sorted(epi), mode, splitk)
    got = {}
    for slot in ((False, True) if epi.get("colsum") else (False,)):
        first, ran = launch(ops, d, epi, mode, colsum_bf16=slot, **extra)
        again, ran2 = launch(ops, d, epi, mode, colsum_bf16=slot, **extra)
        assert len(ran) == 1 and G.symbol_matches(symbol, ran[0]) and ran2 == ran, (where, ran, symbol)
        assert G.exact_verdict(again, {k: v.cpu() for k, v in first.items()}) == [], ("run to run", where)
        got.update(first)
    bad = G.exact_verdict(got, st)
    assert bad == [], (where, bad, {k: int((got[k].cpu() != st[k]).sum()) for k in bad if got[k].shape == st[k].shape})
    assert set(got) == set(st), (where, sorted(got), sorted(st))
    SEEN[family][ran[0]] += 1
    return inp, got, d


# ---- persistent kernel (gemm8p_kernel) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.P8_MODES)
@pytest.mark.parametrize("K", G.P8_KS)
def test_persistent_rows_and_k(ops, mode, K):
    """One tile, tile + 1, 2 tile - 1, tile + 8 rows at every k-loop length (the shortest; odd and even counts of 128-deep pairs)."""
    for i, M in enumerate(G.p8_rows(mode)):
        check_case(ops, "persistent", M, 512, K, "unit", G.P8_EPILOGUES["bias"], mode, G.p8_symbol(mode, 0), tag=i)


@pytest.mark.parametrize("mode,M,N,K,symbol", G.P8_WALK_CASES)
def test_persistent_tile_walk_and_queue(ops, mode, M, N, K, symbol):
    check_case(ops, "persistent", M, N, K, "unit", G.P8_EPILOGUES["bias"], mode, symbol)


@pytest.mark.parametrize("mode", (8, 9, 10))
@pytest.mark.parametrize("ragged", (False, True))
def test_persistent_every_epilogue(ops, mode, ragged):
    """Every instantiated MASK on an aligned and a ragged M: C, the fused column sums (fp32 and a bf16 slot), the bit mask written
    and read; and the generic kernel stores the same bits."""
    M = G.p8_epilogue_rows(mode)[ragged]
    for i, (name, epi) in enumerate(G.P8_EPILOGUES.items()):
        fused = bool(epi.get("colsum"))
        inp, got, d = check_case(ops, "persistent", M, 512, 256, "unit", epi, mode, G.p8_symbol(mode, G.mask_of(epi)), tag=i, fused=fused)
        plain = {k: v for k, v in epi.items() if k not in ("colsum", "bits")}
        generic, ran = launch(ops, d, plain, 1)
        assert ran == [G.generic_symbol(False, False)] and torch.equal(generic["c"], got["c"]), (name, ran)
        if epi.get("bits") and epi.get("dact"):                    # reading the bits is reading aux_in
            no_bits, _ = launch(ops, d, {k: v for k, v in epi.items() if k != "bits"}, mode)
            assert torch.equal(no_bits["c"], got["c"]), name


@pytest.mark.parametrize("M,N,K,symbol", G.P8_BIAS_LIMIT_CASES)
def test_bias_vector_at_the_lds_limit(ops, M, N, K, symbol):
    assert (N <= G.BIAS_MAX_N) == symbol.startswith("gemm8p_kernel")
    check_case(ops, "persistent" if N <= G.BIAS_MAX_N else "ring", M, N, K, "unit", G.P8_EPILOGUES["bias"], 0, symbol)


def test_bias_with_dact_never_reaches_the_persistent_kernel(ops):
    """The persistent DACT variants carry no bias: a call with both must fall back (and be exact), forcing it is refused."""
    epi = dict(bias=True, dact=G.ACT_RELU, ds=2.0)
    _, _, d = check_case(ops, "ring", 512, 512, 256, "unit", epi, 0, G.ring_symbol(False, False, 128))
    with pytest.raises(Exception, match="not eligible"):
        launch(ops, d, epi, 8)


def test_persistent_strided_operands(ops):
    """A, out= and the residual as column slices of wider tensors (ld* multiples of 8): exact C, the columns outside keep a sentinel."""
    M, N, K, epi = 328, 512, 256, G.P8_EPILOGUES["bias+res"]
    inp = G.build_case(M, N, K, "unit", epi, False)
    assert G.bf16_exact_bound(inp["want"])
    wide_a = torch.full((M, K + 16), 3.0, device="cuda", dtype=BF16)
    wide_r = torch.full((M, N + 16), 5.0, device="cuda", dtype=BF16)
    wide_a[:, 8:8 + K] = dev(inp["a"])
    wide_r[:, 8:8 + N] = dev(inp["res"])
    for mode in (8, 9, 10):
        wide_c = torch.full((M, N + 16), 77.0, device="cuda", dtype=BF16)
        for _ in range(2):
            _, ran = logged(ops, lambda: ops.gemm(wide_a[:, 8:8 + K], dev(inp["b"]), bias=dev(inp["bias"]), residual=wide_r[:, 8:8 + N],
                                                  out=wide_c[:, 8:8 + N], force_generic=mode))
            torch.cuda.synchronize()
            assert len(ran) == 1 and G.symbol_matches(G.p8_symbol(mode, 4), ran[0]), ran
            assert torch.equal(wide_c[:, 8:8 + N].cpu(), inp["want"]["c"])
            assert bool((wide_c[:, :8] == 77).all()) and bool((wide_c[:, 8 + N:] == 77).all())
        SEEN["persistent"][ran[0]] += 1


def test_persistent_row_slices_share_one_mask(ops):
    M, N, K, epi = 512, 512, 256, G.P8_EPILOGUES["bias+relu+drop"]
    inp, got, d = check_case(ops, "persistent", M, N, K, "unit", epi, 8, G.p8_symbol(8, 3))
    for cut in (256, 320):                                       # an aligned and a ragged pair of slices
        lo = dict(d, M=cut, a=d["a"][:cut])
        hi = dict(d, M=M - cut, a=d["a"][cut:])
        c_lo, ran_lo = launch(ops, lo, epi, 0)
        c_hi, ran_hi = launch(ops, hi, epi, 0, row_offset=cut)
        assert ran_lo[0].startswith("gemm8p_kernel<") and ran_hi[0].startswith("gemm8p_kernel<"), (ran_lo, ran_hi)
        assert torch.equal(torch.cat([c_lo["c"], c_hi["c"]]), got["c"]), cut


def test_row_offset_across_two_to_the_32(ops):
    """include/sfcvit.h makes row_offset a signed int32 and refuses no value; the kernels add it as an unsigned 32-bit number, so
    row_offset = -128 puts rows 0..127 at mask rows 2^32 - 128 .. 2^32 - 1 and rows 128..255 at 2^32 .. 2^32 + 127: the persistent
    kernel's second pre-hashed value (row >> 32 == 1 in epilogue_math).  It must store what the generic kernel, which hashes the
    whole 64-bit row, stores.  That the high word counts at all: rows 128..255 then draw flags independent of the ones rows 0..127
    draw at row_offset = 0 (mask rows 0..127), so about half of the 65 536 positions differ -- 0.25 is over 100 sigma below that."""
    M, N, K, epi = 256, 512, 256, G.P8_EPILOGUES["bias+drop+res"]
    inp = G.build_case(M, N, K, "unit", dict(bias=True, res=True), False)          # dropout aside: the kernels are compared
    d = dict(M=M, N=N, a=dev(inp["a"]), b=dev(inp["b"]), bias=dev(inp["bias"]), res=dev(inp["res"]))
    for mode in (8, 9, 10):
        p8, ran = launch(ops, d, epi, mode, row_offset=-128)
        again, _ = launch(ops, d, epi, mode, row_offset=-128)
        gen, ran_g = launch(ops, d, epi, 1, row_offset=-128)
        assert G.symbol_matches(G.p8_symbol(mode, 6), ran[0]) and ran_g == [G.generic_symbol(False, False)], (ran, ran_g)
        assert torch.equal(p8["c"], again["c"]) and torch.equal(p8["c"], gen["c"]), mode
        SEEN["persistent"][ran[0]] += 1
    at0, _ = launch(ops, d, epi, 8, row_offset=0)
    dropped_hi = p8["c"][128:] == d["res"][128:]                 # a dropped element stores the residual alone
    dropped_lo = at0["c"][:128] == d["res"][:128]
    assert 0.25 < float((dropped_hi != dropped_lo).float().mean()) < 0.75


# ---- weight-gradient kernel (gemm8p_km_kernel) -----------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", G.KM_MN)
@pytest.mark.parametrize("K,splitk,symbol", [k[:3] for k in G.KM_KS])
def test_weight_gradient_splits_and_tail_slab(ops, M, N, K, splitk, symbol):
    """fp32 C is the integer, bf16 C its round-to-nearest-even (ties included); the generic kernel on the same split stores the
    same bits; a one-hot A picks single rows of B."""
    for f32 in (True, False):
        inp, got, d = check_case(ops, "weight-gradient", M, N, K, "wide", {}, 0, symbol, akm=True, bkm=True, f32=f32, splitk=splitk)
        if not f32:
            assert G.count_ties(inp["want"]["v"].numpy()) > 0
        if splitk is not None:
            gen, ran = launch(ops, d, {}, 1, akm=True, bkm=True, f32=f32, splitk=splitk)
            assert ran == [G.generic_symbol(True, True)] and torch.equal(gen["c"], got["c"])
    a1, idx = G.one_hot_a(M, K)
    hot, ran = launch(ops, dict(d, a=dev(a1)), {}, 0, akm=True, bkm=True, splitk=splitk)
    assert G.symbol_matches(symbol, ran[0]) and torch.equal(hot["c"].cpu(), dev(inp["b"]).cpu().t()[idx])


def test_four_phase_schedule_of_the_persistent_kernels(ops, monkeypatch):
    """SFCVIT_GEMM_2PHASE=0 (csrc/dispatch.h, read per call) selects the other instantiation of both persistent kernels -- the
    `false` the `*` of the tables' symbols leaves open: the same exact answers, odd and even counts of k-tile pairs, a ragged M."""
    monkeypatch.setenv("SFCVIT_GEMM_2PHASE", "0")
    for mode in (8, 9, 10):
        for K in (256, 384):
            M = G.p8_epilogue_rows(mode)[1]
            check_case(ops, "persistent, four-phase", M, 512, K, "unit", G.P8_EPILOGUES["bias+res"], mode,
                       "gemm8p_kernel<%d, 4, false>" % (G.TILE_OF_MODE[mode] // 32))
    for M, N, K, splitk in ((256, 512, 384, 2), (256, 256, 1096, 3)):
        for f32 in (True, False):
            check_case(ops, "weight-gradient, four-phase", M, N, K, "wide", {}, 0, "gemm8p_km_kernel<false>", akm=True, bkm=True, f32=f32,
                       splitk=splitk)


# ---- ring kernel (gemm256_kernel) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.RING_MODES)
@pytest.mark.parametrize("akm,bkm", G.LAYOUTS)
def test_ring_shapes_and_layouts(ops, mode, akm, bkm):
    """K = 32 .. 256 (1, 3, 5, 8 stages of the 3- or 4-slot ring: the prologue issues min(slots, stages) and every wait counts the
    stages really in flight), M = 256 / 512, N = 128 / 256 / 384."""
    for i, (m, ka, kb, M, N, K, symbol) in enumerate(c for c in G.ring_cases() if c[:3] == (mode, akm, bkm)):
        check_case(ops, "ring", M, N, K, "unit", {}, mode, symbol, akm=akm, bkm=bkm, tag=i)


@pytest.mark.parametrize("M,N,K,splitk,what", G.RING_SPLIT_CASES)
def test_ring_split_k(ops, M, N, K, splitk, what):
    for akm, bkm in ((False, False), (True, True)):
        for f32 in (True, False):
            check_case(ops, "ring", M, N, K, "wide", {}, 4, G.ring_symbol(akm, bkm, 128), akm=akm, bkm=bkm, f32=f32, splitk=splitk)


@pytest.mark.parametrize("mode", (4, 7))
@pytest.mark.parametrize("M,N,K", G.RING_EPILOGUE_SHAPES)
def test_ring_epilogues(ops, mode, M, N, K):
    for i, epi in enumerate(G.RING_EPILOGUES.values()):
        check_case(ops, "ring", M, N, K, "unit", epi, mode, G.ring_symbol(False, False, G.ring_bn(mode, N)), f32=bool(epi.get("f32")), tag=i)


# ---- generic kernel (gemm_kernel) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", G.GEN_KS + (12,))
def test_generic_shapes_and_layouts(ops, K):
    """M = 1 .. 200, N = 4 .. 264 (the 4-column half vector, nvalid < 4 past the end), every layout the alignment rules allow."""
    for i, (akm, bkm, M, N, k, symbol) in enumerate(c for c in G.generic_cases() if c[4] == K):
        check_case(ops, "generic", M, N, K, "unit", {}, 1, symbol, akm=akm, bkm=bkm, tag=i)


@pytest.mark.parametrize("M,N,K,splitk,empty", G.GEN_SPLIT_CASES)
def test_generic_split_k_with_one_set_of_ranges_per_xcd(ops, M, N, K, splitk, empty):
    """Fewer than 64 output tiles: the split count is rounded up to a multiple of 8, so some ranges may be empty -- their slabs
    must be written (zeros) all the same."""
    for akm, bkm in G.LAYOUTS:
        for f32 in (True, False):
            check_case(ops, "generic", M, N, K, "wide", {}, 1, G.generic_symbol(akm, bkm), akm=akm, bkm=bkm, f32=f32, splitk=splitk)


@pytest.mark.parametrize("M,N,K", G.GEN_EPILOGUE_SHAPES + (G.GEN_BITS_SHAPE,))
def test_generic_epilogues(ops, M, N, K):
    for i, (name, epi) in enumerate(G.GEN_EPILOGUES.items()):
        if bool(epi.get("bits")) == ((M, N, K) == G.GEN_BITS_SHAPE):
            check_case(ops, "generic", M, N, K, "unit", epi, 1, G.generic_symbol(False, False), f32=bool(epi.get("f32")), tag=i)


# ---- GELU (HEAVY instantiations of the generic and ring kernels) -------------------------------------------------------------
@pytest.mark.parametrize("mode,M,N,K,symbol", G.GELU_CASES)
def test_gelu_epilogues(ops, mode, M, N, K, symbol):
    a, b8 = G.exact_inputs(M, N, K, "gelu")
    bias8 = torch.randint(-12, 13, (N,), generator=G._gen(5, N))
    pre_want, y_ref, floor = G.gelu_expect(a, b8, bias8)
    ad, bd, biasd = dev(a), dev(b8, 1 / 8), dev(bias8, 1 / 8)
    runs = [logged(ops, lambda: ops.gemm(ad, bd, bias=biasd, act=G.ACT_GELU, want_aux=True, force_generic=mode)) for _ in range(2)]
    torch.cuda.synchronize()
    (y, pre), ran = runs[0]
    assert ran == [symbol] and runs[1][1] == ran and torch.equal(y, runs[1][0][0]) and torch.equal(pre, runs[1][0][1])
    assert torch.equal(pre.cpu(), pre_want)                        # the pre-activation bit for bit
    ok, on_floor, worst = G.elementwise_verdict(y.cpu(), y_ref, floor)
    print(f"FIGURE gemm gelu fwd {symbol} ({M}, {N}, {K}): outside={int((~ok).sum())} floor_share={on_floor.mean():.4f} worst_of_floor={worst:.3f}")
    GELU_WORST[0] = max(GELU_WORST[0], worst)
    assert ok.all()
    SEEN["gelu"][ran[0]] += 1
    aux, _, _ = G.gelu_expect(*G.exact_inputs(M, N, K, "gelu", tag=1), bias8)
    for ds in G.GELU_DS:
        v, ref, fl = G.gelu_dx_expect(a, b8, aux, ds)
        runs = [logged(ops, lambda: ops.gemm(ad, bd, aux_in=aux.cuda(), dact=G.ACT_GELU, dact_scale=ds, force_generic=mode)) for _ in range(2)]
        torch.cuda.synchronize()
        assert runs[0][1] == [symbol] and torch.equal(runs[0][0], runs[1][0])
        ok, on_floor, worst = G.elementwise_verdict(runs[0][0].cpu(), ref, fl)
        print(f"FIGURE gemm gelu dact ds={ds} {symbol} ({M}, {N}, {K}): outside={int((~ok).sum())} floor_share={on_floor.mean():.4f} "
              f"worst_of_floor={worst:.3f}")
        GELU_WORST[0] = max(GELU_WORST[0], worst)
        assert ok.all(), ds
        SEEN["gelu"][symbol] += 1


# ---- gemm_dx -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(G.DX_ROUTES))
def test_gemm_dx_routes(ops, route):
    """dX = dY W through the transposed W on the persistent or the ring kernel, and with W read k-major by the generic kernel:
    with and without residual, dact, column sums, bit mask."""
    M, K, N, symbol = G.DX_ROUTES[route]
    for i, (name, epi) in enumerate(G.DX_EPILOGUES.items()):
        check_case(ops, "gemm_dx " + route, M, N, K, "unit", epi, 0, symbol(epi), tag=i, dx=True,
                   fused=route == "persistent" and bool(epi.get("colsum")))
