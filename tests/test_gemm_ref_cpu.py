"""Qualifies tests/gemm_ref.py without a GPU: (1) the magnitude bounds its docstring states hold at every exact case, on the
reference alone; (2) fp32 a @ b^T is the int64 product there, i.e. the answers are independent of the summation order;
(3) expect() agrees with a plain torch fp64 restatement of the epilogue order; (4) bf16 ties exist and round to even; (5) every
mutant -- an fp32 restatement of a wrong kernel, judged by the bit-for-bit verdict of tests/test_gemm_exact_gpu.py -- is rejected
at every case it applies to; (6) the kernel symbols parse and their MASK values are the P8_* bits of csrc/dispatch.h and the
instantiations of csrc/gemm8p.hip; (7) the GELU floors hold for an fp32 restatement of the epilogue and reject the tanh form."""
import math
import os
import re

import numpy as np
import pytest
import torch

import gemm_ref as G

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "space-filling-curves-for-vision-transformers_amd", "csrc")
CASES = G.all_exact_cases()


def fused(family, epi):
    """Column sums come out of the persistent kernel's epilogue (csrc/dispatch.cpp plan_p8: CSUM only with DACT)."""
    return family in ("p8", "dx-persistent") and bool(epi.get("colsum")) and epi.get("dact") == G.ACT_RELU


# ---- the fp32 restatement of the kernels, with its mutants ---------------------------------------------------------------
def truncate_bf16(v32):
    return (v32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(G.BF16)


def kernel32(inp, epi, out_f32, keep, family, extra, mutant=None):
    """fp32 math in the documented order on the bf16 inputs; -> the dict gemm_ref.stored() describes."""
    a, b = inp["a"].float(), inp["b"].float()
    M, K = a.shape
    N = b.shape[0]
    acc = a @ b.t()
    if mutant == "drop_one_k":
        k = int(((a != 0).any(0) & (b != 0).any(0)).nonzero()[-1])      # the last k that reaches any output
        acc = acc - torch.outer(a[:, k], b[:, k])
    elif mutant in ("drop_last_8", "drop_last_64", "drop_last_128"):
        n = int(mutant.rsplit("_", 1)[1])
        acc = acc - a[:, K - n:] @ b[:, K - n:].t()
    elif mutant == "tail_slab_left_out":
        acc = acc - a[:, K - extra["tail"]:] @ b[:, K - extra["tail"]:].t()
    elif mutant == "empty_split_unzeroed":
        acc = acc + 1.0                                              # a slab nobody wrote holds whatever was there: say ones
    elif mutant == "last_row_from_prev":
        acc = acc.clone()
        acc[M - 1] = acc[M - 2]
    elif mutant == "frag_transposed":
        acc = acc.clone()
        acc[:16, :16] = acc[:16, :16].t().clone()
    v = acc
    if epi.get("bias") and not (mutant == "bias_with_dact" and epi.get("dact")):
        v = v + inp["bias"].float()
    pre = v.to(G.BF16)
    if epi.get("act") == G.ACT_RELU:
        v = v.clamp_min(0.0)
    before_drop = v
    if mutant == "res_before_drop":
        v = v + inp["res"].float()
    if epi.get("drop"):
        k = torch.roll(keep, 2, dims=1) if mutant == "keep_shifted" else keep
        v = torch.where(k, v * 2.0, torch.zeros_like(v))
    if epi.get("res") and mutant not in ("res_before_drop", "res_after_dact"):
        v = v + inp["res"].float()
    if epi.get("dact") == G.ACT_RELU:
        v = torch.where(inp["aux"].float() > 0, v * float(epi.get("ds", 1.0)), torch.zeros_like(v))
    if mutant == "res_after_dact":
        v = v + inp["res"].float()
    rnd = truncate_bf16 if mutant == "truncation" else (lambda t: t.to(G.BF16))
    c = v if out_f32 else rnd(v)
    out = dict(c=c)
    if epi.get("aux"):
        out["pre"] = pre
    if epi.get("colsum"):
        rows = v if fused(family, epi) else c.float()
        s = rows.sum(0)
        if mutant == "overlap_rows_twice":
            t = extra["tile"]
            s = s + rows[M - t:(M - 1) // t * t].sum(0)
        out["colsum"], out["colsum_bf16"] = s, rnd(s)
    if epi.get("bits") and epi.get("act") == G.ACT_RELU:
        out["bits"] = G.pack_bits((before_drop if mutant == "bits_before_dropout" else c.float()) > 0)
    return out


def rounds_away(v64):
    """Some entry is stored with a larger magnitude than it has: what truncation would get wrong."""
    return bool((G.round_bf16(v64.numpy()).double().abs() > v64.abs()).any())


MUTANTS = {     # name -> (what wrong kernel it stands for, the cases it applies to)
    "drop_one_k": ("one k index left out of the contraction", lambda c: True),
    "drop_last_8": ("the last 16-byte vector of k left out", lambda c: c["K"] >= 8),
    "drop_last_64": ("the last k-tile left out", lambda c: c["K"] >= 64),
    "drop_last_128": ("the last pair of k-tiles left out", lambda c: c["K"] >= 128),
    "last_row_from_prev": ("an edge row taken from its neighbour", lambda c: c["M"] >= 2),
    "frag_transposed": ("one 16 x 16 accumulator fragment stored transposed", lambda c: c["M"] >= 16 and c["N"] >= 16),
    "overlap_rows_twice": ("the rows the overlapping last tile shares summed twice in the fused column sums",
                           lambda c: fused(c["family"], c["epi"]) and c["M"] % c["extra"]["tile"] != 0),
    "res_before_drop": ("the residual added before the dropout", lambda c: c["epi"].get("drop") and c["epi"].get("res")),
    "res_after_dact": ("the residual added after dact instead of being scaled and masked by it", lambda c: c["epi"].get("res") and c["epi"].get("dact")),
    "bias_with_dact": ("a launch with dact treated as bias-free (the persistent DACT variants are) although a bias was given",
                       lambda c: c["epi"].get("bias") and c["epi"].get("dact")),
    "keep_shifted": ("keep flags of the neighbouring column pair", lambda c: c["epi"].get("drop")),
    "bits_before_dropout": ("the bit mask taken from the value before the dropout",
                            lambda c: c["epi"].get("bits") and c["epi"].get("drop") and c["epi"].get("act") == G.ACT_RELU),
    "truncation": ("bf16 by truncation", lambda c: not c["f32"] and (rounds_away(c["want"]["v"]) or (
        c["epi"].get("colsum") and rounds_away(c["want"]["colsum" if fused(c["family"], c["epi"]) else "colsum_c"])))),
    "tail_slab_left_out": ("the K % 128 tail slab of the weight-gradient kernel left out", lambda c: c["extra"].get("tail", 0) > 0),
    "empty_split_unzeroed": ("the slab of an empty split-K range summed without having been written", lambda c: bool(c["extra"].get("empty"))),
}


def walk_cases():
    for i, (family, akm, bkm, M, N, K, kind, epi, f32, sym, extra) in enumerate(CASES):
        keep = G.synthetic_keep(M, N, i) if epi.get("drop") else None
        inp = G.build_case(M, N, K, kind, epi, f32, keep=keep, tag=i)
        yield dict(family=family, M=M, N=N, K=K, kind=kind, epi=epi, f32=f32, sym=sym, extra=extra, keep=keep, inp=inp, want=inp["want"])


# ---- 1, 2, 4, 5: one walk over every exact case ---------------------------------------------------------------------------
def test_bounds_order_independence_and_mutants_at_every_exact_case():
    applied = {m: 0 for m in MUTANTS}
    ties, missed, int64_done = 0, [], set()
    for c in walk_cases():
        inp, want, epi = c["inp"], c["want"], c["epi"]
        where = (c["family"], c["M"], c["N"], c["K"], sorted(epi))
        a, b = inp["a"], inp["b"]
        # (1) the stated bounds, on the reference alone
        if c["kind"] == "unit":
            assert int(a.abs().max()) <= 1 and int(b.abs().max()) <= 2 and G.bf16_exact_bound(want), where
        else:
            assert int(a.abs().max()) <= 4 and int(b.abs().max()) <= 4 and 16 * c["K"] < 2 ** 24, where
        assert float(want["v"].abs().max()) < 2 ** 24 and float(want["colsum"].abs().max()) < 2 ** 24, where
        # (2) fp32 a @ b^T is the integer product: against fp64 (exact below 2^53) everywhere, against int64 as far as that is quick
        acc32 = a.float() @ b.float().t()
        assert torch.equal(acc32.double(), want["acc"]), where
        shape = (c["kind"], c["M"], c["N"], c["K"])
        if c["M"] * c["N"] * c["K"] <= 1 << 22 or shape not in int64_done:    # int64 is slow: once per shape above 4 M products,
            int64_done.add(shape)                                               # and there on every step-th row (all of B and k)
            step = max(1, c["M"] * c["N"] * c["K"] >> 28)
            assert torch.equal(a[::step] @ b.t(), want["acc"][::step].long()), where
        # the unmutated restatement is what expect() says, bit for bit
        st = G.stored(want, epi, fused(c["family"], epi))
        assert G.exact_verdict(kernel32(inp, epi, c["f32"], c["keep"], c["family"], c["extra"]), st) == [], where
        # (4) ties
        if c["kind"] == "wide" and not c["f32"]:
            n = G.count_ties(want["v"].numpy())
            assert n > 0, where
            ties += n
            at = torch.from_numpy(np.mod(np.abs(want["v"].numpy()), G.bf16_step(want["v"].numpy())) == G.bf16_step(want["v"].numpy()) / 2)
            assert int((want["c"].view(torch.int16)[at] & 1).sum()) == 0, where                    # even mantissa
        # (5) the mutants
        for name, (_, applies) in MUTANTS.items():
            if applies(c):
                applied[name] += 1
                bad = G.exact_verdict(kernel32(inp, epi, c["f32"], c["keep"], c["family"], c["extra"], mutant=name), st)
                if not bad:
                    missed.append((name, where))
    assert not missed, missed
    print(f"{len(CASES)} exact cases, {ties} bf16 ties; mutants applied and rejected: {applied}")
    assert all(n > 0 for n in applied.values()), applied


def test_unit_sums_at_the_listed_shapes_and_the_zero_share():
    for M, N, K in ((512, 1792, 256), (448, 512, 1024), (256, 7936, 256), (1001, 512, 896)):
        a, b = G.exact_inputs(M, N, K, "unit")
        acc = a.double() @ b.double().t()
        zero = float((acc == 0).double().mean())
        print(f"unit ({M}, {N}, {K}): max |sum| {int(acc.abs().max())}, {zero:.2%} exactly 0")
        assert float(acc.abs().max()) < 256 and 0.005 < zero < 0.04


def test_wide_products_are_exact_in_fp32_up_to_k_4168():
    a, b = G.exact_inputs(256, 512, 4168, "wide")
    acc = a.double() @ b.double().t()
    assert torch.equal((a.float() @ b.float().t()).double(), acc) and torch.equal(a @ b.t(), acc.long())
    odd = ((acc.abs() >= 256) & (acc.abs() < 512) & (acc.long() % 2 == 1)).sum()
    assert int(odd) > 1000


# ---- 3. expect() against a plain restatement of the order ----------------------------------------------------------------
@pytest.mark.parametrize("name,epi", list(G.P8_EPILOGUES.items()) + list(G.GEN_EPILOGUES.items()) + list(G.RING_EPILOGUES.items()))
def test_expectation_follows_the_documented_order(name, epi):
    M, N, K = 72, 48, 40
    keep = G.synthetic_keep(M, N, 3)
    inp = G.build_case(M, N, K, "unit", epi, bool(epi.get("f32")), keep=keep, tag=3)
    v = torch.zeros(M, N, dtype=torch.float64)
    for k in range(K):                                               # sum_k A(m, k) B(n, k), one k at a time
        v += inp["a"][:, k, None].double() * inp["b"][None, :, k].double()
    if epi.get("bias"):
        v += inp["bias"].double()[None, :]
    pre = v.clone()
    if epi.get("act") == G.ACT_RELU:
        v = torch.relu(v)
    if epi.get("drop"):
        v = v * keep.double() / (1 - G.DROP_P)
    if epi.get("res"):
        v += inp["res"].double()
    if epi.get("dact"):
        v = v * (inp["aux"] > 0).double() * epi["ds"]
    want = inp["want"]
    assert torch.equal(want["v"], v) and torch.equal(want["pre"].double(), pre)
    assert torch.equal(want["c"].double(), v if epi.get("f32") else v.to(torch.float32).to(G.BF16).double())
    assert torch.equal(want["colsum"], v.sum(0))
    bits = want["bits"]
    for n in (0, 7, 8, 47):
        assert torch.equal((bits[:, n >> 3] >> (n & 7)) & 1, (want["c"][:, n] > 0).to(torch.uint8))


# ---- 6. symbols ----------------------------------------------------------------------------------------------------------
def test_symbols_parse_and_masks_are_the_dispatch_bits():
    with open(os.path.join(CSRC, "dispatch.h")) as f:
        header = f.read()
    bits = dict(re.findall(r"P8_([A-Z]+) = (\d+)", header))
    assert {k: int(v) for k, v in bits.items()} == G.P8_BITS
    consts = dict(re.findall(r"constexpr int (P8_LDS_BIAS|P8_LDS_MAX) = ([0-9 +*]+);", header))
    assert (eval(consts["P8_LDS_MAX"]) - eval(consts["P8_LDS_BIAS"])) // 2 == G.BIAS_MAX_N      # digits, + and * only (the regex)
    assert 7936 <= G.BIAS_MAX_N < 8192
    with open(os.path.join(CSRC, "gemm8p.hip")) as f:
        built = re.findall(r"case ([A-Z0 |]+): return launch<NI", f.read())
    built = {sum(G.P8_BITS[w] for w in re.findall(r"[A-Z]+", expr)) for expr in built}
    assert built == set(G.P8_MASKS) == {G.mask_of(e) for e in G.P8_EPILOGUES.values()}            # every instantiated variant has a case
    for case in CASES:
        sym = case[9]
        assert G.SYMBOL_RE.match(sym), sym
        m = re.match(r"gemm8p_kernel<(\d), (\d+), ", sym)
        if m:
            assert int(m.group(2)) in G.P8_MASKS and int(m.group(2)) == G.mask_of(case[7]) and 32 * int(m.group(1)) == case[10]["tile"]
    assert G.symbol_matches("gemm8p_kernel<7, 12, *>", "gemm8p_kernel<7, 12, true>")
    assert not G.symbol_matches("gemm8p_kernel<7, 12, *>", "gemm8p_kernel<7, 1, true>")
    assert not G.symbol_matches(G.KM_SYMBOL, "gemm8p_kernel<8, 0, true>")


def test_the_automatic_split_of_the_weight_gradient_cases():
    from sfcvit import ops
    for M, N in G.KM_MN:
        assert ops.auto_splitk(M, N, 4168) == 1                      # K / s >= 512 fails for every s the tile count allows


# ---- 7. GELU floors --------------------------------------------------------------------------------------------------------
def gelu_erf32(x):
    return 0.5 * x * (1 + torch.erf(x * 0.70710678118654752))


def gelu_erf_grad32(x):
    return 0.5 * (1 + torch.erf(x * 0.70710678118654752)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


@pytest.mark.parametrize("mode,M,N,K,sym", G.GELU_CASES)
def test_gelu_floors_hold_for_the_fp32_epilogue_and_reject_the_tanh_form(mode, M, N, K, sym):
    a, b8 = G.exact_inputs(M, N, K, "gelu")
    bias8 = torch.randint(-12, 13, (N,), generator=G._gen(5, N))
    pre, y_ref, floor = G.gelu_expect(a, b8, bias8)
    span = float(pre.float().abs().max())
    assert 8 <= span < 32
    y32 = gelu_erf32(pre.float()).to(G.BF16)
    ok, on_floor, worst = G.elementwise_verdict(y32, y_ref, floor)
    assert ok.all()       # (no bound on the share resting on the floor: every pre-activation below about -4 does, by cancellation)
    tanh = torch.nn.functional.gelu(pre.float(), approximate="tanh").to(G.BF16)
    ok_t, on_t, _ = G.elementwise_verdict(tanh, y_ref, floor)
    assert not ok_t.all()
    aux, _, _ = G.gelu_expect(*G.exact_inputs(M, N, K, "gelu", tag=1), bias8)
    worsts = [worst]
    for ds in G.GELU_DS:
        v, ref, fl = G.gelu_dx_expect(a, b8, aux, ds)
        dx32 = (v.float() * gelu_erf_grad32(aux.float()) * ds).to(G.BF16)        # v * gelu_erf_grad(a) * ds, as gemm_core.h forms it
        ok, on_floor, worst = G.elementwise_verdict(dx32, ref, fl)
        assert ok.all(), ds
        worsts.append(worst)
        half = (v.float() * gelu_erf_grad32(aux.float()) * (ds / 2)).to(G.BF16)  # a forgotten factor of two
        assert not G.elementwise_verdict(half, ref, fl)[0].all()
    print(f"gelu fp32 restatement ({M}, {N}, {K}): |pre| up to {span}, worst |err| / floor {max(worsts):.3f}")
    assert math.isfinite(max(worsts))
