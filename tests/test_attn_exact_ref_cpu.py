"""tests/attn_exact_ref.py qualified without a GPU, for every (design, N, head dim, scale, p) tests/test_attention_exact_gpu.py
runs: what it calls exact is exact, what it bounds is bounded, and a miscounted key fails the bars of the GPU test.

Per case: inputs and expectations survive bf16; P, P keep / (1 - p) and dS are bf16-exact; every fp32 sum is a sum of integers
times one factor under 2^24; the off-selection mass is under 2^-30 at the gain used and not at half of it; the expectations are
fp64 softmax attention and its autograd gradient up to that mass; the leak is under 2^-12 of the smallest non-zero expectation;
an fp32 / bf16 restatement of the kernels' arithmetic (exp2 of scaled scores, P and dS rounded to bf16, fp32 sums, one bf16
rounding of each result) meets the verdict the GPU test applies -- and shows that "dQ = dK = 0 exactly" would be an over-claim
(the restatement's zeros are not zero); dropping a key, counting one twice or appending a zero padding key fails the bars."""
import ctypes
import math

import pytest
import torch

import attn_exact_ref as R

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LOG2E = torch.tensor(1.4426950408889634, dtype=F32)
CUS = 256                                                        # an MI355X; the GPU test reads the real count


def keep_for(c, seed=5):
    I, N = c["B"] * c["H"], c["N"]
    return torch.rand(I, N, N, generator=R._gen(seed, N, I)) < 0.5


def built(case, design):
    B, H = R.shape_of(case)
    return R.build(design, B, H, case["N"], case["hd"], case["scale"])


PARAMS = [pytest.param(c, d, id=R.case_id(c) + "-" + d) for c in R.CASES for d in R.DESIGNS]


def ps_of(case, design):
    return (0.0, R.DROP_P) if design == "ties" and case["drop"] else (0.0,)


@pytest.mark.parametrize("case,design", PARAMS)
def test_inputs_and_expectations_are_what_the_reference_says(case, design):
    c = built(case, design)
    for n in ("q", "k", "v", "do"):
        assert torch.equal(R.rb(c[n]), c[n]) and float(c[n].abs().max()) <= 128, n
    if design != "uniform":
        assert R._off_mass(c["q"] / c["gain"], c["k"], c["sel"], c["gain"], c["scale"]) < R.MASS
        assert c["gain"] == 1.0 or R._off_mass(c["q"] / c["gain"], c["k"], c["sel"], c["gain"] / 2, c["scale"]) >= R.MASS
    for p in ps_of(case, design):
        keep = keep_for(c) if p > 0 else None
        e = R.expect(c, keep, p)
        assert e["sums_exact"] and e["ds_exact"], (p, e["sums_exact"], e["ds_exact"])
        exact = ["out", "dv", "dk"] if design == "uniform" else ["out", "dv"] + (["dq", "dk"] if c["pow2"] else [])
        if design == "uniform" and not R.uniform_dv_exact(c["N"]):
            exact.remove("dv")
        for n in exact:
            if not (design == "uniform" and n == "dv"):                 # the uniform dV is P colsum(dO) rounded once
                assert torch.equal(R.rb(e[n]), e[n]), (n, p)
            nz = e[n][e[n] != 0].abs()
            if design != "uniform" and nz.numel():
                assert e["leak"][n] <= 2.0 ** -12 * float(nz.min()), (n, p, e["leak"][n], float(nz.min()))
                # element by element: leak and accumulation error stay under half a bf16 step (2^-10 just above a power of two)
                assert bool((R.allow(c, e, n) <= 2.0 ** -10 * e[n].abs())[e[n] != 0].all()), (n, p)
        # against plain fp64 softmax attention and autograd: equal up to the off-selection mass
        t = R.truth(c, keep, p)
        ex = R.expect(c, keep, p, rounded=False)
        sizes = dict(out=c["v"].abs().amax(), dq=ex["gross_dq"], dk=ex["gross_dk"], dv=ex["terms_dv"])
        for n in ("out", "dq", "dk", "dv"):
            tol = ex["leak"][n] + 2.0 ** -29 * sizes[n] + 1e-12
            assert bool(((t[n] - ex[n]).abs() <= tol).all()), (n, p, float((t[n] - ex[n]).abs().max()))
        if design == "uniform":
            assert float((t["lse"] - math.log(c["N"])).abs().max()) < 1e-14
        else:
            top = torch.where(c["sel"], c["scale"] * (c["q"] @ c["k"].transpose(1, 2)), torch.tensor(-math.inf, dtype=F64)).amax(-1)
            assert float((t["lse"] - top - torch.log(c["sel"].sum(-1).to(F64))).abs().max()) <= R.MASS


def mm_down(a, b, depth=32):
    """a @ b accumulated `depth` products at a time in fp32, every inexact partial sum rounded DOWN instead of to nearest --
    what the bf16 MFMA results of the GPU run look like (attn_exact_ref.allow)."""
    acc = torch.zeros(*a.shape[:-1], b.shape[-1], dtype=F64)
    for lo in range(0, a.shape[-1], depth):
        x = acc + a[..., lo:lo + depth].to(F64) @ b[..., lo:lo + depth, :].to(F64)
        y = x.to(F32)
        acc = torch.where(y.to(F64) > x, torch.nextafter(y, torch.full_like(y, -math.inf)), y).to(F64)
    return acc.to(F32)


def restate(c, keep, p, mm=torch.matmul):
    """The kernels' arithmetic in fp32 with their bf16 roundings (csrc/attention_seq.hip and attention_bwd_fused.hip; the other
    families differ in tiling and summation order, which these inputs do not see)."""
    f = lambda t: t.to(F32)                                              # noqa: E731
    r16 = lambda t: t.to(BF16).to(F32)                                   # noqa: E731
    q, k, v, do = (f(c[n]) for n in ("q", "k", "v", "do"))
    sc = torch.tensor(c["scale"], dtype=F32)
    c2 = sc * LOG2E
    kk = f(keep) * (1.0 / (1.0 - p)) if keep is not None else torch.ones(1, dtype=F32)
    s = q @ k.transpose(1, 2)                                            # integers
    mx = s.amax(-1, keepdim=True)
    pe = torch.exp2(s * c2 - mx * c2)
    l = pe.sum(-1, keepdim=True)
    out = r16(mm(r16(pe * kk), v) / l)
    lse = (mx * sc + torch.log(l)).squeeze(-1)
    pb = torch.exp2(s * c2 - (lse * LOG2E)[..., None])
    delta = (do * out).sum(-1, keepdim=True)
    dp = do @ v.transpose(1, 2)
    ds = r16(pb * (dp * kk - delta) * sc)
    pm = r16(pb * kk)
    return dict(out=out, lse=lse, dq=r16(mm(ds, k)), dk=r16(mm(ds.transpose(1, 2), q)), dv=r16(mm(pm.transpose(1, 2), do)))


# accumulators that round down: exact sums (uniform) do not round at all, and the cases above N = 320 add nothing but time
RESTATED = [pytest.param(c, d, down, id=R.case_id(c) + "-" + d + ("-down" if down else "-nearest")) for c in R.CASES for d in R.DESIGNS
            for down in (False, True) if not (down and (d == "uniform" or c["N"] > 320))]


@pytest.mark.parametrize("case,design,down", RESTATED)
def test_an_fp32_restatement_of_the_kernels_meets_the_gpu_verdict(case, design, down):
    """down: with accumulators that round inexact sums down.  Two terms that cancel then leave -ulp(term) where the expectation
    is zero -- far above the leak, which is why attn_exact_ref.allow grants an fp32 ulp of the terms per accumulation step."""
    c = built(case, design)
    for p in ps_of(case, design):
        keep = keep_for(c) if p > 0 else None
        e, got = R.expect(c, keep, p), restate(c, keep, p, mm_down if down else torch.matmul)
        if down and design == "ties" and (case["family"], c["N"]) == ("seq + fused", 196):
            at = (e["dq"] == 0) & (e["terms_dq"] > 0)
            assert float(got["dq"].to(F64)[at].abs().max()) > 100 * e["leak"]["dq"], "no residue where two terms cancel"
        assert float((got["lse"].to(F64) - e["lse"]).abs().max()) <= R.lse_bar(c)
        assert R.wrong(got["out"], e["out"], R.allow(c, e, "out")) == 0
        if design == "uniform":
            assert R.wrong(got["dk"], e["dk"], 0.0) == 0
            if R.uniform_dv_exact(c["N"]):
                assert R.wrong(got["dv"], R.rb(e["dv"]), 0.0) == 0
            d = (got["dq"].to(F64) - e["dq"]).abs()
            assert bool((d <= R.rounding_bound(got["dq"].to(F64), e["dq"], e["terms_dq"])).all())
            continue
        assert R.wrong(got["dv"], e["dv"], R.allow(c, e, "dv")) == 0
        for n in ("dq", "dk"):
            if c["pow2"]:
                assert R.wrong(got[n], e[n], R.allow(c, e, n)) == 0, (n, p)
            else:
                assert bool(((got[n].to(F64) - e[n]).abs() <= 2.0 ** -7 * e["terms_" + n] + R.allow(c, e, n)).all()), (n, p)
    if design == "onehot" and c["N"] >= 16 and not down:
        # the over-claim this file exists to catch: the expectation is zero, the arithmetic's answer is the leak
        assert float(e["dq"].abs().max()) == 0.0 and float(e["dk"].abs().max()) == 0.0
        assert float(got["dq"].abs().max()) > 0.0 and float(got["dq"].abs().max()) <= e["leak"]["dq"]


@pytest.mark.parametrize("N", sorted({c["N"] for c in R.CASES if R.uniform_dv_exact(c["N"])}))
def test_uniform_probability_rounds_the_same_way_under_the_kernels_errors(N):
    """P = exp2(-lse log2 e) with lse = logf(N) up to 4 ulp off still rounds to bf16(fp32(1 / N)) wherever the builder calls the
    uniform dV exact (elsewhere the GPU test bounds dV)."""
    want = torch.tensor(1.0 / N, dtype=F32).to(BF16)
    lse = torch.log(torch.tensor(float(N), dtype=F32))
    ulp = max(float(torch.nextafter(lse, lse + 1) - lse), 2.0 ** -24)
    for k in range(-4, 5):
        pv = torch.exp2(-((lse + k * ulp) * LOG2E))
        for shift in (-2, 0, 2):                                          # the hardware exp2 within 2 ulp as well
            got = (pv * (1 + shift * 2.0 ** -23)).to(BF16)
            assert torch.equal(got, want), (N, k, shift)


def mutation_positions(N):
    return sorted({j for j in (0, 15, 16, 31, 32, 63, 64, 191, 192, 255, 256, N // 2, N - 2, N - 1) if 0 <= j < N})


@pytest.mark.parametrize("case,design", PARAMS)
def test_a_miscounted_key_fails_the_bars_of_the_gpu_test(case, design):
    """One key dropped or counted twice, at every block boundary, changes lse by more than its bar or some element of out
    beyond bit equality (the leak at expected zeros), in every item.  One zero padding key with score 0: the uniform design sees
    it; one-hot and ties cannot (their maximum is g hd scale >= 8 above it), which is asserted too so that nobody relies on it."""
    c = built(case, design)
    N = c["N"]
    e = R.expect(c)
    bar = R.lse_bar(c)

    def seen(lse, out):
        by_lse = ((lse - e["lse"]).abs() > bar).any(-1)
        got = R.rb(out)
        by_out = R.off(got, e["out"], R.allow(c, e, "out")).flatten(1).any(-1)
        return by_lse | by_out

    for j in mutation_positions(N):
        if N > 1:
            assert bool(seen(*R.mutate(c, "drop", j)).all()), ("drop", j)
        assert bool(seen(*R.mutate(c, "twice", j)).all()), ("twice", j)
    pad = seen(*R.mutate(c, "pad", 0))
    if design == "uniform":
        assert bool(pad.all())
        lse, _ = R.mutate(c, "pad", 0)
        assert float((lse - e["lse"]).abs().min()) > 100 * bar            # about 1 / N against 1e-5
    elif N > 1:
        assert not bool(pad.any())


@pytest.mark.parametrize("N,which", [(N, w) for N, ws in R.MANY_ITEMS for w in ws])
def test_many_item_cases(N, which):
    """The persistent-backward cases (more items than CUs, one head): the same proofs for the ties design at p = 0 and 0.5, for
    the batch sizes of a 256-CU part.  The data depend on B, so the GPU test calls attn_exact_ref.proven on its own inputs as
    well, whatever the CU count."""
    B = R.many_items_b(CUS, which)
    c = R.build("ties", B, 1, N, 64)
    for p in (0.0, R.DROP_P):
        keep = keep_for(c) if p > 0 else None
        R.proven(c, R.expect(c, keep, p), p)
    first, last = c["sel"][0], c["sel"][-1]
    assert not torch.equal(first, last) and not torch.equal(c["k"][0], c["k"][-1])     # items have data of their own


FUSED_TIES = [pytest.param(c, id=R.case_id(c)) for c in R.CASES if c["family"] == "seq + fused" and c["N"] > 1]


@pytest.mark.parametrize("case", FUSED_TIES)
def test_only_a_sum_of_unrounded_ds_moves_the_column_sums(case):
    """The column sums of the ties design against the fp64 sums of the stored dqkv (attn_exact_ref.colsum_tolerance).  Sums built
    from rounded values -- the MFMA accumulators of dK and dV, sum_k (sum_q bf16(dS)) K, a pass over the stored tensor -- meet
    the exact bar.  scale sum_k (sum_q dS) K with dS summed before it is rounded, which is what attn_seq_bwd_fused_kernel does
    for the Q third, is another number: P = 1/2 (1 + eps) survives in it, so it is held to the bar with the exp2 term."""
    c = built(case, "ties")
    B, H, N, hd = c["B"], c["H"], c["N"], c["hd"]
    D = H * hd
    un = lambda t: t.to(F64).reshape(B, H, -1, hd).sum((0, 2)).reshape(D)                  # noqa: E731
    r16 = lambda t: t.to(BF16).to(F32)                                                     # noqa: E731
    moved = False
    for p in ps_of(case, "ties"):
        keep = keep_for(c) if p > 0 else None
        e, got = R.expect(c, keep, p), restate(c, keep, p)
        q, k, v, do = (c[n].to(F32) for n in ("q", "k", "v", "do"))
        sc = torch.tensor(c["scale"], dtype=F32)
        kk = keep.to(F32) * (1.0 / (1.0 - p)) if keep is not None else torch.ones(1, dtype=F32)
        pb = torch.exp2((q @ k.transpose(1, 2)) * (sc * LOG2E) - (got["lse"] * LOG2E)[..., None])
        dr = pb * ((do @ v.transpose(1, 2)) * kk - (do * got["out"]).sum(-1, keepdim=True))
        exact, loose = R.colsum_tolerance(c, e, False), R.colsum_tolerance(c, e, True)
        assert torch.equal(exact[D:], loose[D:])                          # only the Q third is granted more
        stored = torch.cat([un(got[n]) for n in ("dq", "dk", "dv")])
        rounded = torch.cat([un(sc * (r16(dr).sum(1, keepdim=True) @ k)), un(sc * (r16(dr).transpose(1, 2) @ q)),
                             un(r16(pb * kk).transpose(1, 2) @ do)])     # the accumulators before their one bf16 rounding
        assert bool(((rounded - stored).abs() <= exact).all()), p
        unrounded = un(sc * (dr.sum(1, keepdim=True) @ k))
        assert bool(((unrounded - stored[:D]).abs() <= loose[:D]).all()), p
        # it is another number than the sum of the rounded dS, by more than any leak: the error of P, not of the design
        moved |= bool(((unrounded - rounded[:D]).abs() > 100 * B * N * e["leak"]["dq"]).any())
    assert moved, "summing dS before rounding it left no trace"


def plan(B, N, H, hd, bwd, any_length, p):
    from sfcvit import _lib
    a = _lib.AttnArgs()
    a.qkv, a.out, a.lse, a.dout, a.dqkv, a.delta = (0x100000 * (i + 1) for i in range(6))   # checked, never read
    a.B, a.N, a.H, a.hd, a.scale, a.dropout_p = B, N, H, hd, hd ** -0.5, p
    buf = ctypes.create_string_buffer(96)
    rc = _lib.lib.sfcvit_attention_plan(ctypes.byref(a), int(bwd), int(any_length), buf, len(buf))
    return None if rc else buf.value.decode()


SWITCHES = ("SFCVIT_ATTN_WIDE_STREAM", "SFCVIT_ATTN_LONG", "SFCVIT_ATTN_BWD_FUSED", "SFCVIT_ATTN_DQSUM", "SFCVIT_ATTN_BWD_PERSIST")


@pytest.mark.parametrize("case", [pytest.param(c, id=R.case_id(c)) for c in R.CASES])
def test_the_symbols_the_gpu_test_expects_are_the_plans(case, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, val in case["env"].items():
        monkeypatch.setenv(name, val)
    B, H = R.shape_of(case)
    for p in (0.0, R.DROP_P):
        fwd, bwd = R.symbols(case["hd"], case["N"], p, case["env"], case["any_length"])
        assert plan(B, case["N"], H, case["hd"], False, case["any_length"], p) == fwd
        assert plan(B, case["N"], H, case["hd"], True, case["any_length"], p) == bwd
    assert (bwd is None) == (case["family"] == "wide, forward only")


def test_the_cases_reach_every_symbol_of_the_issue():
    seen = set()
    for c in R.CASES:
        for p in (0.0, R.DROP_P) if c["drop"] else (0.0,):
            seen.update(R.symbols(c["hd"], c["N"], p, c["env"], c["any_length"]))
    want = {"attn_seq_fwd_kernel<0, false>", "attn_seq_fwd_kernel<0, true>", "attn_seq_fwd_kernel<13, false>", "attn_seq_fwd_kernel<13, true>",
            "attn_seq_bwd_fused_kernel<0, false>", "attn_seq_bwd_fused_kernel<0, true>", "attn_seq_bwd_fused_kernel<13, false>",
            "attn_seq_bwd_fused_kernel<13, true>", "attn_seq_bwd_kv_kernel<0>", "attn_seq_bwd_kv_kernel<13>", "attn_long_fwd_kernel<0>",
            "attn_long_fwd_kernel<36>", "attn_long_bwd_kv_kernel", "attn_fwd_kernel", "attn_bwd_kv_kernel"}
    want |= {"attn_wide_%s_kernel<%d>" % (k, s) for k in ("fwd", "bwd_kv") for s in (2, 3, 4)}
    want |= {"attn_wide_stream_%s_kernel<%d>" % (k, s) for k in ("fwd", "bwd_kv") for s in (2, 4)}
    assert want <= seen, sorted(want - seen)
    assert R.wide_max_n(128, True) == 256 and R.wide_max_n(192, True) == 192 and (R.wide_max_n(256, False), R.wide_max_n(256, True)) == (160, 128)
