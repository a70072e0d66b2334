"""tests/attn_masked_exact_ref.py qualified without a GPU, for every (case, design, p) tests/test_attention_masked_exact_gpu.py runs.

Own claims   inputs survive bf16; attn_exact_ref.proven holds (exact sums, bf16-exact P and dS, the leak margins); the gain is the
             smallest that isolates the selected keys with the term included; the block-class, m_safe and wrapped-corner conditions
             hold on the map the library's own host code returns; every bucket's smallest non-zero term is >= 8 x its bound; at
             p = 0 at least half of the tie design's dQ and dK elements have a non-zero expectation.  (At p = 0.5 the expectation
             of that share is under one half with q = g (k_a + k_b), whatever the data: dS_b = -dS_a, so dQ is non-zero only where
             the two codes differ, half the columns, and a quarter of the rows lose both keys -- dQ <= 3/8, dK <= 1 - (5/8)^2,
             mean 0.49.  It is printed: 0.47 .. 0.57.)
Truth        plain fp64 softmax of scale q k^T + term with autograd agrees with the expectations up to the leak.
Restatement  an fp32 restatement of the kernels' order of operations -- block-wise online softmax over the visited blocks only,
             m_safe, no mask read in an all-zero block, P rounded to bf16 for P V, dS rounded after the scale, fp32 table terms
             summed per chunk of images, then over the chunks, then per bucket; accumulators that round to nearest and (N <= 320)
             that round down like tests/test_attn_exact_ref_cpu.py's mm_down -- meets attn_masked_exact_ref.verdict, the bars of
             the GPU test.
Mutations    each wrong kernel of MUTATIONS, stated as a change to what that restatement reads, fails the verdict wherever
             UNDETECTABLE does not name the reason why it cannot."""
import math

import numpy as np
import pytest
import torch

import attn_exact_ref as R
import attn_masked_exact_ref as M

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
BLK = M.BLK
PARAMS = [pytest.param(case, d, id=M.case_id(case) + "-" + d) for case in M.CASES for d in M.DESIGNS]


def built(case, design):
    return M.build(case["family"], design, case["B"], case["H"], case["N"])


@pytest.mark.parametrize("case,design", PARAMS)
def test_inputs_and_expectations_are_what_the_reference_says(case, design):
    c = built(case, design)
    for n in ("q", "k", "v", "do"):
        assert torch.equal(R.rb(c[n]), c[n]) and float(c[n].abs().max()) <= 128, n
    bmap, _, _ = M.block_map(c)
    M.geometry_claims(c, bmap)
    if design in M.SELECT:
        qs = c["q"] / c["gain"]
        assert R._off_mass(qs, c["k"], c["sel"], c["gain"], c["scale"], c["term"]) < R.MASS
        assert c["gain"] == 1.0 or R._off_mass(qs, c["k"], c["sel"], c["gain"] / 2, c["scale"], c["term"]) >= R.MASS
        assert c["gain"] <= 64.0
    else:
        count = c["sel"].sum(-1)
        assert bool(((count & (count - 1)) == 0).all()) and set(count.unique().tolist()) <= {4, 16, 128}
    for p in M.ps_of(case):
        keep = M.host_keep(c, p)
        e = M.expectation(c, keep, p)                            # select designs: attn_exact_ref.proven inside
        assert e["sums_exact"]
        if design == "tie":
            share = M.nonzero_share(e)
            print(f"[masked exact ref] {M.case_id(case)} p={p}: non-zero share of the tie design's dQ and dK expectations {share:.3f}")
            assert p > 0 or share >= 0.5, share
        if design == "uniform":
            assert float(e["dk"].abs().max()) == 0.0 and float((e["lse"] - torch.log(c["sel"].sum(-1).to(F64))).abs().max()) < 1e-14
        if design == "hidden":
            hid = M.unseen_keys(c)
            assert bool((hid.sum(-1) == 1).all()) and float(e["dk"][hid].abs().max()) == 0.0 and float(e["dv"][hid].abs().max()) == 0.0
        if design == "tiec":
            # without the c on the selected keys the others weigh e^c more: the tie twin's own leak, far under any lse bar
            shift = M.tiec_shift(c)
            assert float((e["lse"] - e["lse_tie"] - shift).abs().max()) <= math.exp(float(shift.max())) * R.MASS < 1e-6
        if case["family"] == "bias":
            assert torch.equal(e["dtable"][:, ~e["used"]], torch.zeros_like(e["dtable"][:, ~e["used"]]))
            if design in ("tie", "tiec"):
                margin = M.bucket_margin(c, e)
                assert margin >= 8.0, margin
                assert int((e["dtable"] != 0).sum()) >= e["dtable"].numel() // 32
            if design in ("demoted", "hidden"):
                assert float(e["dtable"].abs().max()) == 0.0 and float(e["A"].max()) == 0.0
        # against plain fp64 softmax attention and autograd: equal up to the off-selection mass
        t = R.truth(c, keep, p)
        sizes = dict(out=c["v"].abs().amax(), dq=e["gross_dq"], dk=e["gross_dk"], dv=e["terms_dv"])
        for n in ("out", "dq", "dk", "dv"):
            tol = e["leak"][n] + 2.0 ** -29 * sizes[n] + 1e-12
            assert bool(((t[n] - e[n]).abs() <= tol).all()), (n, p, float((t[n] - e[n]).abs().max()))
        assert float((t["lse"] - e["lse"]).abs().max()) < 1e-12


# ---- the kernels' order of operations in fp32 -----------------------------------------------------------------------------------
def r16(t):
    return t.to(BF16).to(F32)


def mma(acc, a, b, down, depth=32):
    """acc + a @ b as a chain of `depth`-deep fp32 accumulations; down: every inexact partial sum rounded down, not to nearest."""
    if not down:
        return acc + a @ b
    acc = acc.to(F64)
    for lo in range(0, a.shape[-1], depth):
        x = acc + a[..., lo:lo + depth].to(F64) @ b[..., lo:lo + depth, :].to(F64)
        y = x.to(F32)
        acc = torch.where(y.to(F64) > x, torch.nextafter(y, torch.full_like(y, -math.inf)), y).to(F64)
    return acc.to(F32)


def full(blocks, N):
    return torch.from_numpy(np.ascontiguousarray(blocks)).repeat_interleave(BLK, 0).repeat_interleave(BLK, 1)[:N, :N]


def bias_chunks(B, H, VB):
    """csrc/attention_bias.h, bias_chunks."""
    want = max(1, min(32, B, -(-2048 // (H * VB))))
    per = -(-B // want)
    return per, -(-B // per)


def kernel_view(c, bmap, keep):
    """What the kernels read: the term in fp32, the class of every block, the keep bits."""
    return dict(term=c["term"].to(F32).clone(), cls=bmap.copy(), keep=keep, stale=False, skip_chunk=None, drop_last=False)


def term_read(c, st):
    """The term as the block loop sees it: not read (0) in a block of the all-zero class."""
    N = c["N"]
    zero = full(st["cls"] == M.ZERO, N) if c["family"] == "masked" else torch.zeros(N, N, dtype=torch.bool)
    t = torch.where(zero[None], torch.zeros((), dtype=F32), st["term"])
    if st["stale"]:                                              # the registers still hold the mask of the block visited before
        nb = st["cls"].shape[0]
        for qb in range(nb):
            prev = None
            for kb in range(nb):
                if st["cls"][qb, kb] == M.ZERO and prev is not None:
                    width = min(BLK, N - kb * BLK)
                    t[:, qb * BLK:(qb + 1) * BLK, kb * BLK:kb * BLK + width] = st["term"][:, qb * BLK:(qb + 1) * BLK, prev * BLK:prev * BLK + width]
                if st["cls"][qb, kb] != M.SKIP:
                    prev = kb
    return t, full(st["cls"] != M.SKIP, N)


def restate_forward(c, st, p, down):
    q, k, v = (c[n].to(F32) for n in ("q", "k", "v"))
    I, N, hd = q.shape
    sc = torch.tensor(c["scale"], dtype=F32)
    term, visit = term_read(c, st)
    kk = st["keep"].to(F32) * (1.0 / (1.0 - p)) if p > 0 else None
    m = torch.full((I, N), -math.inf, dtype=F32)
    l = torch.zeros(I, N, dtype=F32)
    o = torch.zeros(I, N, hd, dtype=F32)
    for kb in range((N + BLK - 1) // BLK):
        rv = visit[:, kb * BLK]
        if not bool(rv.any()):
            continue
        ks = slice(kb * BLK, min(N, (kb + 1) * BLK))
        s = (q @ k[:, ks].transpose(1, 2)) * sc + term[:, :, ks]
        m_new = torch.maximum(m, s.amax(-1))
        m_safe = torch.where(m_new == -math.inf, torch.zeros_like(m_new), m_new)
        alpha = torch.exp(m - m_safe)
        pe = torch.exp(s - m_safe[..., None])
        l_new = l * alpha + pe.sum(-1)
        o_new = mma(o * alpha[..., None], r16(pe if kk is None else pe * kk[:, :, ks]), v[:, ks], down)
        m, l, o = torch.where(rv[None], m_new, m), torch.where(rv[None], l_new, l), torch.where(rv[None, :, None], o_new, o)
    return dict(out=r16(o * (1.0 / l)[..., None]), lse=m + torch.log(l))


def restate_backward(c, st, p, down, fwd):
    q, k, v, do = (c[n].to(F32) for n in ("q", "k", "v", "do"))
    I, N, hd = q.shape
    sc = torch.tensor(c["scale"], dtype=F32)
    term, visit = term_read(c, st)
    kk = st["keep"].to(F32) * (1.0 / (1.0 - p)) if p > 0 else torch.ones((), dtype=F32)
    pv = torch.exp((q @ k.transpose(1, 2)) * sc + term - fwd["lse"][..., None])
    pv = torch.where(visit[None], pv, torch.zeros((), dtype=F32))
    x = (do @ v.transpose(1, 2)) * kk - (do * fwd["out"]).sum(-1, keepdim=True)
    ds, pm = r16(pv * x * sc), r16(pv * kk)
    zero = torch.zeros(I, N, hd, dtype=F32)
    res = dict(dq=r16(mma(zero, ds, k, down)), dk=r16(mma(zero, ds.transpose(1, 2), q, down)), dv=r16(mma(zero, pm.transpose(1, 2), do, down)))
    if c["family"] == "bias":
        B, H, T = c["B"], c["H"], c["T"]
        g = (pv * x).reshape(B, H, N * N)
        per, chunks = bias_chunks(B, H, int((st["cls"] != M.SKIP).sum()))
        total = torch.zeros(H, N * N, dtype=F32)
        for ch in range(chunks):
            if ch == st["skip_chunk"]:
                continue
            part = torch.zeros(H, N * N, dtype=F32)
            for b in range(ch * per, min(B, (ch + 1) * per)):
                part = part + g[b]
            total = total + part
        flat = c["index"].reshape(-1).long()
        at = flat >= 0
        if st["drop_last"]:
            pos = torch.arange(N * N)
            last = torch.full((T,), -1, dtype=torch.long).scatter_reduce_(0, flat[at], pos[at], "amax")
            at = at & (pos != last[flat.clamp_min(0)])
        res["dtable"] = torch.zeros(H, T, dtype=F32).index_add_(1, flat[at], total[:, at])
    return res


def judge(c, e, got, bar):
    return M.verdict(c, e, {n: t.to(F64) for n, t in got.items()}, bar)[0]


@pytest.mark.parametrize("case,design", PARAMS)
def test_an_fp32_restatement_of_the_kernels_meets_the_gpu_verdict(case, design):
    c = built(case, design)
    bmap, _, _ = M.block_map(c)
    bar = M.lse_bar(c)
    for p in M.ps_of(case):
        keep = M.host_keep(c, p)
        e = M.expectation(c, keep, p)
        for down in (False, True) if c["N"] <= 320 else (False,):
            st = kernel_view(c, bmap, keep)
            fwd = restate_forward(c, st, p, down)
            got = dict(fwd, **restate_backward(c, st, p, down, fwd))
            bad = judge(c, e, got, bar)
            assert not bad, (p, down, bad)


# ---- mutations ------------------------------------------------------------------------------------------------------------------
def selected_blocks(c):
    """Blocks that hold selected pairs: of the first pair, of the last (the wrapped corner) and of one off the diagonal."""
    si, sj = c["sel"][0].nonzero(as_tuple=True)
    blocks = {(int(si[0]) // BLK, int(sj[0]) // BLK), (int(si[-1]) // BLK, int(sj[-1]) // BLK)}
    offd = (sj // BLK != si // BLK).nonzero()
    if offd.numel():
        blocks.add((int(si[offd[0]]) // BLK, int(sj[offd[0]]) // BLK))
    return sorted(blocks)


def m_transposed(c, st, p):
    st["term"] = st["term"].transpose(1, 2).contiguous()
    return [st]


def m_shifted(c, st, p):
    N = c["N"]
    st["term"] = st["term"][:, :, torch.arange(1, N + 1).clamp_max(N - 1)]
    return [st]


def m_finite_as_zero(c, st, p):
    st["term"] = torch.where(torch.isfinite(st["term"]), torch.zeros((), dtype=F32), st["term"])
    return [st]


def m_block_skipped(c, st, p):
    out = []
    for qb, kb in selected_blocks(c):
        s2 = dict(st, cls=st["cls"].copy())
        s2["cls"][qb, kb] = M.SKIP
        out.append(s2)
    return out


def m_skipped_visited(c, st, p):
    qb, kb = np.argwhere(st["cls"] == M.SKIP)[0]
    st["cls"][qb, kb] = M.ZERO
    return [st]


def m_stale(c, st, p):
    st["stale"] = True
    return [st]


def m_keep_column(c, st, p):
    st["keep"] = st["keep"][:, :, torch.arange(c["N"]) % BLK]
    return [st]


def m_keep_head(c, st, p):
    B, H, N = c["B"], c["H"], c["N"]
    st["keep"] = st["keep"].view(B, H, N, N)[:, :1].expand(B, H, N, N).reshape(B * H, N, N)
    return [st]


def m_drop_last(c, st, p):
    st["drop_last"] = True
    return [st]


def m_skip_chunk(c, st, p):
    st["skip_chunk"] = 1
    return [st]


MUTATIONS = {"the mask or index transposed": m_transposed, "the mask or index shifted by one column": m_shifted,
             "a finite value treated as 0": m_finite_as_zero, "one visited block skipped": m_block_skipped,
             "one skipped block visited as all-zero": m_skipped_visited, "the all-zero class read as mixed from a stale buffer": m_stale,
             "the dropout column taken relative to the block": m_keep_column, "the row of the keep key taken without the head": m_keep_head,
             "a bucket's last position left out of the sum": m_drop_last, "the second batch chunk left out": m_skip_chunk}


def undetectable(name, case, c, bmap, p):
    """None, or the reason this (case, design, p) cannot see the mutation."""
    design, family, N = c["design"], c["family"], c["N"]
    if name == "a finite value treated as 0" and design in ("tie", "hidden", "uniform"):
        return "the term holds 0 and -inf only"
    if name == "one skipped block visited as all-zero":
        if not bool((bmap == M.SKIP).any()):
            return "the map has no skipped block"
        if family == "bias":
            return "the bias map has no all-zero class: a visited block reads its index, and -1 hides every pair of it"
        if design != "uniform":
            return "the gain isolates the selected keys from every other key, hidden ones included: only the count (uniform) moves"
    if name == "the all-zero class read as mixed from a stale buffer" and not (family == "masked" and bool((bmap == M.ZERO).any())):
        return "the map has no all-zero block"
    if name == "the all-zero class read as mixed from a stale buffer" and design != "uniform" and N < 2 * BLK + M.WIDE - BLK + 1:
        return "N = 130: the plain rows' cyclic band of 128 hides the offsets -1 and -2 only, never a selected key; the count (uniform) moves"
    if name == "the dropout column taken relative to the block" and (p == 0 or N <= BLK):
        return "no dropout, or one block: key - k0 is the key"
    if name == "the row of the keep key taken without the head" and (p == 0 or c["H"] == 1):
        return "no dropout, or one head"
    if name in ("a bucket's last position left out of the sum", "the second batch chunk left out"):
        if family != "bias":
            return "no table"
        if design in ("demoted", "hidden"):
            return "every row has one key with P = 1: every table term is 0 (a demoted key read as hidden is invisible by design too)"
        if name == "the second batch chunk left out" and bias_chunks(c["B"], c["H"], int((bmap != M.SKIP).sum()))[1] < 2:
            return "one chunk"
    return None


@pytest.mark.parametrize("case,design", PARAMS)
def test_every_mutation_fails_the_bars_of_the_gpu_test(case, design):
    c = built(case, design)
    bmap, _, _ = M.block_map(c)
    bar = M.lse_bar(c)
    applied = 0
    for p in M.ps_of(case):
        keep = M.host_keep(c, p)
        e = M.expectation(c, keep, p)
        for name, fn in MUTATIONS.items():
            why = undetectable(name, case, c, bmap, p)
            if why is not None:
                continue
            if p == 0 and case["drop"] and "dropout" not in name and "keep" not in name and c["N"] > 320:
                continue                                         # the large cases: once, with dropout
            for st in fn(c, kernel_view(c, bmap, keep), p):
                fwd = restate_forward(c, st, p, False)
                bad = judge(c, e, fwd, bar)
                if not bad:                                      # the forward did not see it: the backward must
                    bad = judge(c, e, dict(fwd, **restate_backward(c, st, p, False, fwd)), bar)
                assert bad, (name, p, "passes the bars")
                applied += 1
    assert applied >= 2


def test_every_mutation_is_seen_by_some_case_of_each_family_it_applies_to():
    """The reasons of `undetectable` leave every mutation at least one (case, design, p) per family that has the feature."""
    for family, cases in (("masked", M.MASKED_CASES), ("bias", M.BIAS_CASES)):
        for name in MUTATIONS:
            if (family == "masked" and ("bucket" in name or "chunk" in name)) or (family == "bias" and ("stale" in name or "skipped block visited" in name)):
                continue
            seen = False
            for case in cases:
                if seen or case["N"] > 320:
                    continue
                for design in M.DESIGNS:
                    c = built(case, design)
                    bmap, _, _ = M.block_map(c)
                    seen |= any(undetectable(name, case, c, bmap, p) is None for p in M.ps_of(case))
            assert seen, (family, name)


# ---- the dropout mask restated on the host --------------------------------------------------------------------------------------
def test_dropout_keep_is_keep_flags_in_column_0_and_keeps_the_right_share():
    """tests/drop_path_ref.dropout_keep: column 0 is keep_flags (the restatement the DropPath tests already rest on), and over
    4096 x 770 elements the keep rate is 1 - p within 2e-3 (three standard deviations are 5e-4 at p = 0.1, 8e-4 at p = 0.5)."""
    from drop_path_ref import dropout_keep, keep_flags
    for seed in (M.SEED, 77, 0xFFFFFFFF):
        for p in (0.1, 0.5):
            keep = dropout_keep(seed, p, 4096, 770)
            assert keep.shape == (4096, 770) and keep.dtype == np.bool_
            assert np.array_equal(keep[:, 0], keep_flags(seed, p, 4096))
            assert abs(float(keep.mean()) - (1.0 - p)) <= 2e-3, (seed, p, float(keep.mean()))
    rows = np.array([5, 3, 2 ** 32 - 1], dtype=np.uint64)                        # row numbers, not a count
    assert np.array_equal(dropout_keep(9, 0.5, rows, 7)[:2], dropout_keep(9, 0.5, 6, 7)[[5, 3]])
    assert not np.array_equal(dropout_keep(9, 0.5, 64, 64), dropout_keep(10, 0.5, 64, 64))
