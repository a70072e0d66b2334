"""The masked and the biased attention kernels (csrc/attention_masked.hip, csrc/attention_bias.hip) held to
tests/attn_masked_exact_ref.py, whose docstring describes the geometry and the five designs and which
tests/test_attn_masked_exact_ref_cpu.py qualifies without a GPU.

Every (case, design), at p = 0 and, where the case says so, p = 0.5: inputs built on the CPU, the reference's own claims asserted
on them (attn_exact_ref.proven), forward and backward run twice (the runs must agree bit for bit), the kernel symbols asserted,
then attn_masked_exact_ref.verdict -- the verdict the CPU test applies to its fp32 restatement and to every mutation of it:
  out, dV; dQ, dK of tie / tiec / demoted / hidden   bit for bit; where the expectation is zero, |got| <= attn_exact_ref.allow
  uniform                                           out, dV the exact sums rounded once; dK exactly 0; dQ one bf16 step + 2^-8
                                                    sum |terms| (attn_exact_ref.rounding_bound)
  lse                                               uniform: 1e-5 against log(count); the others: 4 x the worst error of the CPU's
                                                    fp32 restatement of m_run + logf(l) on the same inputs; the tiec rows the same
                                                    bar against c above the tie rows' fp64 lse
  a key no query sees (hidden design)               dK and dV rows exactly 0
  dTable                                            per bucket eps_exp2 A_t plus the leak; a bucket no pair uses exactly 0
No element is exempt and no case is skipped.  The keep bits are ops.dropout_mask's, rows (b H + h) N + q, which
test_dropout_mask_is_the_host_restatement pins to tests/drop_path_ref.dropout_keep element for element.
FIGURE lines per family when the module is done: cases and symbols, worst lse error (CPU restatement and GPU), residues where zero
was expected, the worst share of each bound used."""
import collections

import numpy as np
import pytest
import torch

import attn_exact_ref as R
import attn_masked_exact_ref as M
from drop_path_ref import dropout_keep, keep_flags

pytestmark = pytest.mark.gpu
BF16, F64 = torch.bfloat16, torch.float64
SYMBOLS = {"masked": ("attn_masked_fwd_kernel", "attn_masked_bwd_kv_kernel"), "bias": ("attn_bias_fwd_kernel", "attn_bias_bwd_kv_kernel")}
SEEN = collections.defaultdict(collections.Counter)              # family -> symbol -> runs
LSE = collections.defaultdict(lambda: [0.0, 0.0])                # family -> [CPU fp32 restatement's worst error, GPU worst error]
SHARE = collections.defaultdict(lambda: collections.defaultdict(float))      # family -> bound -> worst share used
RESIDUE = collections.defaultdict(lambda: [0, 0, 0, 0.0])        # family -> [zeros expected, above the leak, of those > 0, largest in ulps]
ZEROS = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, 0]))   # family -> output -> [zero expectations, elements]


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    for fam, syms in SEEN.items():
        print(f"FIGURE attn masked exact {fam}: {sum(syms.values())} runs; " + "; ".join(f"{s} x {n}" for s, n in sorted(syms.items())))
    for fam, (cpu, gpu) in LSE.items():
        print(f"FIGURE attn masked exact lse {fam}: select designs worst |err| CPU fp32 restatement {cpu:.3e}, GPU {gpu:.3e}")
    for fam, shares in SHARE.items():
        print(f"FIGURE attn masked exact bounds {fam}: worst share used " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(shares.items())))
    for fam, (zeros, above, positive, ulps) in RESIDUE.items():
        print(f"FIGURE attn masked exact residue {fam}: {zeros} elements expected 0 in the select designs, {above} hold more than the leak, "
              f"{positive} of those are positive, largest {ulps:.2f} fp32 ulps of sum |terms|")
    for fam, outs in ZEROS.items():
        print(f"FIGURE attn masked exact zero expectations {fam}: " + ", ".join(f"{n} {z / max(t, 1):.3f}" for n, (z, t) in sorted(outs.items())))


def keep_bits(ops, c, p):
    """The keys dropout keeps, from the library's own mask: rows (b H + h) N + query, columns = keys."""
    if p == 0:
        return None
    I, N = c["B"] * c["H"], c["N"]
    mask = ops.dropout_mask(I * N, N, p, M.SEED).float().cpu().view(I, N, N)
    assert set(mask.unique().tolist()) <= {0.0, 1.0 / (1.0 - p)}
    return mask > 0


def launchers(ops, c, p):
    """(forward, backward(out, lse, **kw)) of the case's family on the GPU."""
    qkv, dout = (t.cuda() for t in R.pack(c))
    H = c["H"]
    if c["family"] == "masked":
        holder = ops.AttentionMask(c["mask"])
        assert np.array_equal(holder.block_map.numpy(), M.block_map(c)[0])
        m, bm = holder.on("cuda")
        return (lambda: ops.attention_masked_fwd(qkv, H, m, bm, p, M.SEED, scale=M.SCALE),
                lambda out, lse, **kw: ops.attention_masked_bwd(qkv, out, lse, dout, H, m, bm, p, M.SEED, scale=M.SCALE, **kw))
    holder = ops.AttentionBiasIndex(c["index"], c["T"])
    assert np.array_equal(holder.block_map.numpy(), M.block_map(c)[0])
    table = c["table"].cuda()
    return (lambda: ops.attention_bias_fwd(qkv, H, table, holder, p, M.SEED, scale=M.SCALE),
            lambda out, lse, **kw: ops.attention_bias_bwd(qkv, out, lse, dout, H, table, holder, p, M.SEED, scale=M.SCALE, **kw))


def run(ops, c, p):
    """Forward and backward twice -> the outputs as fp64 [items, N, hd] (lse [items, N], dtable [H, T]), and the raw dqkv."""
    fam, D = c["family"], c["H"] * c["hd"]
    fwd, bwd = launchers(ops, c, p)
    (out, lse), (out2, lse2) = fwd(), fwd()
    assert ops.last_attn_kernel() == SYMBOLS[fam][0]
    SEEN[fam][ops.last_attn_kernel()] += 1
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "forward: two runs differ"
    r1, r2 = bwd(out, lse), bwd(out, lse)
    assert ops.last_attn_kernel() == SYMBOLS[fam][1]
    SEEN[fam][ops.last_attn_kernel()] += 1
    d1, d2 = (r1[0], r2[0]) if fam == "bias" else (r1, r2)
    assert torch.equal(d1, d2), "backward: two runs differ"
    got = {n: R.unpack(c, d1[..., i * D:(i + 1) * D].cpu()) for i, n in enumerate(("dq", "dk", "dv"))}
    got.update(out=R.unpack(c, out.cpu()), lse=lse.cpu().to(F64).view(c["B"] * c["H"], c["N"]))
    if fam == "bias":
        assert torch.equal(r1[1], r2[1]), "table gradient: two runs differ"
        got["dtable"] = r1[1].cpu().to(F64)
    return got, d1, (out, lse, bwd)


def note(c, e, got, fig, bar):
    fam = c["family"]
    for n in ("out", "dq", "dk", "dv"):
        z = ZEROS[fam][n]
        z[0] += int((e[n] == 0).sum())
        z[1] += e[n].numel()
    if c["design"] == "uniform":
        SHARE[fam]["uniform dQ rounding bound"] = max(SHARE[fam]["uniform dQ rounding bound"], fig["dq_share"])
        SHARE[fam]["uniform lse / 1e-5"] = max(SHARE[fam]["uniform lse / 1e-5"], fig["lse_err"] / 1e-5)
    else:
        LSE[fam][0], LSE[fam][1] = max(LSE[fam][0], bar / 4), max(LSE[fam][1], fig["lse_err"])
        r = RESIDUE[fam]
        for n in ("out", "dq", "dk", "dv"):
            at = (e[n] == 0) & (got[n].abs() > e["leak"][n])
            r[0] += int((e[n] == 0).sum())
            r[1] += int(at.sum())
            r[2] += int((got[n][at] > 0).sum())
            if bool(at.any()):
                r[3] = max(r[3], float((got[n][at].abs() / (2.0 ** -23 * e["terms_" + n][at]).clamp_min(1e-300)).max()))
    if fam == "bias":
        SHARE[fam]["dTable bound"] = max(SHARE[fam]["dTable bound"], fig["table_share"])
        SHARE[fam]["dTable |err| / A_t"] = max(SHARE[fam]["dTable |err| / A_t"], fig["table_ratio"])


@pytest.mark.parametrize("case,design", [pytest.param(case, d, id=M.case_id(case) + "-" + d) for case in M.CASES for d in M.DESIGNS])
def test_exact_answers(ops, case, design):
    c = M.build(case["family"], design, case["B"], case["H"], case["N"])
    bar = M.lse_bar(c)
    for p in M.ps_of(case):
        where = (M.case_id(case), design, p)
        e = M.expectation(c, keep_bits(ops, c, p), p)            # the select designs: attn_exact_ref.proven on these very inputs
        assert e["sums_exact"], where
        if design == "tie" and p == 0:                           # (with dropout one half is out of reach: the CPU test's docstring)
            share = M.nonzero_share(e)
            assert share >= 0.5, (where, "non-zero share of the dQ and dK expectations", share)
        got, _, _ = run(ops, c, p)
        bad, fig = M.verdict(c, e, got, bar)
        print(f"[attention masked exact] {where}: gain {c['gain']:g}, lse |err| {fig['lse_err']:.3e} (bar {bar:.3e}), zero expectations "
              + ", ".join(f"{n} {fig['zero_share_' + n]:.3f}" for n in ("out", "dv", "dk") + (() if design == "uniform" else ("dq",)))
              + (f", uniform dQ uses {fig['dq_share']:.3f} of its bound" if design == "uniform" else "")
              + (f", dTable worst |err| / A_t {fig['table_ratio']:.3e}, share of its bound {fig['table_share']:.3f}" if case["family"] == "bias" else ""))
        note(c, e, got, fig, bar)
        assert not bad, (where, bad)


@pytest.mark.parametrize("family,N,B", M.COLSUM_CASES)
def test_column_sums_are_the_sums_of_the_stored_dqkv(ops, family, N, B):
    """The tie design: the fp32 column sums against the fp64 sums of the dqkv the same call stored, up to what `allow` grants
    the rows (attn_exact_ref.colsum_tolerance, sums built from rounded values)."""
    c = M.build(family, "tie", B, 2, N)
    e = M.expectation(c, None, 0.0)
    _, d1, (out, lse, bwd) = run(ops, c, 0.0)
    res = bwd(out, lse, colsum=True)
    assert torch.equal(res[0], d1)
    cs = res[-1]
    ref = d1.to(F64).sum((0, 1)).cpu()
    diff = (cs.cpu().to(F64) - ref).abs()
    tol = R.colsum_tolerance(c, e, False)
    off = (diff > tol).nonzero().flatten().tolist()
    print(f"[attention masked exact] column sums {family} N={N}: worst |diff| {float(diff.max()):.3e}, worst share of the bar {float((diff / tol.clamp_min(1e-300)).max()):.3f}")
    assert not off, (family, N, len(off), [(i, float(cs[i]), float(ref[i]), float(tol[i])) for i in off[:8]])


@pytest.mark.parametrize("rows,cols", [(5, 7), (777, 770), (2 * 2 * 196, 196)])
def test_dropout_mask_is_the_host_restatement(ops, rows, cols):
    """ops.dropout_mask against tests/drop_path_ref.dropout_keep, the hash of csrc/device_common.h restated in numpy, element for
    element; the kept value is bf16(1 / (1 - p))."""
    for p in (0.1, 0.5):
        for seed in (M.SEED, 77):
            got = ops.dropout_mask(rows, cols, p, seed).cpu()
            want = torch.from_numpy(dropout_keep(seed, p, rows, cols))
            on = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).to(BF16)
            assert torch.equal(got, torch.where(want, on, torch.zeros((), dtype=BF16))), (rows, cols, p, seed, int(((got > 0) != want).sum()))
            assert np.array_equal(want[:, 0].numpy(), keep_flags(seed, p, rows))
