"""Exact-answer inputs for the attention kernels that add a term to the score -- csrc/attention_masked.hip (an fp32 mask [N, N])
and csrc/attention_bias.hip (table[h, index[i, j]]) -- and their fp64 expectations.  CPU only.  Built on tests/attn_exact_ref.py:
the arithmetic is attn_exact_ref.expect with c["term"], the bars are its `allow`, `proven`, `off`, `wrong`, `rounding_bound` and
`eps_exp2`.  The claims made here are proven by tests/test_attn_masked_exact_ref_cpu.py and asserted on the GPU by
tests/test_attention_masked_exact_gpu.py.

Fixed: head dim 64, scale 1/8 (a power of two: dQ and dK are bit-exact), dropout p = 0.5 (1 / (1 - p) = 2 is exact).

Geometry.  Row i sees the cyclic band (j - i) mod N in [0, w_i].  w_i is the case's narrow width (15; 3 at N = 5 and 70, where a
wider band would leave no row of the tail block unwrapped) -- except, in the masked family from N = 130 up, the first 64 rows:
they are PLAIN rows with w_i = 127, zero on every visible pair in every design, so that block (0, 1) of the map is all zero.  The
other rows are the VARIANT rows of the design.  The two keys a row selects are the cyclic shifts a(i) = (i + s1) mod N and
b(i) = (i + s2) mod N, 0 <= s1 < s2 <= w: permutations, so every key serves at most two queries.

Designs (q_i = g (k_a + k_b) over +-1 codes except in `uniform`; k, v, dO are the same in the four of them, the gain is each one's own):
  tie      the term is 0 on both selected keys: P = 1/2, 1/2.
  tiec     the same integer c on both (3 in the mask; 3 + head + row class parity in the table): P is unchanged, lse moves by
           exactly c.  Catches a finite value treated as 0 or as "visible".
  demoted  -64 on b (on a instead in the odd rows of the mask and in the table of an odd head): P = 1 on the other key, e^-64 on
           the demoted one -- below the leak.
  hidden   -inf (index -1) on b: P = 1 on a.  One key column, N - 2, is hidden from EVERY row as well (the row that would select
           it as a selects b alone): its dK and dV rows are exactly 0.  A term read transposed or a row / column off shows the
           hidden key (P = 1/2) or hides the selected one.
  uniform  q = 0, the term in {0, -inf}: every row sees w_i + 1 = 4, 16 or 128 keys with P = 1 / count, a power of two that bf16
           holds, so no N needs excluding.  v and dO are small integers: the sums behind out and dV are exact in fp32 and the
           kernel's one bf16 rounding is the reference's (rb); dK = 0 exactly; dQ rounds dS and gets `rounding_bound`.  (The
           zero-sum v of attn_exact_ref's uniform design needs rows that see every key; bounded integers serve here.)

Gain: the smallest power of two <= 64 that leaves less than 2^-30 outside the selected keys of every row, the term included.

Bias family.  index[i, j] = offset * R + (i mod R) for the visible pairs (offset = (j - i) mod N, R row classes), -1 elsewhere: a
bucket holds one offset of N / R rows, so that no bucket sums so many terms that a missing one hides under its bound
(`bucket_margin`).  Expected dTable[h, t] = sum over images and the pairs of bucket t of P (keep dP - delta), no scale factor: a
sum of dyadic numbers, exact in fp64.  The kernel forms P in fp32 and never rounds the term to bf16, so a bucket is held to
eps_exp2(e) A_t (A_t = sum |terms|) plus what the off-selection probability can add (the leak); a bucket no pair uses to 0."""
import ctypes
import math

import numpy as np
import torch

import attn_exact_ref as R
from drop_path_ref import dropout_keep

F64, F32 = torch.float64, torch.float32
HD, SCALE, DROP_P, SEED = 64, 0.125, 0.5, 4242
BLK, WIDE, DEMOTE, C_TIE = 64, 127, -64.0, 3.0
NEG = -math.inf
DESIGNS = ("tie", "tiec", "demoted", "hidden", "uniform")
SELECT = DESIGNS[:4]
SKIP, MIXED, ZERO = 0, 1, 2                                      # the masked block map; the bias map has 0 and 1
ROW_CLASSES = {5: 5, 70: 14, 130: 13, 197: 16, 1024: 12}         # bias family: R per N (1024: 85 positions per bucket, two trips of a wave)


def _case(family, N, B, H, drop):
    return dict(family=family, N=N, B=B, H=H, drop=drop)


MASKED_CASES = [_case("masked", N, 1 if N == 2116 else 2, 1 if N == 2116 else 2, N in (5, 130, 196, 2116)) for N in (5, 64, 70, 130, 196, 257, 2116)]
BIAS_CASES = [_case("bias", 5, 2, 2, False), _case("bias", 70, 2, 2, True), _case("bias", 130, 2, 2, False), _case("bias", 197, 2, 2, True),
              _case("bias", 1024, 1, 2, True), _case("bias", 70, 40, 2, True)]
CASES = MASKED_CASES + BIAS_CASES
COLSUM_CASES = (("masked", 196, 2), ("bias", 197, 2))            # (family, N, B) of the two column-sum checks (tie design)


def case_id(case):
    return "%s-N%d-B%d" % (case["family"], case["N"], case["B"])


def ps_of(case):
    return (0.0, DROP_P) if case["drop"] else (0.0,)


def narrow_width(N):
    return 3 if N in (5, 70) else 15


def geometry(family, N):
    """-> dict: w [N] (band width per row), plain [N] bool, off [N, N] = (j - i) mod N, visible [N, N], a, b [N], s1, s2, jstar."""
    w = narrow_width(N)
    s1, s2 = (1, 3) if w == 3 else (2, 15)                       # s2 = w: a term read one column off loses b at the band's edge
    i = torch.arange(N)
    wi = torch.full((N,), w)
    if family == "masked" and N >= 130:
        wi[:BLK] = WIDE
    off = (i[None, :] - i[:, None]) % N
    return dict(w=wi, plain=wi != w, off=off, visible=off <= wi[:, None], a=(i + s1) % N, b=(i + s2) % N, s1=s1, s2=s2, jstar=N - 2, narrow=w)


def bias_index(N, design):
    """(index [N, N] int32, T, R) of the bias family: offset * R + row class on the visible pairs, -1 elsewhere."""
    g = geometry("bias", N)
    Rr = ROW_CLASSES[N]
    i = torch.arange(N)
    index = torch.where(g["visible"], g["off"] * Rr + (i % Rr)[:, None], torch.tensor(-1)).to(torch.int32)
    if design == "hidden":
        index = index.clone()
        hide_a = g["a"] == g["jstar"]
        index[i[~hide_a], g["b"][~hide_a]] = -1
        index[:, g["jstar"]] = -1
    return index.contiguous(), (g["narrow"] + 1) * Rr, Rr


def bias_table(N, H, design):
    """fp32 [H, T]: 0 everywhere but on the buckets of the two selected offsets."""
    g = geometry("bias", N)
    _, T, Rr = bias_index(N, design)
    table = torch.zeros(H, T, dtype=F32)
    cls = torch.arange(Rr)
    for h in range(H):
        if design == "tiec":
            for s in (g["s1"], g["s2"]):
                table[h, s * Rr + cls] = (C_TIE + h + (cls % 2)).to(F32)
        elif design == "demoted":
            table[h, (g["s1"] if h % 2 else g["s2"]) * Rr + cls] = DEMOTE
    return table


def build(family, design, B, H, N):
    """-> the dict attn_exact_ref.expect takes (q, k, v, do, sel, term [items, N, N], gain, scale, pow2, ...) and the family's
    additive input: mask (fp32 [N, N]) or index (int32 [N, N]), table (fp32 [H, T]), T."""
    I = B * H
    geo = geometry(family, N)
    g = R._gen(N, I, 7 if family == "bias" else 3)
    rows = torch.arange(N)
    a, b, plain, jstar = geo["a"], geo["b"], geo["plain"], geo["jstar"]
    k = R.ints(0, 1, (I, N, HD), g) * 2 - 1
    gram = k @ k.transpose(1, 2)
    assert bool((gram - HD * torch.eye(N, dtype=F64) < HD).all()), "sign codes are not distinct"
    v = R.ints(1, 7, (I, N, HD), g)
    do = torch.zeros(I, N, HD, dtype=F64)
    cols = torch.rand(I, N, HD, generator=g).argsort(-1)[..., :3]
    do.scatter_(-1, cols, R.ints(-2, 2, (I, N, 3), g, nonzero=True))
    c = dict(family=family, design=design, B=B, H=H, N=N, hd=HD, scale=SCALE, pow2=True, gain=1.0, geo=geo, table_terms=family == "bias")

    # the additive term, one [N, N] per head
    if family == "masked":
        t = torch.where(geo["visible"], 0.0, NEG).to(F64)
        var = rows[~plain]
        if design == "tiec":
            t[var, a[var]] = C_TIE
            t[var, b[var]] = C_TIE
        elif design == "demoted":                                # b in the even rows, a in the odd ones (one column off: a is no longer demoted)
            ev, od = var[var % 2 == 0], var[var % 2 == 1]
            t[ev, b[ev]] = DEMOTE
            t[od, a[od]] = DEMOTE
        elif design == "hidden":
            t[var, b[var]] = NEG
            t[:, jstar] = NEG
            i1 = rows[a == jstar]
            assert not bool(plain[i1].any()) and not bool(plain[rows[b == jstar]].any())
            t[i1, b[i1]] = 0.0
        c["mask"] = t.to(F32)
        assert torch.equal(c["mask"].to(F64), t)
        per_head = t[None].expand(H, N, N)
    else:
        index, T, _ = bias_index(N, design)
        table = bias_table(N, H, design)
        c.update(index=index, table=table, T=T)
        ix = index.long()
        per_head = torch.where(ix >= 0, table.to(F64)[:, ix.clamp_min(0)], torch.tensor(NEG, dtype=F64))
    term = per_head[None].expand(B, H, N, N).reshape(I, N, N)
    c["term"] = term

    if design == "uniform":
        gu = R._gen(N, I, 11)
        c.update(q=torch.zeros(I, N, HD, dtype=F64), k=k, v=R.ints(-3, 3, (I, N, HD), gu, nonzero=True),
                 do=R.ints(-4, 4, (I, N, HD), gu, nonzero=True), sel=torch.isfinite(term))
        return c
    # the selection: both keys where the term leaves them equal, else the key the term does not push down
    ta, tb = term[:, rows, a], term[:, rows, b]                  # [I, N]
    sel = torch.zeros(I, N, N, dtype=torch.bool)
    sel[:, rows, a] = ta >= tb
    sel[:, rows, b] = tb >= ta
    qs = k[:, a] + k[:, b]
    gain = 1.0
    while R._off_mass(qs, k, sel, gain, SCALE, term) >= R.MASS:
        gain *= 2.0
        assert gain <= 64.0, "no gain up to 64 isolates the selected keys"
    c.update(q=gain * qs, k=k, v=v, do=do, sel=sel, gain=gain)
    return c


def tie_lse(c):
    """fp64 lse of the same q and k under the tie design's term (0 on the band): what the tiec rows sit c above."""
    t = torch.where(c["geo"]["visible"], 0.0, NEG).to(F64)
    out = torch.empty(c["q"].shape[:2], dtype=F64)
    for lo in range(0, c["q"].shape[0], R.CHUNK):
        sl = slice(lo, lo + R.CHUNK)
        out[sl] = torch.logsumexp(c["scale"] * (c["q"][sl] @ c["k"][sl].transpose(1, 2)) + t, -1)
    return out


def tiec_shift(c):
    """[items, N]: the c of every row of a tiec case (0 on the plain rows)."""
    rows = torch.arange(c["N"])
    return c["term"][:, rows, c["geo"]["a"]]


# ---- the block maps, from the library's own host code -------------------------------------------------------------------------
def block_map(c):
    """The map sfcvit_attention_mask_blocks / sfcvit_attention_bias_blocks returns for the case's mask or index: numpy uint8
    [nb, nb] (masked: 0 skip, 1 mixed, 2 all zero; bias: 0 skip, 1 visited) -- and for the bias family offsets, positions."""
    from sfcvit._lib import lib
    N = c["N"]
    nb = (N + BLK - 1) // BLK
    out = np.full((nb, nb), 7, dtype=np.uint8)
    if c["family"] == "masked":
        m = np.ascontiguousarray(c["mask"].numpy(), dtype=np.float32)
        rc = lib.sfcvit_attention_mask_blocks(ctypes.c_void_p(m.ctypes.data), N, ctypes.c_void_p(out.ctypes.data))
        assert rc == 0, lib.sfcvit_last_error().decode()
        return out, None, None
    ix = np.ascontiguousarray(c["index"].numpy(), dtype=np.int32)
    offsets, positions = np.zeros(c["T"] + 1, dtype=np.int32), np.zeros(N * N, dtype=np.int32)
    rc = lib.sfcvit_attention_bias_blocks(ctypes.c_void_p(ix.ctypes.data), N, c["T"], ctypes.c_void_p(out.ctypes.data),
                                          ctypes.c_void_p(offsets.ctypes.data), ctypes.c_void_p(positions.ctypes.data))
    assert rc == 0, lib.sfcvit_last_error().decode()
    return out, offsets, positions[:offsets[-1]]


def geometry_claims(c, bmap):
    """The conditions the cases are chosen for, asserted on the library's map (every design of a case has the same band)."""
    N, geo = c["N"], c["geo"]
    nb = (N + BLK - 1) // BLK
    vis = torch.isfinite(c["term"][0])
    rows = torch.arange(N)
    blocks = torch.from_numpy(bmap.astype(np.int64))
    expanded = blocks.repeat_interleave(BLK, 0).repeat_interleave(BLK, 1)[:N, :N]
    assert bool((expanded[vis] != SKIP).all()), "a visible pair lies in a skipped block"
    if N >= 130:
        want = {SKIP, MIXED, ZERO} if c["family"] == "masked" else {0, 1}
        assert set(np.unique(bmap).tolist()) == want, (np.unique(bmap), want)
    if N >= 1024:                                                # the limits: a band of at most four blocks per row
        assert int((blocks != SKIP).sum(1).max()) <= 4
    if nb < 2:
        return
    # per row block: the first visited key block; per key block: the first visited row block
    first_k = torch.tensor([int((blocks[qb] != SKIP).nonzero()[0]) for qb in range(nb)])
    first_q = torch.tensor([int((blocks[:, kb] != SKIP).nonzero()[0]) for kb in range(nb)])
    sel = c["sel"][0]
    si, sj = sel.nonzero(as_tuple=True)
    assert bool((sj // BLK != first_k[si // BLK]).any()), "every selected pair lies in its row's first visited block"
    assert bool((sj < si).any()), "no selected pair in the wrapped corner"
    # m_safe: a row without a key in the first block its workgroup visits (its keys come later)
    in_first = torch.stack([vis[i, first_k[i // BLK] * BLK:(first_k[i // BLK] + 1) * BLK].any() for i in rows])
    assert bool((~in_first).any()), "no row starts empty: the m_safe path is not run"
    # and the other way round: in the first row block a key block's workgroup visits, a row that sees none of its keys
    sees = [vis[first_q[kb] * BLK:(first_q[kb] + 1) * BLK, kb * BLK:(kb + 1) * BLK].any(1) for kb in range(nb)]
    assert any(bool((~s).any()) for s in sees), "every row of a key block's first visited row block sees it"


# ---- dropout ------------------------------------------------------------------------------------------------------------------
def host_keep(c, p, seed=SEED):
    """bool [items, N, N] from the host restatement of the mask: rows (b H + h) N + q, columns = keys."""
    if p == 0:
        return None
    I, N = c["B"] * c["H"], c["N"]
    return torch.from_numpy(dropout_keep(seed, p, I * N, N)).view(I, N, N)


# ---- expectations and the verdict both tests apply ------------------------------------------------------------------------------
def expectation(c, keep, p):
    e = R.expect(c, keep, p)
    if c["design"] in SELECT:
        R.proven(c, e, p)
    if c["family"] == "bias":
        e.update(table_sums(c, e["g"], e["g_leak"]))
    if c["design"] == "tiec":
        e["lse_tie"] = tie_lse(c)
    return e


def table_sums(c, g, g_leak):
    """dtable, A (sum |terms|) and leak per bucket, fp64 [H, T], and used [T] bool."""
    B, H, N, T = c["B"], c["H"], c["N"], c["T"]
    flat = c["index"].reshape(-1).long()
    at = flat >= 0
    res = {}
    for name, t in (("dtable", g), ("A", g.abs()), ("table_leak", g_leak)):
        per_head = t.reshape(B, H, N * N).sum(0)
        res[name] = torch.zeros(H, T, dtype=F64).index_add_(1, flat[at], per_head[:, at])
    used = torch.zeros(T, dtype=torch.bool)
    used[flat[at]] = True
    res["used"] = used
    return res


def table_bound(c, e):
    return R.eps_exp2(e) * e["A"] + e["table_leak"]


def bucket_margin(c, e):
    """Smallest over the buckets of (smallest non-zero |term| of the bucket) / (its bound): the CPU test wants >= 8."""
    B, H, N, T = c["B"], c["H"], c["N"], c["T"]
    flat = c["index"].reshape(-1).long()
    at = (flat >= 0)[None, None].expand(B, H, N * N)
    mag = e["g"].abs().reshape(B, H, N * N)
    nz = at & (mag > 0)
    big = torch.where(nz, mag, torch.tensor(math.inf, dtype=F64)).amin(0)           # [H, N N]
    smallest = torch.full((H, T), math.inf, dtype=F64).scatter_reduce_(1, flat.clamp_min(0)[None].expand(H, -1), big, "amin")
    has = torch.isfinite(smallest)
    if not bool(has.any()):
        return math.inf
    return float((smallest[has] / table_bound(c, e)[has]).min())


def nonzero_share(e):
    """Share of the dQ and dK elements whose expectation is not zero."""
    return float(((e["dq"] != 0).sum() + (e["dk"] != 0).sum())) / (e["dq"].numel() + e["dk"].numel())


def unseen_keys(c):
    """[items, N] bool: keys no query sees."""
    return ~torch.isfinite(c["term"]).any(1)


def lse_restated(c):
    """Worst |error| against fp64 of the fp32 restatements of the kernels' lse = m_run + logf(l) on a select case: m the row's
    largest score scale * s + term (s an integer, the products exact), l = sum exp(score - m) over the visible keys, the last
    step with and without a fused multiply-add of the scale -- the rule of attn_exact_ref.lse_fp32_error."""
    worst = 0.0
    sc32 = torch.tensor(c["scale"], dtype=F32)
    for lo in range(0, c["q"].shape[0], R.CHUNK):
        sl = slice(lo, lo + R.CHUNK)
        raw = c["q"][sl] @ c["k"][sl].transpose(1, 2)
        want = torch.logsumexp(c["scale"] * raw + c["term"][sl], -1)
        t32 = c["term"][sl].to(F32)
        for s32 in (raw.to(F32) * sc32 + t32, (raw * c["scale"] + c["term"][sl]).to(F32)):
            m = s32.amax(-1)
            l = torch.exp(s32 - m[..., None]).sum(-1)
            plain = m + torch.log(l)
            fused = (m.to(F64) + torch.log(l).to(F64)).to(F32)
            worst = max(worst, float((plain.to(F64) - want).abs().max()), float((fused.to(F64) - want).abs().max()))
    return worst


def lse_bar(c):
    """uniform: 1e-5 against log(count); the other designs: 4 x the fp32 restatement's worst error on the same inputs."""
    return 1e-5 if c["design"] == "uniform" else 4.0 * lse_restated(c)


def verdict(c, e, got, bar):
    """What the GPU test asserts of a kernel and the CPU test of its restatement.  got: out, dq, dk, dv fp64 [items, N, hd], lse
    [items, N], and for the bias family dtable [H, T].  -> (failures: list of strings, figures: dict)."""
    bad, fig = [], {}
    uniform = c["design"] == "uniform"
    zeros = lambda n: torch.zeros_like(e[n]) if uniform else R.allow(c, e, n)      # noqa: E731
    want = {n: (R.rb(e[n]) if uniform and n in ("out", "dv") else e[n]) for n in ("out", "dq", "dk", "dv")}
    for n in ("out", "dv", "dk") + (() if uniform else ("dq",)):
        if n not in got:                                         # a forward-only verdict (the CPU test's mutations)
            continue
        w = R.wrong(got[n], want[n], zeros(n))
        if w:
            at = R.off(got[n], want[n], zeros(n)).nonzero()[:4].tolist()
            bad.append("%s: %d of %d elements wrong, first %s" % (n, w, got[n].numel(), [(i, float(got[n][tuple(i)]), float(want[n][tuple(i)])) for i in at]))
        fig["zero_share_" + n] = float((want[n] == 0).sum()) / want[n].numel()
    if uniform and "dq" in got:
        share = float(((got["dq"] - e["dq"]).abs() / R.rounding_bound(got["dq"], e["dq"], e["terms_dq"])).max())
        fig["dq_share"] = share
        if share > 1.0:
            bad.append("dq: %.3f of the rounding bound" % share)
        if float(got["dk"].abs().max()) != 0.0:
            bad.append("dk: not exactly 0")
    err = float((got["lse"] - e["lse"]).abs().max())
    fig["lse_err"] = err
    if not err <= bar:
        bad.append("lse: |err| %.3e over the bar %.3e" % (err, bar))
    if c["design"] == "tiec":
        err = float((got["lse"] - (e["lse_tie"] + tiec_shift(c))).abs().max())
        if not err <= bar:
            bad.append("lse: the tie + c rows sit %.3e off c above the tie rows (bar %.3e)" % (err, bar))
    hid = unseen_keys(c)
    for n in ("dk", "dv"):
        if n in got and bool(hid.any()) and float(got[n][hid].abs().max()) != 0.0:
            bad.append("%s: a key no query sees has a non-zero row" % n)
    if c["family"] == "bias" and "dtable" in got:
        d = (got["dtable"] - e["dtable"]).abs()
        bound = table_bound(c, e)
        over = d > bound
        if bool(over.any()):
            at = over.nonzero()[:4].tolist()
            bad.append("dtable: %d buckets over their bound, first %s" % (int(over.sum()), [(i, float(got["dtable"][tuple(i)]), float(e["dtable"][tuple(i)]), float(bound[tuple(i)])) for i in at]))
        if bool((~e["used"]).any()) and float(got["dtable"][:, ~e["used"]].abs().max()) != 0.0:
            bad.append("dtable: a bucket no pair uses is not 0")
        has = e["A"] > 0
        fig["table_ratio"] = float((d[has] / e["A"][has]).max()) if bool(has.any()) else 0.0
        fig["table_share"] = float((d[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
    return bad, fig
