"""The unmasked attention kernels (csrc/attention_seq.hip, attention_bwd_fused.hip, attention_long.hip, attention.hip,
attention_wide.hip, attention_wide_stream.hip) held to tests/attn_exact_ref.py, whose docstring describes the three designs and
which tests/test_attn_exact_ref_cpu.py qualifies without a GPU.

Every case: inputs built on the CPU, the reference's own claims asserted on them before a kernel is looked at, forward and backward
run twice (the runs must agree bit for bit), the kernel symbol asserted, then
  out, dV, and dQ / dK of one-hot and ties   bit for bit; where the expectation is zero, |got| <= attn_exact_ref.allow: the fp64
                                             leak (about 2^-30 of the terms: the off-selection probability is small, not zero)
                                             and an fp32 ulp of the terms per MFMA step, which rounds inexact sums down
  lse                                        uniform: 1e-5 against log N; one-hot, ties: 4 x the worst error of the CPU's fp32
                                             restatement of mx * scale + logf(l) on the same inputs, against fp64
  dQ of uniform                              one bf16 step + 2^-8 sum |terms| (the bound of the kernel-roundings test)
  dQ, dK of ties at a scale that is no       one bf16 step (2^-7) of sum |terms|: attention_bwd_fused.hip rounds dS before the
  power of two (wide / stream, default)      scale, the other kernels after it
  column sums                                ties: the fp64 sums of the stored dqkv, up to what `allow` grants the rows; the Q
                                             third of the one-pass backward with in-kernel sums alone also gets the relative
                                             error of an fp32 exp2 times sum |terms| (it sums dS before rounding it:
                                             attn_exact_ref.colsum_tolerance); uniform, one-hot: the existing 1 / 100 bar; the
                                             bf16 slot is the fp32 result rounded
Where a zero is expected and something larger than the leak came back, the count, sign and size (in fp32 ulps of sum |terms|) are
kept per family.  The symbols seen, the worst lse errors and these residues are printed as FIGURE lines when the module is done."""
import collections
import os
import subprocess
import sys

import pytest
import torch

import attn_exact_ref as R
from test_kernels_gpu import attention_backward_roundings

pytestmark = pytest.mark.gpu
BF16, F64 = torch.bfloat16, torch.float64
SEED = 4242
SEEN = collections.defaultdict(collections.Counter)              # family -> symbol -> cases
LSE = collections.defaultdict(lambda: [0.0, 0.0])                # family -> [CPU fp32 restatement's worst error, GPU worst error]
DQ_SHARE = collections.defaultdict(float)                         # family -> worst share of the uniform dQ bound used
QSUM = collections.defaultdict(float)                            # family -> one-pass backward, in-kernel dQ sums: worst |diff| / exact bar
RESIDUE = collections.defaultdict(lambda: [0, 0, 0, 0.0])        # family -> [zeros expected, above the leak, of those > 0, largest in ulps]
SWITCHES = ("SFCVIT_ATTN_WIDE_STREAM", "SFCVIT_ATTN_LONG", "SFCVIT_ATTN_BWD_FUSED", "SFCVIT_ATTN_DQSUM", "SFCVIT_ATTN_BWD_PERSIST")


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    for fam, syms in SEEN.items():
        print(f"FIGURE attn exact {fam}: {sum(syms.values())} cases; " + "; ".join(f"{s} x {n}" for s, n in sorted(syms.items())))
    for fam, (cpu, gpu) in LSE.items():
        print(f"FIGURE attn exact lse {fam}: one-hot / ties worst |err| CPU fp32 restatement {cpu:.3e}, GPU {gpu:.3e}")
    for fam, share in DQ_SHARE.items():
        print(f"FIGURE attn exact uniform dQ {fam}: worst share of the bound {share:.3f}")
    for fam, share in QSUM.items():
        print(f"FIGURE attn exact column sums {fam}: Q third summed from un-rounded dS, worst |diff| / the bar of the rounded sums {share:.3f}")
    for fam, (zeros, above, positive, ulps) in RESIDUE.items():
        print(f"FIGURE attn exact residue {fam}: {zeros} elements expected 0 in one-hot / ties, {above} hold more than the leak, {positive} of those "
              f"are positive, largest {ulps:.2f} fp32 ulps of sum |terms|")


def note_residue(family, c, e, name, got):
    if got.numel() > 2 ** 20:                                    # the many-item cases: the small ones tell the same
        return
    at = (e[name] == 0) & (got.abs() > e["leak"][name])
    r = RESIDUE[family]
    r[0] += int((e[name] == 0).sum())
    r[1] += int(at.sum())
    r[2] += int((got[at] > 0).sum())
    if bool(at.any()):
        r[3] = max(r[3], float((got[at].abs() / (2.0 ** -23 * e["terms_" + name][at])).max()))


def keep_bits(ops, c, p):
    """The keys dropout keeps, from the library's own mask: rows (b H + h) N + query, columns = keys."""
    if p == 0:
        return None
    I, N = c["B"] * c["H"], c["N"]
    mask = ops.dropout_mask(I * N, N, p, SEED).float().cpu().view(I, N, N)
    assert set(mask.unique().tolist()) <= {0.0, 1.0 / (1.0 - p)}
    return mask > 0


def expectation(ops, c, p):
    keep = keep_bits(ops, c, p)
    e = R.expect(c, keep, p)
    if c["design"] == "uniform":                                 # dQ against the un-rounded 1 / N
        true = R.expect(c, keep, p, rounded=False)
        e["dq"], e["terms_dq"] = true["dq"], true["terms_dq"]
    else:
        R.proven(c, e, p)                                        # the margins behind "bit for bit", on these very inputs
    return e


def check(ops, c, p, family, scale, any_length, want_fwd, want_bwd, e=None):
    """One (design, p) of a case -> (dqkv, column sums) for the callers that compare launches."""
    B, H, N, hd, design = c["B"], c["H"], c["N"], c["hd"], c["design"]
    D = H * hd
    where = (family, design, N, hd, p)
    e = expectation(ops, c, p) if e is None else e
    assert e["sums_exact"] and e["ds_exact"], where              # the reference's claims, on these very inputs
    leak = e["leak"]
    qkv, dout = (t.cuda() for t in R.pack(c))
    kw = dict(scale=scale, any_length=any_length)

    (out, lse), (out2, lse2) = (ops.attention_fwd(qkv, H, p, SEED, **kw) for _ in range(2))
    ran = ops.last_attn_kernel()
    assert ran == want_fwd, (where, ran, want_fwd)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), ("run to run", where)
    SEEN[family][ran] += 1
    got_out = R.unpack(c, out.cpu())
    bad = R.wrong(got_out, e["out"], R.allow(c, e, "out"))
    if design != "uniform":
        note_residue(family, c, e, "out", got_out)
    assert bad == 0, (where, "out", f"{bad} of {out.numel()} elements wrong")
    err = float((lse.cpu().to(F64).view(B * H, N) - e["lse"]).abs().max())
    bar = R.lse_bar(c)
    if design != "uniform":
        LSE[family][0], LSE[family][1] = max(LSE[family][0], bar / 4), max(LSE[family][1], err)
    print(f"[attention exact] {where} {ran}: lse |err| {err:.3e} (bar {bar:.3e})")
    assert err <= bar, (where, "lse", err, bar)
    if want_bwd is None:
        with pytest.raises(Exception, match="LDS"):
            ops.attention_bwd(qkv, out, lse, dout, H, p, SEED, **kw)
        return None, None

    d1, d2 = (ops.attention_bwd(qkv, out, lse, dout, H, p, SEED, **kw) for _ in range(2))
    ran = ops.last_attn_kernel()
    assert ran == want_bwd, (where, ran, want_bwd)
    assert torch.equal(d1, d2), ("run to run", where)
    SEEN[family][ran] += 1
    got = {n: R.unpack(c, d1[..., i * D:(i + 1) * D].cpu()) for i, n in enumerate(("dq", "dk", "dv"))}
    def msg(n, bad, want=None):
        want = e[n] if want is None else want
        at = R.off(got[n], want, R.allow(c, e, n)).nonzero()[:6].tolist()
        return (where, n, f"{bad} of {got[n].numel()} elements wrong", leak[n], [(i, float(got[n][tuple(i)]), float(want[tuple(i)])) for i in at])

    if design == "uniform":
        assert R.wrong(got["dk"], e["dk"], 0.0) == 0, msg("dk", R.wrong(got["dk"], e["dk"], 0.0))
        if R.uniform_dv_exact(N):
            bad = R.wrong(got["dv"], R.rb(e["dv"]), 0.0)
            assert bad == 0, msg("dv", bad, R.rb(e["dv"]))
        else:
            assert bool(((got["dv"] - e["dv"]).abs() <= R.rounding_bound(got["dv"], e["dv"], e["terms_dv"])).all()), (where, "dv")
        share = float(((got["dq"] - e["dq"]).abs() / R.rounding_bound(got["dq"], e["dq"], e["terms_dq"])).max())
        DQ_SHARE[family] = max(DQ_SHARE[family], share)
        print(f"[attention exact] {where} {ran}: uniform dQ uses {share:.3f} of its bound")
        assert share <= 1.0, (where, "dq", share)
    else:
        for n in ("dq", "dk", "dv"):
            note_residue(family, c, e, n, got[n])
        bad = R.wrong(got["dv"], e["dv"], R.allow(c, e, "dv"))
        assert bad == 0, msg("dv", bad)
        for n in ("dq", "dk"):
            if c["pow2"]:
                bad = R.wrong(got[n], e[n], R.allow(c, e, n))
                assert bad == 0, msg(n, bad)
            else:                                                # the kernels differ in where they multiply by the scale
                off = (got[n] - e[n]).abs() > 2.0 ** -7 * e["terms_" + n] + R.allow(c, e, n)
                assert not bool(off.any()), msg(n, int(off.sum()))

    d3, cs = ops.attention_bwd(qkv, out, lse, dout, H, p, SEED, colsum=True, **kw)
    slot = torch.full((3 * D,), float("nan"), device="cuda", dtype=BF16)
    d4, cs2 = ops.attention_bwd(qkv, out, lse, dout, H, p, SEED, colsum=slot, **kw)
    assert torch.equal(d3, d1) and torch.equal(d4, d1) and cs2 is slot, where
    assert torch.equal(slot, cs.to(BF16)), (where, "bf16 slot")
    ref = d1.to(F64).sum((0, 1)).cpu()
    diff = (cs.cpu().to(F64) - ref).abs()
    if design == "ties" and c["pow2"]:
        in_kernel = want_bwd.startswith("attn_seq_bwd_fused_kernel") and not os.environ.get("SFCVIT_ATTN_DQSUM", "").startswith("p")
        tol = R.colsum_tolerance(c, e, unrounded_dq=in_kernel)
        if in_kernel:                                            # how far the sum of un-rounded dS is from the bar of the other sums
            exact = R.colsum_tolerance(c, e, unrounded_dq=False)[:D]
            QSUM[family] = max(QSUM[family], float((diff[:D] / exact.clamp_min(1e-30)).max()))
        off = (diff > tol).nonzero().flatten().tolist()
        assert not off, (where, "column sums", len(off), [(i, float(cs[i]), float(ref[i]), float(tol[i])) for i in off[:8]])
    else:
        tol = ref.abs() / 100 + ref.pow(2).mean().sqrt().clamp_min(1e-6) / 100
        assert bool((diff <= tol).all()), (where, "column sums", int((diff > tol).sum()))
    return d1, cs


def set_switches(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)


@pytest.mark.parametrize("case", [pytest.param(c, id=R.case_id(c)) for c in R.CASES])
def test_exact_answers(ops, case, monkeypatch):
    """All three designs at p = 0, ties also at p = 0.5 where the case says so (a ragged and a whole length per family)."""
    set_switches(monkeypatch, case["env"])
    B, H = R.shape_of(case)
    for design in R.DESIGNS:
        c = R.build(design, B, H, case["N"], case["hd"], case["scale"])
        for p in ((0.0, R.DROP_P) if design == "ties" and case["drop"] else (0.0,)):
            fwd, bwd = R.symbols(case["hd"], case["N"], p, case["env"], case["any_length"])
            check(ops, c, p, case["family"], case["scale"], case["any_length"], fwd, bwd)


# ---- the persistent backward with more items than CUs ---------------------------------------------------------------------------
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def fused_symbol(N, p):
    return R.symbols(64, N, p, {}, False)


def many_items(ops, N, B, setenv, per_item_too=True, ps=(0.0, R.DROP_P)):
    """The ties design at p = 0 and 0.5, every item bit-exact, with one workgroup per CU (B > CUs: the rolling prefetch of the next
    item runs) and with one workgroup per item; dqkv and the column sums of the two launches bit-identical."""
    c = R.build("ties", B, 1, N, 64)
    for p in ps:
        fwd, bwd = fused_symbol(N, p)
        res, e = {}, expectation(ops, c, p)
        for persist in ("1", "0") if per_item_too else ("1",):
            setenv("SFCVIT_ATTN_BWD_PERSIST", persist)
            res[persist] = check(ops, c, p, "fused, many items, SFCVIT_ATTN_BWD_PERSIST=" + persist, None, False, fwd, bwd, e)
        setenv("SFCVIT_ATTN_BWD_PERSIST", "1")
        if not per_item_too:
            continue
        assert torch.equal(res["1"][0], res["0"][0]), (N, B, p, "dqkv differs between one workgroup per CU and one per item")
        assert torch.equal(res["1"][1], res["0"][1]), (N, B, p, "column sums differ between one workgroup per CU and one per item")


@pytest.mark.parametrize("N,which", [(N, w) for N, ws in R.MANY_ITEMS for w in ws])
def test_persistent_backward_with_more_items_than_cus(ops, N, which, monkeypatch):
    B = R.many_items_b(cus(), which)
    if B > R.MAX_ITEMS:
        pytest.skip(f"B = {B} items for {cus()} CUs exceeds {R.MAX_ITEMS}")
    set_switches(monkeypatch, {})
    many_items(ops, N, B, monkeypatch.setenv)
    if (N, which) == (196, 3):
        g = torch.Generator(device="cuda").manual_seed(23)
        qkv = torch.randn(B, N, 192, device="cuda", generator=g).to(BF16)
        dout = torch.randn(B, N, 64, device="cuda", generator=g).to(BF16)
        attention_backward_roundings(ops, qkv, dout, 1, 0.1, 77)
        assert ops.last_attn_kernel() == "attn_seq_bwd_fused_kernel<13, true>"


def child():
    """SFCVIT_ATTN_BWD_QUEUE and SFCVIT_ATTN_NT are read once per process: the 2 cus + 37, N = 196 ties case in this process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "space-filling-curves-for-vision-transformers_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from sfcvit import ops
    assert os.environ.get("SFCVIT_ATTN_BWD_QUEUE") == "0" and os.environ.get("SFCVIT_ATTN_NT") == "1"
    B = R.many_items_b(cus(), 3)
    if B <= R.MAX_ITEMS:
        # the two switches concern the walk over items only; with dropout, the walk also stages the row keys of the next item
        many_items(ops, 196, B, os.environ.__setitem__, per_item_too=False, ps=(R.DROP_P,))
    print("child ok")


def test_fixed_item_stride_and_nontemporal_loads_in_a_fresh_process(ops):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(SFCVIT_ATTN_BWD_QUEUE="0", SFCVIT_ATTN_NT="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    child()
