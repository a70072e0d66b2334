"""The tokenizer kernels on the GPU, one by one: the fused gather + projection kernels (pe_fwd_kernel, pe_bwd_kernel,
pe_bwd_reduce), their tiled forms (pe2_*), the general per-pixel gather, the fused hierarchical tokenizer in both forms and
the resample + concatenate pair.

Reference: the fp64 statements of tests/tokenizer_ref.py on the CPU, written from include/sfcvit.h, on the SAME values the
device gets.  Three kinds of test (the construction of test_token_mix_gpu.py):

    exact answers    small integers and weights in halves (conditions checked without a GPU in test_tokenizer_ref_cpu.py):
                     every partial sum is exact in fp32, so the kernel must return the round-to-nearest-even of the exact
                     result, bit for bit, in every element.  In fp32 images a fixed share of the pixels sits 2^-10 + 2^-13
                     below its integer, which rounds to the integer but truncates to the bf16 value below it.
    format bounds    bf16-rounded normals:
                       bf16 outputs     |err| <= 2^-8 |ref| + (K + 1) 2^-23 sum |terms|
                       fp32 dW, dbias   |err| <= R 2^-24 sum |terms|, R = B * N rows summed
                       fused y          judged against Wf . h_device + bf on the h the kernel returned (h itself is judged
                                        by the first bound): a rounding flip in h does not leak into the bar for y
                       resampling       forward: one bf16 rounding of the two-tap value with fp32 taps, 2^-8 |ref| +
                                        3 x 2^-23 sum |terms|; backward 2^-8 |ref| + T 2^-23 sum |terms|, T taps collected.
                                        The reference forms its taps in fp32 as the kernel does (the values the device has).
    isolation        image 0 non-zero, the others zero, every weight non-zero: the other images' rows are the bias (or zero),
                     and dW is image 0's alone.

Every test prints its figure ("elements that differ" or "worst err / bound") before asserting, and asserts through
ops.last_tokenizer_kernel() that the kernel it is about is the one that ran.  Every pixel table is valid for its image."""
import ctypes

import numpy as np
import pytest
import torch

import tokenizer_ref as R

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
TAG = {F32: "fp32", BF16: "bf16"}


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def _bf(t):
    return None if t is None else t.to(BF16).cuda()


def _pix(t):
    return torch.from_numpy(np.ascontiguousarray(t)).cuda()


def _diff(got, want):
    """Elements of a device tensor that differ from the expected CPU tensor (NaN counts as different)."""
    got = got.detach().cpu()
    assert got.numel() == want.numel(), (tuple(got.shape), tuple(want.shape))
    return int((got.reshape(want.shape) != want.to(got.dtype)).sum())


def _ratio(got, ref, bound):
    err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    r = float((err / bound.clamp_min(1e-300)).max())
    return r if r == r else float("inf")


# ---- 1. exact answers ------------------------------------------------------------------------------------------------------
def _exact_pe(ops, dims, pix_h, desc, seed, fwd_name, bwd_name):
    (HW, N, P, C), D, B = dims
    pix, bad = _pix(pix_h), {}
    for xdt in (F32, BF16):
        x, w, bias, dy = R.exact_pe_inputs(dims, seed, xdt == F32)
        tok = R.gather_ref(x, pix_h)
        xd, wd, dyd = x.to(xdt).cuda(), _bf(w), _bf(dy).view(B, N, D)
        assert torch.equal(xd.cpu().to(BF16), x.to(BF16))
        for bb in ((bias, None) if xdt == F32 else (bias,)):
            y = ops.patch_embed_fwd(xd, pix, wd, _bf(bb), desc)
            assert ops.last_tokenizer_kernel() == f"{fwd_name}<{TAG[xdt]}>", ops.last_tokenizer_kernel()
            assert y.shape == (B, N, D) and y.dtype == BF16
            bad[f"y {TAG[xdt]}{'' if bb is not None else ' no bias'}"] = _diff(y, R.project_ref(tok, w, bb).float().to(BF16))
        dw_ref, db_ref = R.wgrad_ref(dy, tok)
        for want_bias in ((True, False) if xdt == F32 else (True,)):
            dw, db = ops.patch_embed_bwd(xd, pix, dyd, D, want_bias, desc)
            assert ops.last_tokenizer_kernel() == f"{bwd_name}<{TAG[xdt]}>", ops.last_tokenizer_kernel()
            assert dw.dtype == F32 and dw.shape == (D, P * C) and (db is None) == (not want_bias)
            bad[f"dW {TAG[xdt]}{'' if want_bias else ' no dbias'}"] = _diff(dw, dw_ref.float())
            if want_bias:
                bad[f"dbias {TAG[xdt]}"] = _diff(db, db_ref.float())
    return bad


@pytest.mark.parametrize("hostile", [False, True], ids=["curve", "hostile"])
@pytest.mark.parametrize("case", R.PE_CASES, ids=R.PE_IDS)
def test_generic_kernels_give_exact_answers(case, hostile, ops):
    dims = case[:3]
    bad = _exact_pe(ops, dims, R.pe_table(case, hostile), None, 100 + dims[0][0] + dims[1], "pe_fwd_kernel", "pe_bwd_kernel")
    print("exact pe", dims, "hostile" if hostile else case[3], "elements that differ:", bad)
    assert not any(bad.values()), bad


@pytest.mark.parametrize("case", R.PE2_CASES, ids=R.PE2_IDS)
def test_tiled_kernels_give_exact_answers(case, ops):
    name, img, C, B = case
    pix_h = R.pe2_table(name, img)
    desc = ops.tile_descriptor(pix_h, img, "cuda")
    assert desc is not None
    dims = ((img * img, pix_h.shape[0], 256, C), R.PE2_D, B)
    bad = _exact_pe(ops, dims, pix_h, desc, 300 + img + C, "pe2_fwd_kernel", "pe2_bwd_kernel")
    print("exact pe2", case, "classes", desc.cnt, "elements that differ:", bad)
    assert not any(bad.values()), bad


@pytest.mark.parametrize("xdt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.GATHER_CASES, ids=lambda c: "HW%d-N%d-P%d-C%d" % c)
def test_general_gather_is_torch_indexing(case, xdt, ops):
    """tokens_gather_kernel (P > 256 or C > 4) against torch indexing with the same table: one bf16 rounding of the same
    pixels, so bit for bit; B = 9 leaves one image in the second group of 8."""
    HW, N, P, C = case
    B, bad = R.GATHER_B, {}
    g = torch.Generator().manual_seed(40 + P)
    x = torch.randn(B, C, *R.image_hw(HW), generator=g)
    for name, pix_h in (("curve", R.curve_pixel_table("hilbert", R.image_hw(HW)[0], P)), ("hostile", R.hostile_table(HW, N, P, 3 * P))):
        tokens = ops.gather_tokens(x.to(xdt).cuda(), _pix(pix_h))
        assert ops.last_tokenizer_kernel() == f"tokens_gather_kernel<{TAG[xdt]}>", ops.last_tokenizer_kernel()
        ld = (P * C + 7) // 8 * 8
        assert tokens.shape == (B * N, ld)
        bad[name] = _diff(tokens, R.gather_ref(x, pix_h, ld).to(BF16))
    print("gather", case, TAG[xdt], "elements that differ:", bad)
    assert not any(bad.values()), bad


def test_general_gather_zeroes_the_padding_columns_of_a_wider_row(ops):
    """The C ABI with ld = P*C + 24 on a NaN-filled buffer: columns P*C .. ld - 1 come out as zeros."""
    HW, N, P, C = R.GATHER_CASES[0]
    B, ld = R.GATHER_B, P * C + 24
    x = torch.randn(B, C, *R.image_hw(HW), generator=torch.Generator().manual_seed(41))
    pix_h = R.hostile_table(HW, N, P, 5)
    xd, pix = x.cuda(), _pix(pix_h)
    tokens = torch.full((B * N, ld), float("nan"), device="cuda", dtype=BF16)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = ops.lib.sfcvit_tokens_gather(xd.data_ptr(), 0, pix.data_ptr(), None, B, C, HW, N, P, tokens.data_ptr(), ld, stream)
    assert rc == 0 and ops.last_tokenizer_kernel() == "tokens_gather_kernel<fp32>"
    bad = _diff(tokens, R.gather_ref(x, pix_h, ld).to(BF16))
    print("gather ld = P*C + 24: elements that differ:", bad)
    assert bad == 0 and not tokens[:, P * C:].any()


@pytest.mark.parametrize("variant", ["signed", "rounding"])
@pytest.mark.parametrize("case", R.HIER_CASES, ids=R.HIER_IDS)
def test_hierarchical_kernel_gives_exact_answers_in_both_forms(case, variant, ops):
    """h of the two forms is equal bit for bit and equals bf16(exact level sums), ties included; y equals the exact fusion
    of that h; the composed path (patch_embed_fwd per level) gives the same h bits.  (The M = 20 row has K = 96, the widest
    level the kernel's LDS holds beside L*D = 768: tokenizer_ref.HIER_CASES.)"""
    L, D, C, P, N, B = case
    bad = {}
    for hostile in (False, True):
        tabs_h = R.hier_tables(case, hostile)
        tabs = [_pix(t) for t in tabs_h]
        for xdt in (F32, BF16):
            x, w, b, wf, bfu = R.exact_hier_inputs(case, 700 + D + P, variant, xdt == F32)
            xd, wd, wfd = x.to(xdt).cuda(), [_bf(t) for t in w], _bf(wf)
            for biased in (True, False):
                bl, bf2 = (b, bfu) if biased else ([None] * L, None)
                _, h_ref, y_ref = R.hier_ref(x, tabs_h, w, bl, wf, bf2)
                bd = [_bf(t) for t in bl]
                y1, h1 = ops.hier_tokenizer_fwd(xd, tabs, wd, bd, wfd, _bf(bf2))
                assert ops.last_tokenizer_kernel() == f"hier_fwd_kernel<{TAG[xdt]}, fuse>", ops.last_tokenizer_kernel()
                y0, h0 = ops.hier_tokenizer_fwd(xd, tabs, wd, bd, None, None)
                assert ops.last_tokenizer_kernel() == f"hier_fwd_kernel<{TAG[xdt]}, levels>", ops.last_tokenizer_kernel()
                assert y0 is None and h1.shape == (B, N, L * D) and y1.shape == (B, N, L * D)
                composed = torch.cat([ops.patch_embed_fwd(xd, tabs[l], wd[l], bd[l]) for l in range(L)], dim=-1)
                assert ops.last_tokenizer_kernel().startswith("pe_fwd_kernel")
                key = f"{'hostile' if hostile else 'curves'} {TAG[xdt]}{'' if biased else ' no bias'}"
                bad[key] = {"h fuse": _diff(h1, h_ref.float().to(BF16)), "h levels": _diff(h0, h_ref.float().to(BF16)),
                            "h forms": int((h0 != h1).sum()), "h composed": int((composed != h0).sum()),
                            "y": _diff(y1, y_ref.float().to(BF16))}
    print("exact hier", case, variant, "elements that differ:", bad)
    assert not any(v for d in bad.values() for v in d.values()), bad


def _tap_sum_worst(grads, refs, mags, taps, dout, counts, D):
    """sum_j dlevels[l][b, j, :] against sum_i dout[b, i, l*D:(l+1)*D] (the taps of a row sum to 1): the allowance is the sum
    of the elements' own bounds, 2^-8 |ref| + T 2^-23 sum |terms| each."""
    worst = 0.0
    for l, (got, ref, mag, T) in enumerate(zip(grads, refs, mags, taps)):
        bound = (2.0 ** -8 * ref.abs() + T * 2.0 ** -23 * mag).sum(1)
        err = (got.cpu().double().sum(1) - dout.double()[..., l * D:(l + 1) * D].sum(1)).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


@pytest.mark.parametrize("D", R.RESAMPLE_D)
@pytest.mark.parametrize("counts", R.RESAMPLE_EXACT, ids=str)
def test_resampling_pair_gives_exact_answers(counts, D, ops):
    g = torch.Generator().manual_seed(60 + D + counts[-1])
    B = R.RESAMPLE_B
    levels = [R.ints(g, B, n, D) for n in counts]
    dout = R.ints(g, B, counts[0], len(counts) * D)
    out = ops.hier_resample_concat([_bf(t) for t in levels])
    assert ops.last_tokenizer_kernel() == "hier_resample_concat_kernel"
    grads = ops.hier_resample_concat_bwd(_bf(dout), list(counts), D)
    assert ops.last_tokenizer_kernel() == "hier_resample_concat_bwd_kernel"
    refs = R.resample_concat_bwd_ref(dout, counts, D)
    bad = {"out": _diff(out, R.resample_concat_ref(levels).float().to(BF16))}
    bad.update({f"dlevel {l}": _diff(got, ref.float().to(BF16)) for l, (got, ref) in enumerate(zip(grads, refs))})
    sums = _tap_sum_worst(grads, refs, R.resample_concat_bwd_abs(dout, counts, D), R.resample_taps_collected(counts), dout, counts, D)
    print("exact resample", counts, D, "elements that differ:", bad, "tap sums, worst err / bound:", sums)
    assert not any(bad.values()), bad
    assert sums <= 1.0


# ---- 2. random inputs within the format bounds -------------------------------------------------------------------------------
def _rn(g, *shape, scale=1.0):
    """bf16-rounded normals held in fp32; scaled first, rounded after."""
    return (torch.randn(*shape, generator=g) * scale).to(BF16).float()


def _bounded_pe(ops, dims, pix_h, desc, seed):
    (HW, N, P, C), D, B = dims
    K, pix, worst = P * C, _pix(pix_h), {}
    g = torch.Generator().manual_seed(seed)
    x = _rn(g, B, C, *R.image_hw(HW))
    w, bias, dy = _rn(g, D, K, scale=K ** -0.5), _rn(g, D, scale=0.1), _rn(g, B * N, D)
    tok = R.gather_ref(x, pix_h)
    y_ref, y_mag = R.project_ref(tok, w, bias), R.project_abs(tok, w, bias)
    (dw_ref, db_ref), (dw_mag, db_mag) = R.wgrad_ref(dy, tok), R.wgrad_abs(dy, tok)
    for xdt in (F32, BF16):
        xd = x.to(xdt).cuda()
        y = ops.patch_embed_fwd(xd, pix, _bf(w), _bf(bias), desc)
        fwd = ops.last_tokenizer_kernel()
        worst[f"y {TAG[xdt]}"] = _ratio(y, y_ref, 2.0 ** -8 * y_ref.abs() + (K + 1) * 2.0 ** -23 * y_mag)
        dw, db = ops.patch_embed_bwd(xd, pix, _bf(dy).view(B, N, D), D, True, desc)
        assert (fwd, ops.last_tokenizer_kernel()) == tuple(f"pe{'2' if desc else ''}_{d}_kernel<{TAG[xdt]}>" for d in ("fwd", "bwd"))
        worst[f"dW {TAG[xdt]}"] = _ratio(dw, dw_ref, B * N * 2.0 ** -24 * dw_mag)
        worst[f"dbias {TAG[xdt]}"] = _ratio(db, db_ref, B * N * 2.0 ** -24 * db_mag)
    return worst


@pytest.mark.parametrize("case", R.PE_CASES, ids=R.PE_IDS)
def test_generic_kernels_within_the_format_bounds(case, ops):
    worst = _bounded_pe(ops, case[:3], R.pe_table(case, True), None, 77 + case[1])
    print("bounded pe", case[:3], "worst err / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("case", [R.PE2_CASES[1], R.PE2_CASES[5]], ids=[R.PE2_IDS[1], R.PE2_IDS[5]])
def test_tiled_kernels_within_the_format_bounds(case, ops):
    name, img, C, B = case
    pix_h = R.pe2_table(name, img)
    desc = ops.tile_descriptor(pix_h, img, "cuda")
    worst = _bounded_pe(ops, ((img * img, pix_h.shape[0], 256, C), R.PE2_D, B), pix_h, desc, 78 + img)
    print("bounded pe2", case, "worst err / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("case", R.HIER_CASES + ["reference"], ids=R.HIER_IDS + ["reference-32px-16-4-1-D256"])
def test_hierarchical_kernel_within_the_format_bounds(case, ops):
    """The rows of the exact tests with one hostile table, and the reference's own configuration (32 px, [16, 4, 1],
    D = 256) with its own tables: pre-patches of 1, 2 and 4 pixels, 16 pixels per token on every level."""
    reference = case == "reference"
    L, D, C, P, N, B = case = R.HIER_REFERENCE_SHAPE if reference else case
    K, E, worst = P * C, L * D, {}
    g = torch.Generator().manual_seed(90 + D)
    x = _rn(g, B, C, *R.image_hw(N * P))
    w, b = [_rn(g, D, K, scale=K ** -0.5) for _ in range(L)], [_rn(g, D, scale=0.1) for _ in range(L)]
    wf, bfu = _rn(g, E, E, scale=E ** -0.5), _rn(g, E, scale=0.1)
    tabs_h = R.hier_reference_tables() if reference else R.hier_tables(case, True)
    assert all(t.shape == (N, P) for t in tabs_h)
    tabs = [_pix(t) for t in tabs_h]
    h_exact = R.hier_ref(x, tabs_h, w, b)[0]
    h_mag = R.hier_abs(x, tabs_h, w, b)[0]
    for xdt in (F32, BF16):
        xd = x.to(xdt).cuda()
        y, h = ops.hier_tokenizer_fwd(xd, tabs, [_bf(t) for t in w], [_bf(t) for t in b], _bf(wf), _bf(bfu))
        assert ops.last_tokenizer_kernel() == f"hier_fwd_kernel<{TAG[xdt]}, fuse>"
        _, h0 = ops.hier_tokenizer_fwd(xd, tabs, [_bf(t) for t in w], [_bf(t) for t in b], None, None)
        assert ops.last_tokenizer_kernel() == f"hier_fwd_kernel<{TAG[xdt]}, levels>"
        assert torch.equal(h, h0)                                               # the header: both forms, bit-identical in h
        worst[f"h {TAG[xdt]}"] = _ratio(h, h_exact, 2.0 ** -8 * h_exact.abs() + (K + 1) * 2.0 ** -23 * h_mag)
        hd = h.cpu().double().reshape(B * N, E)                                   # the h the kernel returned
        y_ref, y_mag = R.project_ref(hd, wf, bfu), R.project_abs(hd, wf, bfu)
        worst[f"y {TAG[xdt]}"] = _ratio(y, y_ref, 2.0 ** -8 * y_ref.abs() + (E + 1) * 2.0 ** -23 * y_mag)
    print("bounded hier", "reference tables" if reference else "", case, "worst err / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("D", R.RESAMPLE_D)
@pytest.mark.parametrize("counts", R.RESAMPLE_BOUNDED, ids=str)
def test_resampling_pair_within_the_format_bounds(counts, D, ops):
    g = torch.Generator().manual_seed(95 + D)
    B, f32 = R.RESAMPLE_B, np.float32
    levels = [_rn(g, B, n, D) for n in counts]
    dout = _rn(g, B, counts[0], len(counts) * D)
    out = ops.hier_resample_concat([_bf(t) for t in levels])
    assert ops.last_tokenizer_kernel() == "hier_resample_concat_kernel"
    grads = ops.hier_resample_concat_bwd(_bf(dout), list(counts), D)
    assert ops.last_tokenizer_kernel() == "hier_resample_concat_bwd_kernel"
    ref, mag = R.resample_concat_ref(levels, f32), R.resample_concat_abs(levels, f32)
    worst = {"out": _ratio(out, ref, 2.0 ** -8 * ref.abs() + 3 * 2.0 ** -23 * mag)}
    refs, mags, taps = R.resample_concat_bwd_ref(dout, counts, D, f32), R.resample_concat_bwd_abs(dout, counts, D, f32), R.resample_taps_collected(counts)
    for l, (got, r, m, T) in enumerate(zip(grads, refs, mags, taps)):
        worst[f"dlevel {l}"] = _ratio(got, r, 2.0 ** -8 * r.abs() + T * 2.0 ** -23 * m)
    worst["tap sums"] = _tap_sum_worst(grads, refs, mags, taps, dout, counts, D)
    print("bounded resample", counts, D, "taps", taps, "worst err / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- 3. isolation --------------------------------------------------------------------------------------------------------
def _isolated_pe(ops, dims, pix_h, desc, seed):
    (HW, N, P, C), D, B = dims
    x, w, bias, dy = R.exact_pe_inputs(dims, seed, False)
    w = w.abs() + 0.5                                              # every weight non-zero: a leak would show
    x[1:] = 0
    x[0] += 1                                                      # image 0 non-zero everywhere
    pix = _pix(pix_h)
    y = ops.patch_embed_fwd(x.cuda(), pix, _bf(w), _bf(bias), desc).cpu()
    assert torch.equal(y[1:].float(), bias.expand(B - 1, N, D)), "rows of the zero images must be the bias"
    assert float(ops.patch_embed_fwd(x.cuda(), pix, _bf(w), None, desc)[1:].abs().max()) == 0.0
    assert _diff(y, R.project_ref(R.gather_ref(x, pix_h), w, bias).float().to(BF16)) == 0
    x2 = R.exact_pe_inputs(dims, seed + 1, False)[0] + 1           # every image non-zero, dY of the others zero
    dy0 = dy.clone()
    dy0[N:] = 0
    dw, db = ops.patch_embed_bwd(x2.cuda(), pix, _bf(dy0).view(B, N, D), D, True, desc)
    dw_ref, db_ref = R.wgrad_ref(dy[:N], R.gather_ref(x2[:1], pix_h))
    return {"dW": _diff(dw, dw_ref.float()), "dbias": _diff(db, db_ref.float())}


@pytest.mark.parametrize("case", [R.PE_CASES[1], R.PE_CASES[2]], ids=[R.PE_IDS[1], R.PE_IDS[2]])
def test_generic_kernels_keep_the_images_apart(case, ops):
    bad = _isolated_pe(ops, case[:3], R.pe_table(case, True), None, 11)
    assert ops.last_tokenizer_kernel() == "pe_bwd_kernel<fp32>"
    print("isolation pe", case[:3], "elements that differ from image 0's gradient:", bad)
    assert not any(bad.values()), bad


@pytest.mark.parametrize("case", [R.PE2_CASES[1], R.PE2_CASES[5]], ids=[R.PE2_IDS[1], R.PE2_IDS[5]])
def test_tiled_kernels_keep_the_images_apart(case, ops):
    name, img, C, B = case
    pix_h = R.pe2_table(name, img)
    bad = _isolated_pe(ops, ((img * img, pix_h.shape[0], 256, C), R.PE2_D, B), pix_h, ops.tile_descriptor(pix_h, img, "cuda"), 12)
    assert ops.last_tokenizer_kernel() == "pe2_bwd_kernel<fp32>"
    print("isolation pe2", case, "elements that differ from image 0's gradient:", bad)
    assert not any(bad.values()), bad


@pytest.mark.parametrize("case", R.HIER_CASES[:2] + R.HIER_CASES[4:], ids=R.HIER_IDS[:2] + R.HIER_IDS[4:])
def test_hierarchical_kernel_keeps_the_images_apart(case, ops):
    L, D, C, P, N, B = case
    x, w, b, wf, bfu = R.exact_hier_inputs(case, 13, "signed", False)
    w, wf = [t.abs().clamp_min(0.5) for t in w], wf.abs().clamp_min(0.5)      # every weight non-zero: a leak would show
    x[1:] = 0
    x[0].clamp_(min=1)                                             # image 0 non-zero everywhere
    tabs_h = R.hier_tables(case, True)
    tabs = [_pix(t) for t in tabs_h]
    _, h_ref, y_ref = R.hier_ref(x, tabs_h, w, b, wf, bfu)
    h_mag, y_mag = R.hier_abs(x, tabs_h, w, b, wf, bfu)
    assert float(2 * h_mag.max() / 0.5) < 2 ** 24 and float(2 * y_mag.max() / 0.25) < 2 ** 24 and torch.equal(y_ref.float().double(), y_ref)
    for fuse in (True, False):
        y, h = ops.hier_tokenizer_fwd(x.cuda(), tabs, [_bf(t) for t in w], [_bf(t) for t in b], _bf(wf) if fuse else None, _bf(bfu) if fuse else None)
        assert ops.last_tokenizer_kernel() == f"hier_fwd_kernel<fp32, {'fuse' if fuse else 'levels'}>"
        assert torch.equal(h.cpu()[1:].float(), torch.cat(b).expand(B - 1, N, L * D)), "h rows of the zero images must be the level biases"
        assert _diff(h, h_ref.float().to(BF16)) == 0
        if fuse:
            row = R.project_ref(torch.cat(b)[None], wf, bfu).float().to(BF16)             # what the fusion makes of the biases
            assert torch.equal(y.cpu()[1:], row.expand(B - 1, N, L * D)) and _diff(y, y_ref.float().to(BF16)) == 0
        _, hz = ops.hier_tokenizer_fwd(x.cuda(), tabs, [_bf(t) for t in w], [None] * L, _bf(wf) if fuse else None, None)
        assert float(hz[1:].abs().max()) == 0.0
    print("isolation hier", case, "ok")


def test_resampling_pair_keeps_the_images_apart(ops):
    counts, D, B = (64, 16, 64), 8, R.RESAMPLE_B
    g = torch.Generator().manual_seed(14)
    for keep in range(B):
        levels = [R.ints(g, B, n, D).abs() + 1 for n in counts]
        dout = R.ints(g, B, counts[0], len(counts) * D).abs() + 1
        for t in levels + [dout]:
            t[[i for i in range(B) if i != keep]] = 0
        out = ops.hier_resample_concat([_bf(t) for t in levels]).cpu()
        grads = [t.cpu() for t in ops.hier_resample_concat_bwd(_bf(dout), list(counts), D)]
        for t in [out] + grads:
            assert all(float(t[i].abs().max()) == 0.0 for i in range(B) if i != keep) and float(t[keep].abs().min()) > 0
        assert _diff(out, R.resample_concat_ref(levels).float().to(BF16)) == 0
    print("isolation resample", counts, "ok")


# ---- 4. same bits twice ----------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(ops):
    g = torch.Generator().manual_seed(15)

    def family_pe(dims, pix_h, desc):
        (HW, N, P, C), D, B = dims
        x, w, bias, dy = _rn(g, B, C, *R.image_hw(HW)).cuda(), _bf(_rn(g, D, P * C, scale=0.1)), _bf(_rn(g, D)), _bf(_rn(g, B, N, D))
        pix = _pix(pix_h)
        return lambda: (ops.patch_embed_fwd(x, pix, w, bias, desc), *ops.patch_embed_bwd(x, pix, dy, D, True, desc))

    case, tiled = R.PE_CASES[3], R.PE2_CASES[5]
    pix2 = R.pe2_table(tiled[0], tiled[1])
    L, D, C, P, N, B = hc = R.HIER_CASES[3]
    tabs = [_pix(t) for t in R.hier_tables(hc, True)]
    hx, hw, hb = _rn(g, B, C, 32, 32).cuda(), [_bf(_rn(g, D, P * C, scale=0.1)) for _ in range(L)], [_bf(_rn(g, D)) for _ in range(L)]
    hwf, hbf = _bf(_rn(g, L * D, L * D, scale=0.03)), _bf(_rn(g, L * D))
    gx, gpix = _rn(g, 9, 3, 32, 32).cuda(), _pix(R.hostile_table(1024, 2, 512, 1))
    counts = (100, 36, 9, 100)
    lev, dout = [_bf(_rn(g, 3, n, 40)) for n in counts], _bf(_rn(g, 3, 100, 160))
    families = {
        "pe": family_pe(case[:3], R.pe_table(case, True), None),
        "pe2": family_pe(((tiled[1] ** 2, pix2.shape[0], 256, tiled[2]), R.PE2_D, tiled[3]), pix2, ops.tile_descriptor(pix2, tiled[1], "cuda")),
        "gather": lambda: (ops.gather_tokens(gx, gpix),),
        "hier": lambda: ops.hier_tokenizer_fwd(hx, tabs, hw, hb, hwf, hbf),
        "resample": lambda: (ops.hier_resample_concat(lev), *ops.hier_resample_concat_bwd(dout, list(counts), 40)),
    }
    for name, run in families.items():
        a, b = run(), run()
        same = all(torch.equal(p, q) for p, q in zip(a, b))
        print("twice", name, ops.last_tokenizer_kernel(), "same bits:", same)
        assert same, name
