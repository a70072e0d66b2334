"""The tokenizer tests' own foundations, without a GPU: the fp64 statements of tests/tokenizer_ref.py against plain torch,
the conditions under which the exact-answer inputs of tests/test_tokenizer_kernels_gpu.py really have exact answers (so
that no GPU run starts on inputs that break them), the fp32 resampling taps of the exact pairs, the guard sizes of the
containment shapes, the sfcvit_last_tokenizer_kernel query and the alignment refusals of sfcvit_patch_embed_fwd / _bwd."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import tokenizer_ref as R
from guarded import guard_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
BF16 = torch.bfloat16


# ---- anchoring -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hostile", [False, True], ids=["curve", "hostile"])
@pytest.mark.parametrize("case", R.PE_CASES[:3], ids=R.PE_IDS[:3])
def test_gather_projection_and_weight_gradients_are_plain_torch(case, hostile):
    """gather_ref / project_ref / wgrad_ref against advanced indexing + F.linear and autograd, fp64 on bf16-rounded values."""
    (HW, N, P, C), D, B = case[0], case[1], case[2]
    g = torch.Generator().manual_seed(5)
    pix = R.pe_table(case, hostile)
    x = torch.randn(B, C, *R.image_hw(HW), generator=g)
    w = torch.randn(D, P * C, generator=g).double().requires_grad_(True)
    bias = torch.randn(D, generator=g).double().requires_grad_(True)
    dy = torch.randn(B * N, D, generator=g).double()
    xb = x.to(BF16).double().reshape(B, C, HW)
    tok = torch.stack([xb[b][:, torch.from_numpy(pix).long()].permute(1, 2, 0).reshape(N, P * C) for b in range(B)]).reshape(B * N, P * C)
    y = TF.linear(tok, w, bias)
    y.backward(dy)
    ld = (P * C + 7) // 8 * 8 + 8
    mine = R.gather_ref(x, pix, ld)
    assert torch.equal(mine[:, :P * C], tok) and not mine[:, P * C:].any() and mine.shape == (B * N, ld)
    assert torch.allclose(R.project_ref(tok, w.detach(), bias.detach()), y.detach(), rtol=1e-13, atol=1e-13)
    dw, db = R.wgrad_ref(dy, tok)
    assert torch.allclose(dw, w.grad, rtol=1e-13, atol=1e-13) and torch.allclose(db, bias.grad, rtol=1e-13, atol=1e-13)
    assert bool((R.project_abs(tok, w.detach(), bias.detach()) >= y.detach().abs() - 1e-12).all())
    assert bool((R.wgrad_abs(dy, tok)[0] >= dw.abs() - 1e-12).all())


@pytest.mark.parametrize("counts", R.RESAMPLE_EXACT + R.RESAMPLE_BOUNDED, ids=str)
def test_resampling_statement_is_torch_linear_interpolation(counts):
    """resample_concat_ref / _bwd_ref against F.interpolate(mode="linear", align_corners=False) + cat and its autograd in
    fp64; the taps of every output row sum to 1."""
    g = torch.Generator().manual_seed(6)
    B, D = 2, 8
    leaves = [torch.randn(B, n, D, generator=g).double().requires_grad_(True) for n in counts]
    parts = [t if t.shape[1] == counts[0] else
             TF.interpolate(t.transpose(1, 2), size=counts[0], mode="linear", align_corners=False).transpose(1, 2) for t in leaves]
    ref = torch.cat(parts, dim=-1)
    dout = torch.randn(ref.shape, generator=g).double()
    ref.backward(dout)
    mine = R.resample_concat_ref([t.detach() for t in leaves])
    assert torch.allclose(mine, ref.detach(), rtol=1e-12, atol=1e-12)
    for got, leaf in zip(R.resample_concat_bwd_ref(dout, counts, D), leaves):
        assert torch.allclose(got, leaf.grad, rtol=1e-12, atol=1e-12)
    for n in counts:
        assert torch.allclose(R.resample_matrix(n, counts[0]).sum(1), torch.ones(counts[0], dtype=torch.float64), rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", ["hier_morton32", "hier_hilbert32_resample", "hier_morton32_d256", "hier_hilbert32_4lvl"])
def test_hierarchical_statement_reproduces_the_reference_fixture(name):
    """Levels -> resampling -> concatenation -> fusion from the statements, on the fixture's formula-valued state, against
    the recorded values of tests/golden/hierarchical.json: 3e-2 of the largest value, the bar of the GPU test that reads
    the same fixture (test_parity_gpu.py::test_hierarchical_tokenizer)."""
    from oracle import formula, vit_oracle
    from oracle.cases import HIER_CASES
    from sfcvit.curves import curve_table
    from sfcvit.tokenizers.embeddings import _pixel_table
    img, cin, plist, dim, curve, batch = HIER_CASES[name]
    with open(os.path.join(ROOT, "tests", "golden", "hierarchical.json")) as f:
        gold = json.load(f)[name]
    sd = vit_oracle.hierarchical_state(img, cin, plist, dim, curve)
    x = formula.image_batch(batch, cin, img, img)
    levels = []
    for i, grp in enumerate(plist):
        p = 2 ** i
        pix = _pixel_table(curve_table(curve, img // p), img, p, grp)
        h = R.hier_ref(x, [pix], [sd[f"levels.{i}.proj.weight"]], [sd[f"levels.{i}.proj.bias"]])[1]
        levels.append(h.reshape(batch, pix.shape[0], dim))
    y = R.project_ref(R.resample_concat_ref(levels).reshape(-1, dim * len(plist)), sd["fusion.weight"], sd["fusion.bias"])
    assert list(y.reshape(batch, -1, dim * len(plist)).shape) == gold["shape"]
    got = y.flatten()[torch.tensor(gold["idx"])]
    err = float((got - torch.tensor(gold["val"], dtype=torch.float64)).abs().max())
    print(name, "worst |err|", err, "of", float(y.abs().max()))
    assert err <= 3e-2 * float(y.abs().max())


# ---- conditions of the exact cases ------------------------------------------------------------------------------------------
def _exact_in_fp32(mag, quantum):
    return float(2 * mag.max() / quantum) < 2 ** 24


@pytest.mark.parametrize("offsets", [False, True], ids=["integers", "fp32-offsets"])
@pytest.mark.parametrize("hostile", [False, True], ids=["curve", "hostile"])
@pytest.mark.parametrize("case", R.PE_CASES, ids=R.PE_IDS)
def test_exact_patch_embed_inputs_have_exact_answers(case, hostile, offsets):
    (HW, N, P, C), D, B = case[0], case[1], case[2]
    x, w, bias, dy = R.exact_pe_inputs(case, 100 + HW + D, offsets)
    tok = R.gather_ref(x, R.pe_table(case, hostile))
    assert torch.equal(tok, tok.round()) and float(tok.min()) >= 0                  # the bf16 rounding returned the integers
    if offsets:
        assert int((x != x.round()).sum()) >= x.numel() // 8 or R.exact_hi(P * C) == 3
        assert int((x != x.round()).sum()) > 0
    y, dwb = R.project_ref(tok, w, bias), R.wgrad_ref(dy, tok)
    assert _exact_in_fp32(R.project_abs(tok, w, bias), 0.5)
    assert all(_exact_in_fp32(m, 1.0) for m in R.wgrad_abs(dy, tok))
    for t in (y, *dwb):
        assert torch.equal(t.float().double(), t)


@pytest.mark.parametrize("case", R.PE2_CASES, ids=R.PE2_IDS)
def test_exact_tiled_inputs_have_exact_answers_and_tile_descriptors(case):
    """The same conditions for the tiled cases, and the table facts they rely on: every table is tileable, the hostile one
    has the descriptor's 8 classes with 1-2 tokens each, and Z at B = 33 has one class of 132 rows (a second row tile)."""
    from sfcvit._lib import lib
    name, img, C, B = case
    pix = R.pe2_table(name, img)
    N = pix.shape[0]
    desc = np.zeros(16 + 2 * N + 2 * 8 * 256, dtype=np.int32)
    n = lib.sfcvit_tile_descriptors(ctypes.c_void_p(pix.ctypes.data), N, 256, img, ctypes.c_void_p(desc.ctypes.data), desc.size)
    assert n > 0 and np.array_equal(np.sort(pix.reshape(-1)), np.arange(img * img))
    cnt = [int(desc[7 + c] - desc[6 + c]) for c in range(desc[1])]
    if name == "hostile8":
        assert desc[0] == 1 and desc[1] == 8 and sorted(set(cnt)) == [1, 2] and [3 * c for c in sorted(set(cnt))] == [3, 6]
    if name == "z":
        assert cnt == [4] and (B != 33 or 4 * B == 132)
    if name == "raster":
        assert desc[0] == 2
    for offsets in (False, True):
        x, w, bias, dy = R.exact_pe_inputs(((img * img, N, 256, C), R.PE2_D, B), 300 + img + C, offsets)
        tok = R.gather_ref(x, pix)
        assert torch.equal(tok, tok.round())
        assert _exact_in_fp32(R.project_abs(tok, w, bias), 0.5) and all(_exact_in_fp32(m, 1.0) for m in R.wgrad_abs(dy, tok))
        for t in (R.project_ref(tok, w, bias), *R.wgrad_ref(dy, tok)):
            assert torch.equal(t.float().double(), t)


@pytest.mark.parametrize("variant", ["signed", "rounding"])
@pytest.mark.parametrize("case", R.HIER_CASES, ids=R.HIER_IDS)
def test_exact_hierarchical_inputs_have_exact_answers(case, variant):
    """Level sums in quanta of 1/2, fusion sums in quanta of 1/4, both exact in fp32 and surviving .float(); in the
    rounding variant at least 10 % of the exact h is not a bf16 value and at least one element is an exact tie."""
    L, D, C, P, N, B = case
    share = {}
    for hostile in (False, True):
        for offsets in (False, True):
            x, w, b, wf, bfu = R.exact_hier_inputs(case, 700 + D + P, variant, offsets)
            tabs = R.hier_tables(case, hostile)
            assert len({t.tobytes() for t in tabs}) == L                     # every level has a table of its own
            for bias_on in (True, False):
                bl, bf2 = (b, bfu) if bias_on else ([None] * L, None)
                h_exact, h, y = R.hier_ref(x, tabs, w, bl, wf, bf2)
                h_mag, y_mag = R.hier_abs(x, tabs, w, bl, wf, bf2)
                assert _exact_in_fp32(h_mag, 0.5) and _exact_in_fp32(y_mag, 0.25), (float(h_mag.max()), float(y_mag.max()))
                assert torch.equal(h_exact.float().double(), h_exact) and torch.equal(y.float().double(), y)
                assert torch.equal(h_exact * 2, (h_exact * 2).round()) and torch.equal(y * 4, (y * 4).round())
                rounded = h != h_exact
                # a tie: the exact value lies midway between two neighbouring bf16 values
                down = h_exact.float().view(torch.int32).bitwise_and(-65536).view(torch.float32).double()
                step = torch.where(h_exact != 0, 2.0 ** (torch.floor(torch.log2(h_exact.abs().clamp_min(1e-30))) - 7), torch.zeros(()).double())
                ties = rounded & ((h_exact - down).abs() * 2 == step)
                share[(hostile, offsets, bias_on)] = (float(rounded.double().mean()), int(ties.sum()), float(y_mag.max() * 8))
    print(case, variant, "(rounded share, ties, worst fusion sum in quanta x 2):", share)
    if variant == "rounding":
        assert all(s >= 0.10 and t >= 1 for s, t, _ in share.values()), share


@pytest.mark.parametrize("counts", R.RESAMPLE_EXACT, ids=str)
def test_exact_resampling_inputs_have_exact_answers(counts):
    """Integers in -2 .. 2 through taps in eighths: forward and transposed sums are bf16 values."""
    g = torch.Generator().manual_seed(8)
    for D in R.RESAMPLE_D:
        levels = [R.ints(g, R.RESAMPLE_B, n, D) for n in counts]
        dout = R.ints(g, R.RESAMPLE_B, counts[0], len(counts) * D)
        for t in [R.resample_concat_ref(levels)] + R.resample_concat_bwd_ref(dout, counts, D):
            assert torch.equal(t.float().to(BF16).double(), t) and torch.equal(t * 8, (t * 8).round())


@pytest.mark.parametrize("n0,nl", R.RESAMPLE_EXACT_PAIRS)
def test_fp32_taps_of_the_exact_pairs_equal_the_fp64_taps(n0, nl):
    """rs_taps' fp32 formula gives the same i0, i1, w1 as fp64 for the ratios 2, 4 and 1/4, with weights in eighths (or
    all 1/2); (7, 1) does not qualify (its fp32 scale is inexact) and belongs to the bounded tests only."""
    a, b = R.resample_taps(nl, n0, np.float32), R.resample_taps(nl, n0, np.float64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].astype(np.float64), b[2])
    assert np.array_equal(b[2] * 8, np.round(b[2] * 8))
    odd32, odd64 = R.resample_taps(1, 7, np.float32), R.resample_taps(1, 7, np.float64)
    assert not np.array_equal(odd32[2].astype(np.float64), odd64[2])


def test_every_exact_resample_level_is_an_exact_pair():
    pairs = set(R.RESAMPLE_EXACT_PAIRS)
    for counts in R.RESAMPLE_EXACT:
        assert all(n == counts[0] or (counts[0], n) in pairs for n in counts[1:]), counts
    assert R.resample_taps_collected((7, 1)) == [1, 10] and R.resample_taps_collected((64, 16, 64))[2] == 1


def test_hierarchical_cases_are_inside_the_envelope_and_the_k768_row_is_refused():
    """Every HIER_CASES row is inside the fused kernel's envelope.  The row as first written (four levels of K = 768 at
    L*D = 768) is not: 64 rows of L*D + sum K bf16 exceed the 160 KiB of LDS in either form, and the library says so on the
    host, before any HIP call."""
    from sfcvit import _lib
    lib = _lib.lib
    for L, D, C, P, N, B in R.HIER_CASES:
        assert lib.sfcvit_hier_tokenizer_supported(L, D, C, (ctypes.c_int32 * 4)(*[P] * L)) == 1, (L, D, C, P)
        assert all(int((t != t2).sum()) > 0 for i, t in enumerate(R.hier_tables((L, D, C, P, N, B), False))
                   for t2 in R.hier_tables((L, D, C, P, N, B), False)[:i])
    L, D, C, P, N, B = R.HIER_OUTSIDE
    assert 64 * (2 * L * D + 16) + 64 * (2 * L * P * C + 16) > 160 * 1024 and 64 * (2 * L * P * C + 16) > 160 * 1024
    assert lib.sfcvit_hier_tokenizer_supported(L, D, C, (ctypes.c_int32 * 4)(*[P] * L)) == 0
    for K in (104, 112, 120, 128):                                 # nothing wider than K = 96 fits beside L*D = 768
        assert lib.sfcvit_hier_tokenizer_supported(4, 192, 1, (ctypes.c_int32 * 4)(*[K] * 4)) == 0, K
    assert lib.sfcvit_hier_tokenizer_supported(4, 192, 1, (ctypes.c_int32 * 4)(*[96] * 4)) == 1
    raw = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(raw) + 15) // 16 * 16                # aligned host addresses: never dereferenced
    for fuse in (True, False):
        a = _lib.HierArgs()
        a.x, a.h, a.y, a.wf = p, p, (p if fuse else None), (p if fuse else None)
        for l in range(L):
            a.pix[l], a.w[l], a.P[l] = p, p, P
        a.B, a.C, a.HW, a.N, a.L, a.D = B, C, N * P, N, L, D
        assert lib.sfcvit_hier_tokenizer_fwd(ctypes.byref(a), None) == EINVAL
        assert "envelope" in lib.sfcvit_last_error().decode()


# ---- guards ----------------------------------------------------------------------------------------------------------------
def test_guards_cover_a_stray_row_of_every_containment_shape():
    """tests/guarded.py sizes guards by rows of the buffer's own pitch: for every tokenizer containment buffer the guard must
    hold one whole stray unit (a row tile of the kernel that writes it, one image for x)."""
    bufs = R.containment_buffers()
    assert len(bufs) >= 25
    for what, shape, dtype, stray in bufs:
        assert guard_bytes(shape, dtype) >= stray, (what, shape, guard_bytes(shape, dtype), stray)


# ---- the query (the refusals: tests/test_tokenizer_plans_cpu.py) ------------------------------------------------------------------
def test_last_tokenizer_kernel_is_exported_and_says_none():
    from sfcvit import _lib, ops
    header = open(os.path.join(ROOT, "include", "sfcvit.h")).read()
    name = "sfcvit_last_tokenizer_kernel"
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", header)
    assert m and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == 2
    assert re.search(r"#define\s+SFCVIT_ABI_VERSION\s+1\b", header) and _lib.lib.sfcvit_abi_version() == 1
    buf = ctypes.create_string_buffer(96)
    assert _lib.lib.sfcvit_last_tokenizer_kernel(buf, 96) == 0 and buf.value == b"none"      # nothing was launched
    assert _lib.lib.sfcvit_last_tokenizer_kernel(None, 96) == EINVAL
    assert _lib.lib.sfcvit_last_tokenizer_kernel(buf, 0) == EINVAL and _lib.lib.sfcvit_last_tokenizer_kernel(buf, -3) == EINVAL
    assert ops.last_tokenizer_kernel() == "none"

