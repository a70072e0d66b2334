"""fp64 statements of the tokenizer operations, written from the contracts in include/sfcvit.h and shared by
test_tokenizer_ref_cpu.py, test_tokenizer_kernels_gpu.py and the tokenizer cases of test_containment_gpu.py:

    gather        tokens[b*N + n][kk*C + c] = bf16(x[b, c, pix[n][kk]]), padding columns zero
    projection    y = tokens . W^T + bias
    weight grads  dW = dY^T . tokens, dbias = sum dY
    hierarchical  h = bf16(W_l tokens_l + b_l) per level, concatenated;  y = Wf . h + bf
    resampling    torch's linear taps src = max(0, (i + 1/2) N_l / N_0 - 1/2), concatenated on the feature axis, and the
                  transpose of that map

Everything is plain torch / numpy on the CPU in fp64: no kernel, no tokenizer module and no oracle code is involved.
Every statement has an `_abs` twin, the sum of |terms|, which is the scale of the error bounds.  The module also holds the
shape lists of the GPU tests (so that the CPU file can check their conditions before any GPU run), the generators of the
exact-answer inputs and the generators of hostile but valid pixel tables."""
import math

import numpy as np
import torch

BF16 = torch.bfloat16

# ---- shape lists ---------------------------------------------------------------------------------------------------------
# generic fused kernels (desc=None): ((HW, N, P, C), D, B, curve of the natural table or None, what it reaches)
PE_CASES = [
    ((81, 9, 9, 3), 8, 1, "peano", "scalar gather, K = 27 padded to 32, smallest D"),
    ((196, 4, 49, 3), 72, 5, "spiral", "K = 147: three k-tiles, last one ragged"),
    ((64, 8, 8, 3), 136, 17, "hilbert", "K = 24, M = 136 and D = 136 past a 128 tile"),
    ((256, 16, 16, 3), 8, 261, "hilbert", "M = 4176: 66 splits, the z += 64 wrap of pe_bwd_reduce"),
    ((256, 1, 256, 1), 256, 3, "hilbert", "one token per image, K = 256, D = 256"),
    ((1024, 4, 256, 3), 256, 3, "hilbert", "K = 768"),
]
PE_IDS = ["HW%d-N%d-P%d-C%d" % c[0] for c in PE_CASES]
# tiled kernels at D = 256: (table, image side, C, B)
PE2_CASES = [("hilbert", 32, 1, 3), ("hilbert", 32, 3, 33), ("z", 32, 3, 3), ("z", 32, 1, 33), ("raster", 32, 3, 3),
             ("hostile8", 48, 3, 3)]
PE2_IDS = ["%s%d-C%d-B%d" % c for c in PE2_CASES]
PE2_D = 256
# general per-pixel gather: (HW, N, P, C), B = 9 (a second group of 8 images holding one)
GATHER_CASES = [(1024, 2, 512, 3), (256, 4, 64, 5), (1024, 1, 1024, 1)]
GATHER_B = 9
# fused hierarchical tokenizer: (L, D, C, P, N, B).  The last row is the "M = 20, wave 3 idle in the level phase" case.  As
# first written it had P = 256 (K = 768 on four levels), which no form of the kernel can hold: 64 rows of L*D + sum K bf16
# must fit 160 KiB of LDS, and at L*D = 768 that leaves sum K <= 496.  D = 192 forces L = 4 (L*D % 256 == 0), so the widest
# level that fits is K = 96 (P = 32; K = 120 pads to 128 per level and is over).  The P = 256 row is kept as HIER_OUTSIDE:
# the library must say so in sfcvit_hier_tokenizer_supported and refuse it with SFCVIT_EINVAL before any launch.
HIER_CASES = [(1, 256, 1, 8, 5, 13), (2, 128, 3, 8, 8, 2), (4, 64, 3, 64, 16, 3), (3, 256, 3, 16, 64, 2), (4, 192, 3, 32, 4, 5)]
HIER_OUTSIDE = (4, 192, 3, 256, 4, 5)
HIER_IDS = ["L%d-D%d-C%d-P%d-N%d-B%d" % c for c in HIER_CASES]
HIER_REFERENCE_SHAPE = (3, 256, 3, 16, 64, 2)       # 32 px, [16, 4, 1], D = 256 (16 pixels per token on every level)
# resampling: token counts per level
RESAMPLE_EXACT = [(64, 32), (64, 16, 64), (16, 64), (48, 12), (256, 64)]
RESAMPLE_BOUNDED = [(100, 36, 9, 100), (7, 1)]
RESAMPLE_EXACT_PAIRS = [(64, 32), (64, 16), (16, 64), (48, 12), (256, 64)]          # (N_0, N_l)
RESAMPLE_D, RESAMPLE_B = (8, 40), 3
# containment shapes (test_containment_gpu.py): name -> {buffer: (shape, dtype)} is built there; the row counts live here
CONTAIN_PE = [((81, 9, 9, 3), 8, 1), ((64, 8, 8, 3), 136, 17), ((256, 16, 16, 3), 8, 261)]
CONTAIN_PE2 = [("hilbert", 32, 3, 33), ("hostile8", 48, 3, 3)]
CONTAIN_GATHER = [((256, 16, 16, 3), 9, 0), ((1024, 2, 512, 3), 9, 0), ((1024, 2, 512, 3), 9, 24)]     # (table, B, extra ld)
CONTAIN_HIER = [HIER_CASES[0], HIER_CASES[4]]
CONTAIN_RESAMPLE = [(64, 16, 64), (7, 1)]


def image_hw(HW):
    """(H, W) of the test image with H * W pixels: square where HW is a square, else rows of 8."""
    r = math.isqrt(HW)
    return (r, r) if r * r == HW else (HW // 8, 8)


def exact_hi(K):
    """Largest pixel value of the exact-answer inputs for a contraction of K features: keeps every partial sum of
    half-integer products exactly representable in fp32 (checked case by case in test_tokenizer_ref_cpu.py)."""
    return 127 if K <= 8 else 63 if K <= 27 else 31 if K <= 48 else 15 if K <= 96 else 3


# ---- pixel tables --------------------------------------------------------------------------------------------------------
def curve_pixel_table(curve, img, P):
    """The tokenizer's own table for a curve: sfcvit_pixel_table on the curve's flat table (host code of the library)."""
    from sfcvit.curves import curve_table
    from sfcvit.tokenizers.embeddings import _pixel_table
    flat = np.arange(img * img, dtype=np.int32) if curve == "raster" else curve_table(curve, img)
    return _pixel_table(flat, img, 1, P)


def hostile_table(HW, N, P, seed):
    """Hostile but valid: a random permutation of 0 .. HW - 1 as [N, P] int32.  Every offset lies inside the image."""
    assert N * P == HW
    return np.random.default_rng(seed).permutation(HW).astype(np.int32).reshape(N, P)


def hostile_tile_table(img, seed, classes=8):
    """The tiled kernels' hostile table: the 16 x 16 tiles of an img x img image in shuffled visiting order, the order
    inside each tile drawn from `classes` distinct random permutations (the tile descriptor's class limit), every class
    used and as evenly as the tile count allows (48 px: nine tiles, class sizes 1-2).  [N, 256] int32."""
    assert img % 16 == 0
    rng = np.random.default_rng(seed)
    t = img // 16
    N = t * t
    classes = min(classes, N)
    perms = []
    while len(perms) < classes:
        p = rng.permutation(256)
        if not any(np.array_equal(p, q) for q in perms):
            perms.append(p)
    cls = np.concatenate([np.arange(classes)] * (N // classes + 1))[:N]
    rng.shuffle(cls)
    pix = np.empty((N, 256), dtype=np.int32)
    for n, tile in enumerate(rng.permutation(N)):
        r0, c0 = (tile // t) * 16, (tile % t) * 16
        j = perms[cls[n]]                                          # curve position kk -> pixel of the tile, raster order
        pix[n] = (r0 + j // 16) * img + c0 + j % 16
    assert np.array_equal(np.sort(pix.reshape(-1)), np.arange(img * img))
    return pix


def pe_table(case, hostile):
    (HW, N, P, C), _, _, curve, _ = case
    if hostile or curve is None:
        return hostile_table(HW, N, P, seed=HW + 7 * P)
    return curve_pixel_table(curve, math.isqrt(HW), P)


def pe2_table(name, img):
    return hostile_tile_table(img, seed=img) if name == "hostile8" else curve_pixel_table(name, img, 256)


def hier_tables(case, hostile):
    """One table per level, all different.  Square images: the curve tables of Hilbert, Z, raster and Moore.  Other images
    (rows of 8 pixels): raster, boustrophedon (odd rows reversed), column-major and a random permutation.  `hostile` swaps
    level 0 for a random permutation."""
    L, D, C, P, N, B = case
    HW = N * P
    H, W = image_hw(HW)
    if H == W:
        tabs = [curve_pixel_table(c, H, P) for c in ("hilbert", "z", "raster", "moore")[:L]]
    else:
        grid = np.arange(HW, dtype=np.int32).reshape(H, W)
        snake = grid.copy()
        snake[1::2] = snake[1::2, ::-1]
        scans = [grid.reshape(-1), snake.reshape(-1), np.ascontiguousarray(grid.T).reshape(-1), hostile_table(HW, N, P, seed=HW + 5).reshape(-1)]
        tabs = [np.ascontiguousarray(t.reshape(N, P)) for t in scans[:L]]
    if hostile:
        tabs[0] = hostile_table(HW, N, P, seed=HW + 11 * L)
    return tabs


def hier_reference_tables():
    """The tables of the reference's own hierarchical configuration (32 px, patch sizes [16, 4, 1], Z order): level i groups
    patch_size pre-patches of 2^i x 2^i pixels, 16 pixels per token and 64 tokens on every level (HIER_REFERENCE_SHAPE)."""
    from sfcvit.curves import curve_table
    from sfcvit.tokenizers.embeddings import _pixel_table
    return [_pixel_table(curve_table("z", 32 // p), 32, p, g) for p, g in ((1, 16), (2, 4), (4, 1))]


# ---- exact-answer inputs -------------------------------------------------------------------------------------------------
RNE_OFFSET = 2.0 ** -10 + 2.0 ** -13


def exact_image(g, B, C, HW, hi, fp32_offsets):
    """Integers 0 .. hi as [B, C, H, W] fp32.  With fp32_offsets every fourth non-zero pixel is lowered by 2^-10 + 2^-13:
    less than half a bf16 step at every value up to 127, so round-to-nearest-even returns the integer while truncation
    returns the bf16 value below it.  (Images handed over as bf16 hold the integers themselves.)"""
    H, W = image_hw(HW)
    x = torch.randint(0, hi + 1, (B, C, H, W), generator=g).float()
    if fp32_offsets:
        assert hi <= 127
        flat = x.view(-1)
        pick = (torch.arange(flat.numel()) % 4 == 1) & (flat > 0)
        flat[pick] -= RNE_OFFSET
    return x


def half_ints(g, *shape, lo=-3, hi=3):
    """Multiples of 1/2 in [lo / 2, hi / 2]."""
    return torch.randint(lo, hi + 1, shape, generator=g).float() / 2


def ints(g, *shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_pe_inputs(case, seed, fp32_offsets):
    """(x, w, bias, dy) of one PE_CASES / PE2-style case: pixels 0 .. hi, weights in halves in [-3/2, 3/2], bias in
    {-1, 0, 1}, dY integers in -2 .. 2."""
    (HW, N, P, C), D, B = case[0], case[1], case[2]
    g = torch.Generator().manual_seed(seed)
    x = exact_image(g, B, C, HW, exact_hi(P * C), fp32_offsets)
    return x, half_ints(g, D, P * C), ints(g, D, lo=-1, hi=1), ints(g, B * N, D)


def exact_hier_inputs(case, seed, variant, fp32_offsets):
    """(x, [W_l], [b_l], Wf, bf) of one HIER_CASES case.  variant "signed": level weights in halves in [-3/2, 3/2];
    "rounding": level weights in {0, 1/2, 1, 3/2}, so that the level sums grow past 256 and most of h has to be rounded
    to bf16, exact ties included.  Wf signed halves, biases in {-1, 0, 1}."""
    L, D, C, P, N, B = case
    g = torch.Generator().manual_seed(seed)
    x = exact_image(g, B, C, N * P, exact_hi(P * C), fp32_offsets)
    lo = -3 if variant == "signed" else 0
    w = [half_ints(g, D, P * C, lo=lo, hi=3) for _ in range(L)]
    b = [ints(g, D, lo=-1, hi=1) for _ in range(L)]
    return x, w, b, half_ints(g, L * D, L * D, lo=-2, hi=2), ints(g, L * D, lo=-1, hi=1)


# ---- the statements ------------------------------------------------------------------------------------------------------
def bf16_round(t):
    """Round-to-nearest-even to bf16, returned in fp64.  A single rounding when t survives .float() (asserted by callers
    that need it)."""
    return t.float().to(BF16).double()


def gather_ref(x, pix, ld=None):
    """tokens [B*N, ld] fp64 = bf16(x[b, c, pix[n][kk]]) at column kk*C + c; columns P*C .. ld - 1 zero."""
    B, C = x.shape[0], x.shape[1]
    pix = torch.as_tensor(np.asarray(pix)).long()
    N, P = pix.shape
    xb = x.to(BF16).double().reshape(B, C, -1)
    tok = xb[:, :, pix]                                            # [B, C, N, P]
    tok = tok.permute(0, 2, 3, 1).reshape(B * N, P * C)
    if ld is not None and ld > P * C:
        tok = torch.cat([tok, torch.zeros(B * N, ld - P * C, dtype=torch.float64)], dim=1)
    return tok


def project_ref(tokens, w, bias=None):
    y = tokens.double() @ w.double().t()
    return y if bias is None else y + bias.double()


def project_abs(tokens, w, bias=None):
    return project_ref(tokens.abs(), w.abs(), None if bias is None else bias.abs())


def wgrad_ref(dy, tokens):
    """(dW [D, K] = dY^T tokens, dbias [D] = sum of dY rows)."""
    dy = dy.double().reshape(-1, dy.shape[-1])
    return dy.t() @ tokens.double(), dy.sum(0)


def wgrad_abs(dy, tokens):
    return wgrad_ref(dy.abs(), tokens.abs())


def hier_ref(x, pix_list, w_list, b_list, wf=None, bf=None, round_h=True):
    """(h_exact, h, y): h_exact [M, L*D] the level outputs before rounding, h = bf16(h_exact) (or h_exact itself with
    round_h=False), y = Wf h + bf (None without wf)."""
    parts = [project_ref(gather_ref(x, pix), w, b) for pix, w, b in zip(pix_list, w_list, b_list)]
    h_exact = torch.cat(parts, dim=1)
    h = bf16_round(h_exact) if round_h else h_exact
    return h_exact, h, (None if wf is None else project_ref(h, wf, bf))


def hier_abs(x, pix_list, w_list, b_list, wf=None, bf=None):
    """(sum |terms| of the level outputs, sum |terms| of y on the rounded h)."""
    parts = [project_abs(gather_ref(x, pix), w, b) for pix, w, b in zip(pix_list, w_list, b_list)]
    h = hier_ref(x, pix_list, w_list, b_list)[1]
    return torch.cat(parts, dim=1), (None if wf is None else project_abs(h, wf, bf))


def resample_taps(n_l, n0, dtype=np.float64):
    """(i0, i1, w1) of every output row i < n0: torch's linear taps with align_corners=False.  dtype=np.float32 evaluates
    the formula operation by operation in fp32, the way the kernels' rs_taps does."""
    f = dtype
    i = np.arange(n0).astype(f)
    scale = f(f(n_l) / f(n0))
    src = (scale * (i + f(0.5))).astype(f) - f(0.5)
    src = np.maximum(src, f(0)).astype(f)
    i0 = np.minimum(src.astype(np.int64), n_l - 1)
    i1 = np.minimum(i0 + 1, n_l - 1)
    w1 = (src - i0.astype(f)).astype(f)
    return i0, i1, w1


def resample_matrix(n_l, n0, taps=np.float64):
    """R [n0, n_l] fp64 with out = R y; the identity when the counts agree.  taps=np.float32: the weights as the kernels
    form them (w1 from the fp32 formula, w0 = 1 - w1 rounded to fp32), summed in fp64 all the same."""
    if n_l == n0:
        return torch.eye(n0, dtype=torch.float64)
    i0, i1, w1 = resample_taps(n_l, n0, taps)
    w0 = (taps(1) - w1).astype(np.float64)
    R = torch.zeros(n0, n_l, dtype=torch.float64)
    rows = torch.arange(n0)
    R.index_put_((rows, torch.from_numpy(i0)), torch.from_numpy(w0), accumulate=True)
    R.index_put_((rows, torch.from_numpy(i1)), torch.from_numpy(w1.astype(np.float64)), accumulate=True)
    return R


def resample_concat_ref(levels, taps=np.float64):
    """levels: [B, N_l, D] each -> [B, N_0, L*D] fp64."""
    n0 = levels[0].shape[1]
    return torch.cat([torch.einsum("ij,bjd->bid", resample_matrix(t.shape[1], n0, taps), t.double()) for t in levels], dim=-1)


def resample_concat_abs(levels, taps=np.float64):
    return resample_concat_ref([t.abs() for t in levels], taps)


def resample_concat_bwd_ref(dout, counts, D, taps=np.float64):
    """The transpose: dlevels[l][b, j, :] = sum_i R_l[i, j] dout[b, i, l*D:(l+1)*D]."""
    n0 = counts[0]
    return [torch.einsum("ij,bid->bjd", resample_matrix(n, n0, taps), dout.double()[..., l * D:(l + 1) * D]) for l, n in enumerate(counts)]


def resample_concat_bwd_abs(dout, counts, D, taps=np.float64):
    return resample_concat_bwd_ref(dout.abs(), counts, D, taps)


def resample_taps_collected(counts):
    """T per level: the largest number of taps (counted as the kernel adds them: both taps of a row, even where they meet
    on one token) any input token of that level collects."""
    n0, out = counts[0], []
    for n in counts:
        if n == n0:
            out.append(1)
            continue
        i0, i1, w1 = resample_taps(n, n0)
        out.append(int((np.bincount(i0, minlength=n) + np.bincount(i1[w1 != 0], minlength=n)).max()))
    return out


def containment_buffers():
    """(what, shape, dtype, stray bytes) of every 2-D-or-more buffer of the tokenizer containment cases: `stray` is how far
    past the view one whole extra unit lands -- a row tile of the kernel for token-row buffers (128 rows for the patch-embed
    kernels, 64 for the hierarchical one, one row for the resampling and gather kernels), one image for x."""
    out = []
    for (HW, N, P, C), D, B in CONTAIN_PE:
        H, W = image_hw(HW)
        out += [("pe x", (B, C, H, W), torch.float32, C * HW * 4), ("pe y", (B * N, D), BF16, 128 * D * 2),
                ("pe dw", (D, P * C), torch.float32, P * C * 4), ("pe pix", (N, P), torch.int32, P * 4)]
    for name, img, C, B in CONTAIN_PE2:
        N = img * img // 256
        out += [("pe2 x", (B, C, img, img), torch.float32, C * img * img * 4), ("pe2 y", (B * N, PE2_D), BF16, 128 * PE2_D * 2),
                ("pe2 dw", (PE2_D, 256 * C), torch.float32, 256 * C * 4)]
    for (HW, N, P, C), B, extra in CONTAIN_GATHER:
        H, W = image_hw(HW)
        out += [("gather x", (B, C, H, W), torch.float32, C * HW * 4), ("gather tokens", (B * N, P * C + extra), BF16, (P * C + extra) * 2)]
    for L, D, C, P, N, B in CONTAIN_HIER:
        H, W = image_hw(N * P)
        out += [("hier x", (B, C, H, W), torch.float32, C * N * P * 4), ("hier h", (B * N, L * D), BF16, 64 * L * D * 2),
                ("hier wf", (L * D, L * D), BF16, L * D * 2)]
    for counts in CONTAIN_RESAMPLE:
        D, B = RESAMPLE_D[0], RESAMPLE_B
        out += [("resample out", (B, counts[0], len(counts) * D), BF16, len(counts) * D * 2)]
        out += [("resample level", (B, n, D), BF16, D * 2) for n in counts]
    return out
