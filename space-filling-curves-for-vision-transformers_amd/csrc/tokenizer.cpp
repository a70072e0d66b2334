// Argument checks, kernel forms and launch geometry of the tokenizer family (tokenizer.h), on the scaffold of plan.h.  Plain
// host code: no HIP call, no environment read, no allocation, so every refusal and every geometry is testable on a machine
// without a GPU.  Sizes are worked out in int64_t (ceil_div) and narrowed where the refusals before have bounded them.
#include "tokenizer.h"

#include <cstdio>

#include "rowwise.h"

namespace sfcvit {

thread_local KernelNote g_tokenizer;

namespace {
constexpr int64_t INT_LIMIT = 0x7fffffff;
bool aligned8(const void *ptr) { return aligned(ptr, 8); }
// Workgroups of a grid-stride kernel over rows * per_row items, 256 per workgroup, at most 65 536; rows * per_row may pass
// int64_t (extents no tensor has), the result cannot.
int stride_blocks(int64_t rows, int64_t per_row) {
    const int64_t cap = int64_t(1) << 16;
    if (rows >= cap * 256) return int(cap);                 // per_row >= 1
    const int64_t b = ceil_div(rows * per_row, 256);
    return int(b < cap ? b : cap);
}
}  // namespace

// ---- token gathers ----
// TILES: tokens that are 16 x 16 pixel tiles of an fp32 image; one workgroup = a pair of tokens x 4 upw images.
GatherPlan gather_tiles_plan(const char *what, const void *x, const int32_t *pix, const int32_t *origin, const int32_t *perm, int B,
                             int C, int H, int W, int N, const void *tokens, int ld, const TokenizerKnobs &k) {
    GatherPlan p;
    if (!x || !pix || !origin || !tokens) REFUSE(SFCVIT_EINVAL, "%s: null pointer", what);
    if (B <= 0 || C < 1 || C > 4 || H <= 0 || W <= 0 || N <= 0 || int64_t(N) * 256 != int64_t(H) * W || (W & 7) || (H & 15))
        REFUSE(SFCVIT_EINVAL, "%s: B=%d C=%d H=%d W=%d N=%d (1 <= C <= 4, W %% 8 == 0, H %% 16 == 0, N * 256 == H * W)", what, B, C, H, W, N);
    if (ld != 256 * C) REFUSE(SFCVIT_EINVAL, "%s: ld=%d (must be 256 * C = %d)", what, ld, 256 * C);
    if (!aligned16(x) || !aligned16(tokens)) REFUSE(SFCVIT_EINVAL, "%s: x and tokens must be 16-byte aligned", what);
    if (int64_t(16) * W * W >= (int64_t(1) << 32)) REFUSE(SFCVIT_EINVAL, "%s: W=%d too wide", what, W);
    // the kernels index a plane with int
    if (int64_t(H) * W > INT_LIMIT) REFUSE(SFCVIT_EINVAL, "%s: H=%d W=%d: H * W must fit 31 bits", what, H, W);
    p.form = GatherForm::TILES;
    p.mix = perm != nullptr;
    p.C = C;
    p.HW = H * W;
    // images per wave (A/B: 2 = fewer, longer workgroups); the mixing form holds twice the lines and exists for 1 only
    p.upw = (!p.mix && k.gather_u == 2) ? 2 : 1;
    // nontemporal loads (1) and stores (2).  The gather is the first kernel of a step: L2 and the memory-side cache are full
    // of the optimizer's dirty lines, and every line an ordinary load allocates evicts one of them -- a write-back that
    // shares HBM with the gather (75.8 us against 42.1 us with clean caches; a plain fp32 -> bf16 cast of the image suffers
    // the same: 69 vs 37 us).  Streaming loads do not allocate: 46.0 us; with streaming stores 43.2 us alone, 44.0 us in
    // the step (profiles/r4/gather_ab.txt).  SFCVIT_GATHER_NT=0..3 for the A/B.
    p.nt = (k.gather_nt >= 1 && k.gather_nt <= 3) ? k.gather_nt : 0;
    const int64_t gy = ceil_div(B, 4 * p.upw);
    if (gy > 65535) REFUSE(SFCVIT_EINVAL, "%s: batch %d too large", what, B);
    p.grid_x = int(ceil_div(N, 2));
    p.grid_y = int(gy);
    p.threads = GATHER_THREADS;
    p.wmagic = uint32_t((uint64_t(1) << 32) / uint32_t(W)) + 1;
    p.lds = 1024 + size_t(4 * p.upw) * C * 1024;
    return p;
}

// P256: P <= 256 pixels per token, C <= 4 and two tokens x GATHER_IMG rows in 64 KiB of LDS: one pixel per thread, two tokens
// per workgroup.  ROWS: any other shape, one token per workgroup.
GatherPlan gather_plan(const char *what, const void *x, int x_is_bf16, const int32_t *pix, const int32_t *perm, int B, int C, int HW,
                       int N, int P, const void *tokens, int ld) {
    GatherPlan p;
    if (!x || !pix || !tokens) REFUSE(SFCVIT_EINVAL, "%s: null pointer", what);
    if (B <= 0 || C <= 0 || HW <= 0 || N <= 0 || P <= 0 || int64_t(N) * P != HW)
        REFUSE(SFCVIT_EINVAL, "%s: B=%d C=%d HW=%d N=%d P=%d (N * P must equal H * W)", what, B, C, HW, N, P);
    const int64_t K = int64_t(P) * C;
    if (ld < K || ld % 8 || ld > 32768) REFUSE(SFCVIT_EINVAL, "%s: ld=%d (>= P * C = %lld, multiple of 8, <= 32768)", what, ld, (long long)K);
    if (!aligned16(tokens)) REFUSE(SFCVIT_EINVAL, "%s: tokens must be 16-byte aligned", what);
    const int64_t gy = ceil_div(B, GATHER_IMG);
    if (gy > 65535) REFUSE(SFCVIT_EINVAL, "%s: batch %d too large", what, B);
    p.mix = perm != nullptr;
    p.x_bf16 = x_is_bf16 != 0;
    p.C = C;
    p.HW = HW;
    p.grid_y = int(gy);
    const size_t lds2 = size_t(2) * GATHER_IMG * ld * 2;
    if (P <= GATHER_THREADS && C <= 4 && lds2 <= 64 * 1024) {
        p.form = GatherForm::P256;
        p.grid_x = int(ceil_div(N, 2));
        p.threads = 2 * GATHER_THREADS;
        p.lds = lds2;
    } else {
        p.form = GatherForm::ROWS;
        p.grid_x = N;
        p.threads = GATHER_THREADS;
        p.lds = size_t(ld) * 2;
    }
    return p;
}

GatherPlan gather_mix_plan(const void *x, const int32_t *pix, const int32_t *origin, const int32_t *perm, const uint32_t *rec, int B,
                           int C, int H, int W, int N, int P, const void *tokens, int ld, const TokenizerKnobs &k) {
    GatherPlan p;
    if (!perm || !rec) REFUSE(SFCVIT_EINVAL, "tokens_gather_mix: null perm / rec (the unmixed gather is sfcvit_tokens_gather)");
    if (H <= 0 || W <= 0 || int64_t(H) * W > INT_LIMIT) REFUSE(SFCVIT_EINVAL, "tokens_gather_mix: H=%d W=%d", H, W);
    if (!aligned16(x)) REFUSE(SFCVIT_EINVAL, "tokens_gather_mix: x must be 16-byte aligned");
    if (origin) {
        if (P != 256) REFUSE(SFCVIT_EINVAL, "tokens_gather_mix: P=%d with a tile origin table (16 x 16 tiles: P = 256)", P);
        return gather_tiles_plan("tokens_gather_mix", x, pix, origin, perm, B, C, H, W, N, tokens, ld, k);
    }
    return gather_plan("tokens_gather_mix", x, 0, pix, perm, B, C, H * W, N, P, tokens, ld);
}

void kernel_name(const GatherPlan &p, char *buf, size_t n) {
    const char *in = p.mix ? "mix" : p.x_bf16 ? "bf16" : "fp32";
    if (p.form == GatherForm::TILES) snprintf(buf, n, "tokens_gather_tiles_kernel<%d, %s>", p.C, in);
    else snprintf(buf, n, "%s<%s>", p.form == GatherForm::P256 ? "tokens_gather_p256_kernel" : "tokens_gather_kernel", in);
}

// ---- fused gather + projection ----
int pe2_bwd_row_range(int B, int ncls, const int32_t *cnt, int tiles, int *nz_out) {
    const int G = 8 * (32 / tiles > 1 ? 32 / tiles : 1);
    int64_t M = 0;
    for (int c = 0; c < ncls; c++) M += int64_t(cnt[c]) * B;
    int64_t kr = ceil_div(M / G, PE2_BW_ROWS) * PE2_BW_ROWS;
    if (kr < PE2_BW_ROWS) kr = PE2_BW_ROWS;
    for (;; kr += PE2_BW_ROWS) {
        int64_t nz = 0;
        for (int c = 0; c < ncls; c++) nz += ceil_div(int64_t(cnt[c]) * B, kr);
        if (nz <= G) { *nz_out = int(nz); return int(kr); }
    }
}

int64_t pe2_bwd_workspace(int C, int D) {
    const int64_t tiles = int64_t(D / 256) * C;
    const int64_t G = 8 * (32 / tiles > 1 ? 32 / tiles : 1);
    return G * D * C * 256 * int64_t(sizeof(float));
}

// A patch embedding whose weight [D, Kp] passes 2^35 elements has a forward workspace of 512 GiB: no such tensor exists, and
// below that bound every size and grid of the generic and the tiled form fits its type (ws_bytes stays 0 above it).
PatchEmbedPlan patch_embed_geometry(int B, int C, int N, int P, int D, bool bwd) {
    PatchEmbedPlan p;
    p.bwd = bwd;
    if (B <= 0 || C <= 0 || N <= 0 || P <= 0 || D <= 0) return p;
    const int64_t M = int64_t(B) * N, K = int64_t(C) * P, Kp = ceil_div(K, 8) * 8;
    if (M > INT_LIMIT / 2 || Kp > (int64_t(1) << 35) / D) return p;
    p.M = int(M);
    p.K = int(K);
    p.Kp = int(Kp);
    p.lds = 4 * PATCH_TILE_BYTES;
    const int64_t tiles_d = ceil_div(D, PATCH_BM), tiles_f = ceil_div(Kp, PATCH_BN);
    if (!bwd) {
        p.wp_bytes = D * Kp * 2;
        p.permute_grid = int(ceil_div(D * Kp, 256));
        p.ws_bytes = ceil_div(p.wp_bytes * PE2_MAXCLS, 16) * 16;      // up to 8 class-permuted copies of W (tiled forward)
        return p;
    }
    // generic backward: ~1024 workgroups, each k-range at least one k-tile
    const int64_t ktiles = ceil_div(M, PATCH_BK);
    int64_t splits = ceil_div(1024, tiles_d * tiles_f);
    if (splits > ktiles) splits = ktiles;
    p.splits = int(splits);
    p.m_per_split = int(ceil_div(ktiles, splits) * PATCH_BK);
    p.zs = int(ceil_div(M, p.m_per_split));
    p.slab_bytes = splits * D * Kp * int64_t(sizeof(float));
    p.reduce_grid = int(ceil_div(D * Kp, 16));
    const int64_t bias_ws = colsum_geometry(p.M, D).ws_bytes;        // dbias reuses the buffer after the slabs are reduced
    const int64_t tiled = (P == 256 && D % 256 == 0) ? pe2_bwd_workspace(C, D) : 0;
    p.ws_bytes = p.slab_bytes > bias_ws ? p.slab_bytes : bias_ws;
    if (tiled > p.ws_bytes) p.ws_bytes = tiled;
    return p;
}

PatchEmbedPlan patch_embed_plan(const sfcvit_patch_embed_args *a, bool bwd) {
    PatchEmbedPlan p;
    const char *what = bwd ? "patch_embed_bwd" : "patch_embed_fwd";
    if (!a || !a->x || !a->pix || !a->y) REFUSE(SFCVIT_EINVAL, "%s: null pointer", what);
    if (a->B <= 0 || a->C <= 0 || a->HW <= 0 || a->N <= 0 || a->P <= 0 || a->D <= 0) REFUSE(SFCVIT_EINVAL, "%s: non-positive dimension", what);
    if (int64_t(a->N) * a->P != a->HW)
        REFUSE(SFCVIT_EINVAL, "%s: N*P=%lld must equal H*W=%d", what, (long long)a->N * a->P, a->HW);
    if (a->D % 8 != 0) REFUSE(SFCVIT_EINVAL, "%s: D=%d must be a multiple of 8", what, a->D);
    if (int64_t(a->B) * a->N > INT_LIMIT / 2) REFUSE(SFCVIT_EINVAL, "%s: B*N too large", what);
    if (!aligned16(a->x) || !aligned16(a->pix) || !aligned16(a->y)) REFUSE(SFCVIT_EINVAL, "%s: alignment", what);
    // pe_fwd_kernel reads the bias with 8-byte loads; the same rule as sfcvit_hier_tokenizer_fwd
    if (!aligned16(a->w) || !aligned8(a->bias)) REFUSE(SFCVIT_EINVAL, "%s: weight / bias alignment (w 16 bytes, bias 8 bytes)", what);
    if (!bwd && !a->w) REFUSE(SFCVIT_EINVAL, "patch_embed_fwd: null weight");
    if (bwd && !a->dw) REFUSE(SFCVIT_EINVAL, "patch_embed_bwd: null dw");
    const PatchEmbedPlan g = patch_embed_geometry(a->B, a->C, a->N, a->P, a->D, bwd);
    if (!g.M) REFUSE(SFCVIT_EINVAL, "%s: C*P=%lld D=%d too large", what, (long long)a->C * a->P, a->D);
    if (!a->workspace || a->workspace_bytes < g.ws_bytes || !aligned16(a->workspace))
        REFUSE(SFCVIT_EINVAL, "%s: workspace of %lld bytes needed", what, (long long)g.ws_bytes);
    p = g;
    p.x_bf16 = a->x_is_bf16 != 0;
    p.dbias = bwd && a->dbias;
    const int64_t tiles_d = ceil_div(a->D, PATCH_BM), tiles_f = ceil_div(p.Kp, PATCH_BN);
    int64_t grid = bwd ? tiles_f * tiles_d * p.zs : ceil_div(a->D, PATCH_BN) * ceil_div(p.M, PATCH_BM);
    // tiles / strips: the coalesced kernels (16-byte loads of x: aligned above, and H * W = 256 N).  Their workspace need is
    // within ws_bytes whatever the class counts are (at most PE2_MAXCLS copies of W; nz <= G slabs): check_tokenizer sweeps it.
    if (a->desc && a->P == 256 && a->D % PE2_TN == 0 && a->desc_ncls > 0 && a->desc_ncls <= PE2_MAXCLS) {
        p.form = PeForm::TILED;
        if (!bwd) {
            int64_t row_tiles = 0;
            for (int c = 0; c < a->desc_ncls; c++) row_tiles += ceil_div(int64_t(a->desc_cnt[c]) * a->B, PE2_TM);
            p.n_row_tiles = int(row_tiles);
            p.groups = int(ceil_div(row_tiles, 8));
            p.wp_bytes *= a->desc_ncls;
            p.permute_grid = 1024;                           // grid-stride
            p.lds = PE2_FWD_LDS;
            grid = int64_t(p.groups) * 8 * (a->D / PE2_TN);
        } else {
            const int tiles = (a->D / 256) * a->C;
            p.KR = pe2_bwd_row_range(a->B, a->desc_ncls, a->desc_cnt, tiles, &p.nz);
            p.slab_bytes = int64_t(p.nz) * a->D * a->C * 256 * int64_t(sizeof(float));
            p.reduce_grid = int(ceil_div(int64_t(a->D) * a->C * 256, 256));
            p.lds = PE2_BWD_LDS;
            grid = ceil_div(p.nz, 8) * 8 * tiles;            // row ranges dealt to the 8 XCD slots
        }
    }
    if (grid > INT_LIMIT) REFUSE(SFCVIT_EINVAL, "%s: B*N=%d D=%d: too many workgroups", what, p.M, a->D);
    p.grid = int(grid);
    return p;
}

void kernel_name(const PatchEmbedPlan &p, char *buf, size_t n) {
    snprintf(buf, n, "%s_%s_kernel<%s>", p.form == PeForm::TILED ? "pe2" : "pe", p.bwd ? "bwd" : "fwd", p.x_bf16 ? "bf16" : "fp32");
}

// ---- hierarchical tokenizer ----
// 64 rows of the concatenation (2 E + 16 bytes each) and of the tokens of all levels (2 kp_sum + 16) within 160 KiB.
bool hier_envelope(int L, int D, int C, const int32_t *P, int &E, int &kp_sum) {
    if (L < 1 || L > HT_MAXL || D <= 0 || D % 64 || (int64_t(L) * D) % 256 || C <= 0 || !P) return false;
    int64_t kp = 0;
    for (int l = 0; l < L; l++) {
        const int64_t K = int64_t(P[l]) * C;
        if (P[l] <= 0 || K % 8) return false;
        kp += (K + 31) & ~int64_t(31);
    }
    const int64_t e = int64_t(L) * D;
    if (HT_ROWS * (2 * e + 16) + HT_ROWS * (2 * kp + 16) > HT_LDS_LIMIT) return false;
    E = int(e);
    kp_sum = int(kp);
    return true;
}

HierPlan hier_plan(const sfcvit_hier_args *a) {
    HierPlan p;
    if (!a || !a->x || !a->h || (a->wf && !a->y)) REFUSE(SFCVIT_EINVAL, "hier_tokenizer_fwd: null pointer");
    if (a->B <= 0 || a->C <= 0 || a->HW <= 0 || a->N <= 0)
        REFUSE(SFCVIT_EINVAL, "hier_tokenizer_fwd: B=%d C=%d HW=%d N=%d", a->B, a->C, a->HW, a->N);
    if (!hier_envelope(a->L, a->D, a->C, a->P, p.E, p.kp_sum))
        REFUSE(SFCVIT_EINVAL, "hier_tokenizer_fwd: L=%d D=%d C=%d outside the fused kernel's envelope "
               "(1..4 levels, D %% 64 == 0, L*D %% 256 == 0, P*C %% 8 == 0, 64 rows of L*D + sum K in 160 KiB LDS)", a->L, a->D, a->C);
    if (int64_t(a->B) * a->N >= (int64_t(1) << 31) - HT_ROWS) REFUSE(SFCVIT_EINVAL, "hier_tokenizer_fwd: too many token rows");
    for (int l = 0; l < a->L; l++) {
        if (!a->pix[l] || !a->w[l]) REFUSE(SFCVIT_EINVAL, "hier_tokenizer_fwd: level %d: null pointer", l);
        if (int64_t(a->P[l]) * a->N != a->HW)
            REFUSE(SFCVIT_EINVAL, "hier_tokenizer_fwd: level %d: N * P = %d * %d != H*W = %d (levels must share the token count)", l,
                   a->N, a->P[l], a->HW);
        if (!aligned16(a->w[l]) || !aligned8(a->b[l])) REFUSE(SFCVIT_EINVAL, "hier_tokenizer_fwd: level %d: weight / bias alignment", l);
    }
    if (!aligned16(a->wf) || !aligned16(a->h) || !aligned16(a->y) || !aligned8(a->bf))
        REFUSE(SFCVIT_EINVAL, "hier_tokenizer_fwd: fusion weight / output alignment");
    p.fuse = a->wf != nullptr;
    p.x_bf16 = a->x_is_bf16 != 0;
    p.M = a->B * a->N;
    p.h_stride = 2 * p.E + 16;
    p.a_stride = 2 * p.kp_sum + 16;
    p.lds = HT_ROWS * p.a_stride + (p.fuse ? HT_ROWS * p.h_stride : 0);
    p.grid = int(ceil_div(p.M, HT_ROWS));
    return p;
}

void kernel_name(const HierPlan &p, char *buf, size_t n) {
    snprintf(buf, n, "hier_fwd_kernel<%s, %s>", p.x_bf16 ? "bf16" : "fp32", p.fuse ? "fuse" : "levels");
}

ResamplePlan resample_plan(bool bwd, const void *const *lev, const int32_t *n_tokens, int L, int B, int N0, int D, const void *cat) {
    ResamplePlan p;
    p.bwd = bwd;
    const char *what = bwd ? "hier_resample_concat_bwd" : "hier_resample_concat";
    if (!lev || !n_tokens || !cat) REFUSE(SFCVIT_EINVAL, "%s: null pointer", what);
    if (L < 1 || L > RS_MAXL || B <= 0 || N0 <= 0 || D <= 0 || D % 8)
        REFUSE(SFCVIT_EINVAL, "%s: L=%d B=%d N0=%d D=%d (1 <= L <= %d, D %% 8 == 0)", what, L, B, N0, D, RS_MAXL);
    if (n_tokens[0] != N0) REFUSE(SFCVIT_EINVAL, "%s: the first level has %d tokens, not N0 = %d", what, n_tokens[0], N0);
    if (!aligned16(cat)) REFUSE(SFCVIT_EINVAL, "%s: alignment", what);
    for (int l = 0; l < L; l++)
        if (!lev[l] || n_tokens[l] <= 0 || !aligned16(lev[l])) REFUSE(SFCVIT_EINVAL, "%s: level %d (pointer / token count / alignment)", what, l);
    // one thread per 8 columns of a row: of the output (forward), of level l's gradient (backward)
    if (!bwd) p.blocks[0] = stride_blocks(int64_t(B) * N0, int64_t(L) * (D / 8));
    else
        for (int l = 0; l < L; l++) p.blocks[l] = stride_blocks(int64_t(B) * n_tokens[l], D / 8);
    return p;
}

void kernel_name(const ResamplePlan &p, char *buf, size_t n) {
    snprintf(buf, n, "hier_resample_concat%s_kernel", p.bwd ? "_bwd" : "");
}

// ---- MixUp / CutMix ----
MixPlan mix_images_plan(const void *x, const int32_t *perm, const uint32_t *rec, const void *out, int B, int C, int H, int W) {
    MixPlan p;
    if (!x || !perm || !rec || !out) REFUSE(SFCVIT_EINVAL, "mix_images: null pointer");
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || int64_t(H) * W > INT_LIMIT || int64_t(B) * C > INT_LIMIT)
        REFUSE(SFCVIT_EINVAL, "mix_images: B=%d C=%d H=%d W=%d", B, C, H, W);
    const uint64_t bytes = uint64_t(B) * C * (uint64_t(H) * W) * 4;         // < 2^64
    if (overlap(x, bytes, out, bytes))
        REFUSE(SFCVIT_EINVAL, "mix_images: out must not alias x (an image is also read as its partner's partner)");
    if (!aligned16(x) || !aligned16(out)) REFUSE(SFCVIT_EINVAL, "mix_images: x and out must be 16-byte aligned");
    p.HW = H * W;
    p.vec = (p.HW & 3) ? 1 : 4;
    p.grid = int(ceil_div(p.HW / p.vec, MIX_THREADS));
    const int64_t planes = int64_t(B) * C;                                   // walked with the stride of grid_y
    p.grid_y = int(planes < 4096 ? planes : 4096);
    return p;
}

MixPlan soft_ce_pair_plan(const void *logits, const int64_t *y_a, const int64_t *y_b, const uint32_t *rec, const float *loss_rows, int B,
                          int C, int ld) {
    MixPlan p;
    if (!logits || !y_a || !y_b || !rec || !loss_rows) REFUSE(SFCVIT_EINVAL, "soft_ce_pair: null pointer");
    if (B <= 0 || C <= 0 || ld < C) REFUSE(SFCVIT_EINVAL, "soft_ce_pair: B=%d C=%d ld=%d", B, C, ld);
    p.grid = int(ceil_div(B, MIX_WAVES));                                    // one wave per row
    return p;
}

}  // namespace sfcvit

extern "C" int sfcvit_last_tokenizer_kernel(char *buf, int n) { return sfcvit::g_tokenizer.read(buf, n); }
