// Argument checks, kernel forms and launch geometry of the row-wise family (rowwise.h), on the scaffold of plan.h.  Plain host
// code: no HIP call, no environment read, no allocation, so every refusal and every geometry is testable on a machine without a GPU.
#include "rowwise.h"

#include <cstdio>

#include "model_ema.h"

namespace sfcvit {

namespace {
bool rate_ok(float p) { return p >= 0.f && p < 1.f; }      // false for NaN
}  // namespace

// Workgroups of the optimizer's grid-stride kernels over n >= 1 elements: one lane per 8, 1 .. ADAMW_MAX_BLOCKS (model_ema.h).
int optim_grid(int64_t n) {
    const int64_t b = ceil_div((n - 1) / 8 + 1, ADAMW_THREADS);            // (n - 1) / 8 + 1: ceil(n / 8) without n + 7
    return int(b > ADAMW_MAX_BLOCKS ? ADAMW_MAX_BLOCKS : b);
}

// ---- LayerNorm ----
void ln_fwd_rows(int M, int D, int &vpl, int &blocks) {
    vpl = D <= 512 ? 1 : D <= 1024 ? 2 : D <= 2048 ? 4 : 8;
    blocks = int(ceil_div(M, ROW_WAVES));
}

LnFwdPlan ln_fwd_plan(const void *x, const void *gamma, const void *beta, const void *y, const float *mean, const float *rstd,
                      int M, int D, const RowwiseKnobs &k) {
    LnFwdPlan p;
    if (!x || !gamma || !beta || !y || !mean || !rstd) REFUSE(SFCVIT_EINVAL, "layernorm_fwd: null pointer");
    if (M <= 0 || D <= 0 || D % 8 || D > LN_FWD_MAX_D)
        REFUSE(SFCVIT_EINVAL, "layernorm_fwd: M=%d D=%d (D %% 8 == 0, D <= %d)", M, D, LN_FWD_MAX_D);
    if (!aligned16(x) || !aligned16(y) || !aligned16(gamma) || !aligned16(beta)) REFUSE(SFCVIT_EINVAL, "layernorm_fwd: alignment");
    // two rows per wave where they fill the lanes (768 = 2 x 96 vectors = 3 per lane, 1 024: 4) and the grid stays large
    p.two_rows = k.ln_fwd_two_rows && (D == 768 || D == 1024) && M >= 4096;
    if (p.two_rows) {
        p.vpl = D == 768 ? 3 : 4;
        p.blocks = int(ceil_div(M, 2 * ROW_WAVES));
    } else {
        ln_fwd_rows(M, D, p.vpl, p.blocks);
    }
    return p;
}

// cols: SFCVIT_LN_COLS=0 runs the 16-byte-vector kernel also at D = 768 / 1 024 (A/B in tools/bench_rowwise.py; at D = 1 024,
// ViT-L, the float-pair form gains 2-6 %: 45.3 -> 44.6 us, with dropout output 61.4 -> 57.9 us at M = 36 864).
// blocks: two (16-byte-vector kernel, 190-222 registers) or three (column-chunk kernel, 145-156) resident waves per SIMD.
// Measured at M 50 176, D 768: 52.1 / 56.4 us with 512 / 768 workgroups of the former, 47.5 / 45.8 of the latter (with dropout
// output and column sums 70.3 / 77.2 and 59.0 / 57.3).  (D = 1 024: 179-194 registers, two waves per SIMD.)
LnBwdPlan ln_bwd_geometry(int M, int D, bool add, const RowwiseKnobs &k) {
    LnBwdPlan p;
    p.M = M;
    p.D = D;
    p.add = add;
    p.cols = k.ln_cols && (D == 768 || D == 1024);
    p.inst = p.cols ? D / 256 : D <= 512 ? 1 : D <= 1024 ? 2 : 4;
    const int64_t want = ceil_div(M, ROW_WAVES);
    const int cap = k.ln_blocks > 0 ? k.ln_blocks : (p.cols && D == 768 ? 768 : 512);
    p.blocks = int(want < cap ? want : cap);
    p.lds = size_t(ROW_WAVES) * 3 * D * sizeof(float);
    p.ws_bytes = int64_t(p.blocks) * 3 * D * int64_t(sizeof(float));
    return p;
}

LnBwdPlan ln_bwd_plan(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma, const void *dx_add,
                      const void *dx, const void *dx_drop, float drop_p, const void *dgamma, const void *dbeta, int M, int D,
                      const void *ws, const RowwiseKnobs &k) {
    LnBwdPlan p;
    if (!dy || !x || !mean || !rstd || !gamma || !dx || !dgamma || !dbeta || !ws) REFUSE(SFCVIT_EINVAL, "layernorm_bwd: null pointer");
    if (M <= 0 || D <= 0 || D % 8 || D > LN_BWD_MAX_D)
        REFUSE(SFCVIT_EINVAL, "layernorm_bwd: M=%d D=%d (D %% 8 == 0, D <= %d)", M, D, LN_BWD_MAX_D);
    if (!aligned16(dy) || !aligned16(x) || !aligned16(dx) || !aligned16(gamma) || !aligned16(dx_add) || !aligned16(dx_drop))
        REFUSE(SFCVIT_EINVAL, "layernorm_bwd: alignment");
    if (dx_drop && !rate_ok(drop_p)) REFUSE(SFCVIT_EINVAL, "layernorm_bwd: dropout p=%g", drop_p);
    return ln_bwd_geometry(M, D, dx_add != nullptr, k);
}

void kernel_name(const LnBwdPlan &p, bool path, char *buf, size_t n) {
    snprintf(buf, n, "ln_bwd%s%s_kernel<%d, %s>", p.cols ? "_cols" : "", path ? "_path" : "", p.inst, p.add ? "true" : "false");
}

// ---- clip + AdamW ----
AdamwPlan adamw_plan(const sfcvit_adamw_args *a, const RowwiseKnobs &k, const char *what) {
    AdamwPlan p;
    if (!a) REFUSE(SFCVIT_EINVAL, "%s: null pointer (a)", what);
    if (!a->param || !a->master || !a->grad || !a->m || !a->v)
        REFUSE(SFCVIT_EINVAL, "%s: null pointer (param / master / grad / m / v)", what);
    if (a->n <= 0 || (a->step < 1 && !a->dev_state)) REFUSE(SFCVIT_EINVAL, "%s: n=%lld step=%d", what, (long long)a->n, a->step);
    if (!aligned16(a->param) || !aligned16(a->master) || !aligned16(a->grad) || !aligned16(a->m) || !aligned16(a->v))
        REFUSE(SFCVIT_EINVAL, "%s: buffers must be 16-byte aligned", what);
    p.grid = optim_grid(a->n);
    p.nt = k.adamw_nt & 3;
    return p;
}

// ---- column sums ----
ColsumPlan colsum_geometry(int M, int N) {
    ColsumPlan p;
    p.col_blocks = int(ceil_div(N, 256));
    p.row_blocks = 1024 / p.col_blocks;      // ~1024 workgroups in the first pass; the partials stay a few MB
    if (p.row_blocks > 256) p.row_blocks = 256;
    if (p.row_blocks < 1) p.row_blocks = 1;
    p.rpb = int(ceil_div(ceil_div(M, p.row_blocks), 8) * 8);
    p.row_blocks = int(ceil_div(M, p.rpb));
    p.ws_bytes = int64_t(p.row_blocks) * N * int64_t(sizeof(float));
    return p;
}

ColsumPlan colsum_plan(const void *x, int M, int N, int ld, const void *out, const void *workspace, int64_t workspace_bytes) {
    ColsumPlan p;
    if (!x || !out) REFUSE(SFCVIT_EINVAL, "colsum: null pointer");
    if (M <= 0 || N <= 0 || N % 8 || ld % 8 || ld < N) REFUSE(SFCVIT_EINVAL, "colsum: M=%d N=%d ld=%d (N, ld %% 8 == 0)", M, N, ld);
    if (!aligned16(x)) REFUSE(SFCVIT_EINVAL, "colsum: alignment");
    const ColsumPlan g = colsum_geometry(M, N);
    if (!workspace || workspace_bytes < g.ws_bytes) REFUSE(SFCVIT_EINVAL, "colsum: workspace of %lld bytes needed", (long long)g.ws_bytes);
    return g;
}

// ---- refusals + a grid ----
RowGridPlan transpose_plan(const void *src, int R, int C, int lds, const void *dst, int ldd) {
    RowGridPlan p;
    if (!src || !dst) REFUSE(SFCVIT_EINVAL, "transpose: null pointer");
    if (R <= 0 || C <= 0 || R % 8 || C % 8 || lds % 8 || ldd % 8 || lds < C || ldd < R)
        REFUSE(SFCVIT_EINVAL, "transpose: R=%d C=%d lds=%d ldd=%d (multiples of 8)", R, C, lds, ldd);
    if (!aligned16(src) || !aligned16(dst)) REFUSE(SFCVIT_EINVAL, "transpose: alignment");
    p.grid = int(ceil_div(C, 64));           // 64 x 64 tiles
    p.grid_y = int(ceil_div(R, 64));
    return p;
}

RowGridPlan transpose_batched_plan(const void *src_base, const void *dst_base, const void *tiles, int n_tiles) {
    RowGridPlan p;
    if (!src_base || !dst_base || !tiles || n_tiles <= 0) REFUSE(SFCVIT_EINVAL, "transpose_batched: null pointer or no tiles");
    if (!aligned16(src_base) || !aligned16(dst_base)) REFUSE(SFCVIT_EINVAL, "transpose_batched: alignment");
    p.grid = n_tiles;
    return p;
}

PlanStatus gelu_plan(bool bwd, const void *dy, const void *x, const void *out, int64_t n) {
    PlanStatus p;
    if ((bwd && !dy) || !x || !out || n <= 0 || n % 8)
        REFUSE(SFCVIT_EINVAL, "gelu_%s: n=%lld must be a positive multiple of 8", bwd ? "bwd" : "fwd", (long long)n);
    return p;
}

PlanStatus gelu_drop_plan(bool bwd, const void *dy, const void *x, const void *out, int rows, int cols, float drop_p) {
    PlanStatus p;
    const char *what = bwd ? "gelu_drop_bwd" : "gelu_drop_fwd";
    if (bwd && !dy) REFUSE(SFCVIT_EINVAL, "%s: null pointer", what);
    if (!x || !out || rows <= 0 || cols <= 0 || cols % 8) REFUSE(SFCVIT_EINVAL, "%s: rows=%d cols=%d (cols %% 8 == 0)", what, rows, cols);
    if (!rate_ok(drop_p)) REFUSE(SFCVIT_EINVAL, "%s: dropout p=%g", what, drop_p);
    return p;
}

PlanStatus dropout_mask_plan(const void *out, int64_t rows, int cols, float drop_p) {
    PlanStatus p;
    if (!out || rows <= 0 || cols <= 0 || !rate_ok(drop_p)) REFUSE(SFCVIT_EINVAL, "dropout_mask: bad argument");
    return p;
}

RowGridPlan soft_ce_plan(const void *logits, const float *targets, const float *loss_rows, int B, int C, int ld) {
    RowGridPlan p;
    if (!logits || !targets || !loss_rows) REFUSE(SFCVIT_EINVAL, "soft_ce: null pointer");
    if (B <= 0 || C <= 0 || ld < C) REFUSE(SFCVIT_EINVAL, "soft_ce: B=%d C=%d ld=%d", B, C, ld);
    p.grid = int(ceil_div(B, ROW_WAVES));
    return p;
}

RowGridPlan sumsq_plan(const void *g, int64_t n, const float *out, const void *workspace) {
    RowGridPlan p;
    if (!g || !out || !workspace || n <= 0) REFUSE(SFCVIT_EINVAL, "sumsq: bad argument");
    if (!aligned16(g)) REFUSE(SFCVIT_EINVAL, "sumsq: alignment");
    const int max_parts = SFCVIT_SUMSQ_WORKSPACE_BYTES / int(sizeof(float));      // one partial per workgroup
    p.grid = optim_grid(n);
    if (p.grid > max_parts) p.grid = max_parts;
    return p;
}

RowGridPlan step_advance_plan(const void *state) {
    RowGridPlan p;
    if (!state || !aligned16(state)) REFUSE(SFCVIT_EINVAL, "step_advance: state must be a 16-byte aligned device buffer of 8 words");
    p.grid = 1;
    return p;
}

}  // namespace sfcvit
