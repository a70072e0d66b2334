// Argument checks and launch geometry of sfcvit_add_layernorm_scale_fwd / sfcvit_layernorm_bwd_scale (layer_scale.h), on the
// scaffold of plan.h.  Plain host code: no HIP call, no allocation, so every refusal is testable on a machine without a GPU.
#include "layer_scale.h"

#include <climits>
#include <cstdio>

namespace sfcvit {

AddLnScalePlan add_ln_scale_plan(const void *branch, const void *x, const void *lam, const void *gamma, const void *beta,
                                 const void *s, const void *y, const float *mean, const float *rstd, int B, int N, int D, float rate) {
    AddLnScalePlan p;
    const char *what = "add_layernorm_scale_fwd";
    if (!branch || !x || !lam || !gamma || !beta || !s || !y || !mean || !rstd)
        REFUSE(SFCVIT_EINVAL, "%s: null pointer (branch / x / lam / gamma / beta / s / y / mean / rstd)", what);
    if (B <= 0 || N <= 0) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d (B, N >= 1)", what, B, N);
    if (int64_t(B) * N > INT_MAX) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d: B * N rows leave int", what, B, N);
    if (D < 8 || D % 8 || D > LN_FWD_MAX_D) REFUSE(SFCVIT_EINVAL, "%s: D=%d (D %% 8 == 0, 8 <= D <= %d)", what, D, LN_FWD_MAX_D);
    if (!aligned16(branch) || !aligned16(x) || !aligned16(lam) || !aligned16(gamma) || !aligned16(beta) || !aligned16(s) || !aligned16(y))
        REFUSE(SFCVIT_EINVAL, "%s: branch, x, lam, gamma, beta, s and y must be 16-byte aligned", what);
    if (!(rate >= 0.f && rate < 1.f)) REFUSE(SFCVIT_EINVAL, "%s: rate=%g outside [0, 1)", what, rate);
    p.M = B * N;
    const uint64_t bytes = uint64_t(p.M) * D * 2;
    // a wave stores a row of s before it has read the row's gamma / beta, and y while other waves still read their inputs
    const auto shares = [bytes](const void *a, const void *b) { return overlap(a, bytes, b, bytes); };
    if (shares(s, x) || shares(s, branch) || shares(y, x) || shares(y, branch) || shares(s, y))
        REFUSE(SFCVIT_EINVAL, "%s: s or y overlaps an input or the other output (no in-place form)", what);
    ln_fwd_rows(p.M, D, p.vpl, p.blocks);
    return p;
}

LnBwdScalePlan ln_bwd_scale_geometry(int M, int D, bool add, const RowwiseKnobs &k) {
    LnBwdScalePlan p = ln_bwd_geometry(M, D, add, k);          // its form, its grid (and with them the summation order), its LDS region
    p.ws_bytes = int64_t(p.blocks) * 4 * D * int64_t(sizeof(float));
    return p;
}

LnBwdScalePlan ln_bwd_scale_plan(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma,
                                 const void *dx_add, const void *branch, const void *lam, const void *dx, const void *dx_drop,
                                 float drop_p, const void *dgamma, const void *dbeta, const void *dlam, int B, int rows_per_image,
                                 int D, const void *ws, float path_rate, const RowwiseKnobs &k) {
    LnBwdScalePlan p;
    const char *what = "layernorm_bwd_scale";
    if (!dy || !x || !mean || !rstd || !gamma || !branch || !lam || !dx || !dgamma || !dbeta || !dlam || !ws)
        REFUSE(SFCVIT_EINVAL, "%s: null pointer", what);
    if (!dx_drop) REFUSE(SFCVIT_EINVAL, "%s: dx_drop is missing (null pointer): the scaled gradient has no other output", what);
    if (B <= 0 || rows_per_image <= 0) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d (B, rows_per_image >= 1)", what, B, rows_per_image);
    if (int64_t(B) * rows_per_image > INT_MAX)
        REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d: B * rows_per_image rows leave int", what, B, rows_per_image);
    if (D < 8 || D % 8 || D > LN_BWD_MAX_D) REFUSE(SFCVIT_EINVAL, "%s: D=%d (D %% 8 == 0, 8 <= D <= %d)", what, D, LN_BWD_MAX_D);
    if (!aligned16(dy) || !aligned16(x) || !aligned16(gamma) || !aligned16(dx_add) || !aligned16(branch) || !aligned16(lam) ||
        !aligned16(dx) || !aligned16(dx_drop))
        REFUSE(SFCVIT_EINVAL, "%s: dy, x, gamma, dx_add, branch, lam, dx and dx_drop must be 16-byte aligned", what);
    if (!(drop_p >= 0.f && drop_p < 1.f)) REFUSE(SFCVIT_EINVAL, "%s: dropout p=%g outside [0, 1)", what, drop_p);
    if (!(path_rate >= 0.f && path_rate < 1.f)) REFUSE(SFCVIT_EINVAL, "%s: rate=%g outside [0, 1)", what, path_rate);
    return ln_bwd_scale_geometry(B * rows_per_image, D, dx_add != nullptr, k);
}

void scale_kernel_name(const LnBwdScalePlan &p, char *buf, size_t n) {
    snprintf(buf, n, "ln_bwd%s_scale_kernel<%d, %s>", p.cols ? "_cols" : "", p.inst, p.add ? "true" : "false");
}

}  // namespace sfcvit
