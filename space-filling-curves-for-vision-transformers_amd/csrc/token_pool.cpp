// Argument checks and launch geometry of sfcvit_cls_prepend_fwd / _bwd and sfcvit_token_pool_fwd / _bwd (token_pool.h), on
// the scaffold of plan.h.  Plain host code: no HIP call, no allocation, so every refusal is testable on a machine without
// a GPU.
#include "token_pool.h"

#include "common_host.h"

namespace sfcvit {

thread_local KernelNote g_token_pool;

ClsPrependPlan cls_prepend_plan(const char *what, int B, int N, int D) {
    ClsPrependPlan p;
    if (B <= 0 || N <= 0) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d (B, N >= 1)", what, B, N);
    if (D < 8 || D % 8) REFUSE(SFCVIT_EINVAL, "%s: D=%d must be a positive multiple of 8 (16-byte vectors)", what, D);
    const int64_t nd1 = (int64_t(N) + 1) * D;                   // < 2^62
    if (nd1 > (INT64_MAX / 4) / B) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d D=%d: the byte counts leave int64", what, B, N, D);
    p.dv = D / 8;
    p.xv = int64_t(N) * p.dv;
    const int64_t fwd_blocks = ceil_div(p.xv + p.dv, TP_THREADS), bwd_blocks = ceil_div(p.xv, TP_THREADS);
    p.slabs = int(ceil_div(p.dv, CP_CV));
    if (fwd_blocks + p.slabs > INT32_MAX) REFUSE(SFCVIT_EINVAL, "%s: N=%d D=%d beyond the launch grid", what, N, D);
    p.fwd_blocks = int(fwd_blocks);
    p.bwd_blocks = int(bwd_blocks);
    // copies: as many images per lane (1, 2, 4, 8) as still leave ~1024 workgroups
    const int64_t want = fwd_blocks * B / 1024;
    p.imgs = 1;
    while (p.imgs < CP_MAX_IMGS && p.imgs * 2 <= want) p.imgs *= 2;
    const int64_t groups = ceil_div(B, p.imgs);
    if (groups > 65535) REFUSE(SFCVIT_EINVAL, "%s: B=%d beyond the launch grid", what, B);
    p.groups = int(groups);
    // dcls: one range of the batch up to 2048 images (64 per image lane), whole rounds of the 32 image lanes
    const int64_t splits = ceil_div(B, CP_MAX_ROWS);
    p.rows = int(ceil_div(ceil_div(B, splits), CP_RL) * CP_RL);
    p.splits = int(ceil_div(B, p.rows));
    p.ws_bytes = p.splits > 1 ? int64_t(p.splits) * D * int64_t(sizeof(float)) : 0;
    return p;
}

TokenPoolPlan token_pool_plan(const char *what, int B, int T, int D, int first, int count) {
    TokenPoolPlan p;
    if (B <= 0 || T <= 0) REFUSE(SFCVIT_EINVAL, "%s: B=%d T=%d (B, T >= 1)", what, B, T);
    if (D < 8 || D % 8) REFUSE(SFCVIT_EINVAL, "%s: D=%d must be a positive multiple of 8 (16-byte vectors)", what, D);
    if (first < 0 || count < 1 || int64_t(first) + count > T)
        REFUSE(SFCVIT_EINVAL, "%s: tokens [%d, %d + %d) are not a non-empty range of the %d tokens", what, first, first, count, T);
    if (int64_t(T) * D > (INT64_MAX / 4) / B) REFUSE(SFCVIT_EINVAL, "%s: B=%d T=%d D=%d: the byte counts leave int64", what, B, T, D);
    p.dv = D / 8;
    // the column slab narrows (32 -> 16 -> 8 vectors) while B x slabs leaves the GPU short of workgroups: the lanes it
    // frees split the token range further
    p.cv = TP_MAX_CV;
    while (p.cv > TP_MIN_CV && ceil_div(p.dv, p.cv) * B < TP_MIN_WGS) p.cv /= 2;
    p.tl = TP_THREADS / p.cv;
    p.slabs = int(ceil_div(p.dv, p.cv));
    p.row_blocks = int(ceil_div(p.dv, TP_THREADS));
    if (p.slabs > 65535) REFUSE(SFCVIT_EINVAL, "%s: D=%d beyond the launch grid", what, D);
    p.row_copy = count == 1;
    return p;
}

int cls_prepend_check_fwd(const ClsPrependPlan &p, const void *x, const void *cls, const void *y, int B, int N, int D) {
    if (p.err) return fail(p.err, "%s", p.msg);
    if (!x || !cls || !y) return fail(SFCVIT_EINVAL, "cls_prepend_fwd: null pointer (x / cls / y)");
    if (!aligned16(x) || !aligned16(cls) || !aligned16(y)) return fail(SFCVIT_EINVAL, "cls_prepend_fwd: x, cls and y must be 16-byte aligned");
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y);
    const uint64_t xb = uint64_t(B) * N * D * 2, yb = uint64_t(B) * (uint64_t(N) + 1) * D * 2;
    if (x0 < y0 + yb && y0 < x0 + xb) return fail(SFCVIT_EINVAL, "cls_prepend_fwd: y overlaps x (the rows move: no in-place form)");
    return SFCVIT_OK;
}

int cls_prepend_check_bwd(const ClsPrependPlan &p, const void *dy, const void *dx, const void *dcls, const void *workspace,
                          int64_t workspace_bytes) {
    if (p.err) return fail(p.err, "%s", p.msg);
    if (!dy || !dcls) return fail(SFCVIT_EINVAL, "cls_prepend_bwd: null pointer (dy / dcls)");
    if (!aligned16(dy) || !aligned16(dx) || !aligned16(workspace))
        return fail(SFCVIT_EINVAL, "cls_prepend_bwd: dy, dx and the workspace must be 16-byte aligned");
    if (p.ws_bytes && (!workspace || workspace_bytes < p.ws_bytes))
        return fail(SFCVIT_EINVAL, "cls_prepend_bwd: workspace of %lld bytes needed", (long long)p.ws_bytes);
    return SFCVIT_OK;
}

int token_pool_check(const TokenPoolPlan &p, const char *what, const void *a, const void *b) {
    if (p.err) return fail(p.err, "%s", p.msg);
    if (!a || !b) return fail(SFCVIT_EINVAL, "%s: null pointer", what);
    if (!aligned16(a) || !aligned16(b)) return fail(SFCVIT_EINVAL, "%s: both tensors must be 16-byte aligned", what);
    return SFCVIT_OK;
}

}  // namespace sfcvit

extern "C" int64_t sfcvit_cls_prepend_bwd_workspace(int B, int N, int D) {
    const sfcvit::ClsPrependPlan p = sfcvit::cls_prepend_plan("cls_prepend_bwd_workspace", B, N, D);
    return p.err ? 0 : p.ws_bytes;
}

extern "C" int sfcvit_last_token_pool_kernel(char *buf, int n) { return sfcvit::g_token_pool.read(buf, n); }
