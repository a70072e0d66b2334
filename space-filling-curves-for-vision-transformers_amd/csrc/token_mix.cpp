// Argument checks and launch geometry of sfcvit_tokmix_left / _wgrad (token_mix.h), on the scaffold of plan.h.  Plain host
// code: no HIP call, no allocation, so every refusal is testable on a machine without a GPU.
#include "token_mix.h"

#include "common_host.h"

namespace sfcvit {

thread_local KernelNote g_tokmix;

namespace {

// The envelope both entry points share; what = the entry's name.
bool shape_ok(TokmixPlan &p, const char *what, int B, int M, int K, int D) {
    if (B <= 0 || M <= 0 || K <= 0) {
        refuse(p, SFCVIT_EINVAL, "%s: B=%d M=%d K=%d (every extent must be >= 1)", what, B, M, K);
        return false;
    }
    if (D <= 0 || D % 8) {
        refuse(p, SFCVIT_EINVAL, "%s: D=%d must be a positive multiple of 8", what, D);
        return false;
    }
    if (M % 8 && K % 8) {
        refuse(p, SFCVIT_EINVAL, "%s: M=%d K=%d: the hidden width (one of the two) must be a multiple of 8", what, M, K);
        return false;
    }
    if (int64_t(M) * K + M > INT32_MAX || int64_t(M) * D > INT32_MAX || int64_t(K) * D > INT32_MAX) {
        refuse(p, SFCVIT_EINVAL, "%s: M=%d K=%d D=%d too large", what, M, K, D);
        return false;
    }
    return true;
}

}  // namespace

TokmixPlan tokmix_left_plan(const sfcvit_tokmix_args *a) {
    TokmixPlan p;
    if (!a) REFUSE(SFCVIT_EINVAL, "tokmix_left: null argument block");
    if (!shape_ok(p, "tokmix_left", a->B, a->M, a->K, a->D)) return p;
    if (a->act != SFCVIT_ACT_NONE && a->act != SFCVIT_ACT_GELU) REFUSE(SFCVIT_EINVAL, "tokmix_left: act=%d (NONE or GELU)", a->act);
    if (!a->w || !a->x || !a->c) REFUSE(SFCVIT_EINVAL, "tokmix_left: null pointer (w / x / c)");
    if (!aligned16(a->x) || !aligned16(a->c) || !aligned16(a->residual) || !aligned16(a->aux_in) || !aligned16(a->aux_out))
        REFUSE(SFCVIT_EINVAL, "tokmix_left: x, c, residual, aux_in and aux_out must be 16-byte aligned");
    if (!aligned(a->w, 2) || !aligned(a->bias, 2)) REFUSE(SFCVIT_EINVAL, "tokmix_left: w and bias must be 2-byte aligned");
    p.tiles_m = int(ceil_div(a->M, TMX_TILE));
    p.tiles_n = int(ceil_div(a->D, TMX_TILE));
    const int64_t grid = int64_t(p.tiles_m) * p.tiles_n * a->B;
    if (grid > INT32_MAX) REFUSE(SFCVIT_EINVAL, "tokmix_left: B=%d M=%d D=%d beyond the launch grid", a->B, a->M, a->D);
    p.grid = int(grid);
    // the weight is dense: its row pitch is the contiguous extent.  Widest load that both the pitch and the pointer allow.
    const int pitch = a->w_transposed ? a->M : a->K;
    p.wunit = 1;
    for (int u = 8; u > 1; u >>= 1)
        if (pitch % u == 0 && aligned(a->w, 2 * u)) {
            p.wunit = u;
            break;
        }
    return p;
}

TokmixPlan tokmix_wgrad_plan(const char *what, int B, int M, int K, int D) {
    TokmixPlan p;
    if (!shape_ok(p, what, B, M, K, D)) return p;
    p.tiles_m = int(ceil_div(M, TMX_TILE));
    p.tiles_n = int(ceil_div(K, TMX_TILE));
    const int tiles = p.tiles_m * p.tiles_n;
    int want = TMX_SLOTS / tiles;                      // ranges that fill the device once
    if (want < 1) want = 1;
    if (want > TMX_MAX_RANGES) want = TMX_MAX_RANGES;
    p.per_range = int(ceil_div(B, want));
    p.ranges = int(ceil_div(B, p.per_range));
    const int64_t grid = int64_t(tiles) * p.ranges;
    if (grid > INT32_MAX) REFUSE(SFCVIT_EINVAL, "%s: M=%d K=%d beyond the launch grid", what, M, K);
    p.grid = int(grid);
    p.ld = M * K + M;
    p.ws_bytes = int64_t(p.ranges) * p.ld * int64_t(sizeof(float));
    return p;
}

int tokmix_check_wgrad(const TokmixPlan &p, const void *g, const void *x, const void *dw, const void *db, const void *workspace,
                       int64_t workspace_bytes) {
    if (p.err) return fail(p.err, "%s", p.msg);
    if (!g) return fail(SFCVIT_EINVAL, "tokmix_wgrad: null pointer (g)");
    if (!dw && !db) return fail(SFCVIT_EINVAL, "tokmix_wgrad: both outputs are NULL: nothing to compute");
    if (dw && !x) return fail(SFCVIT_EINVAL, "tokmix_wgrad: null pointer (x, needed for dw)");
    if (!aligned16(g) || !aligned16(x) || !aligned16(workspace))
        return fail(SFCVIT_EINVAL, "tokmix_wgrad: g, x and the workspace must be 16-byte aligned");
    if (!workspace || workspace_bytes < p.ws_bytes)
        return fail(SFCVIT_EINVAL, "tokmix_wgrad: workspace of %lld bytes needed", (long long)p.ws_bytes);
    return SFCVIT_OK;
}

}  // namespace sfcvit

extern "C" int64_t sfcvit_tokmix_wgrad_workspace(int B, int M, int K, int D) {
    const sfcvit::TokmixPlan p = sfcvit::tokmix_wgrad_plan("tokmix_wgrad_workspace", B, M, K, D);
    return p.err ? 0 : p.ws_bytes;
}

extern "C" int sfcvit_last_tokmix_kernel(char *buf, int n) { return sfcvit::g_tokmix.read(buf, n); }
