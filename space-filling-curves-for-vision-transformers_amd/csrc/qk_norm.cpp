// Argument checks and launch geometry of sfcvit_qk_norm_fwd / sfcvit_qk_norm_bwd (qk_norm.h), on the scaffold of plan.h.
// Plain host code: no HIP call, no allocation, so every refusal is testable on a machine without a GPU.
#include "qk_norm.h"

#include <climits>
#include <cmath>

namespace sfcvit {

QkNormPlan qk_norm_geometry(int M, int H, int hp, const char *what) {
    QkNormPlan p;
    if (M <= 0 || H <= 0) REFUSE(SFCVIT_EINVAL, "%s: M=%d H=%d (M, H >= 1)", what, M, H);
    if (hp != 64 && hp != 128 && hp != 192 && hp != 256)
        REFUSE(SFCVIT_EINVAL, "%s: hp=%d is not a kernel head dim (64, 128, 192, 256)", what, hp);
    if (int64_t(3) * H * hp > INT_MAX) REFUSE(SFCVIT_EINVAL, "%s: H=%d hp=%d: the row width 3 * H * hp leaves int", what, H, hp);
    p.M = M;
    p.H = H;
    p.hp = hp;
    p.vpl = hp / 64;
    p.slot_groups = int(ceil_div(int64_t(2) * H, QK_SLOTS));
    p.rows_per_wg = QK_ROWS_PER_WG;
    p.chunks = int(ceil_div(M, QK_ROWS_PER_WG));
    const int64_t blocks = int64_t(p.slot_groups) * p.chunks;
    if (blocks > INT_MAX) REFUSE(SFCVIT_EINVAL, "%s: M=%d H=%d: the grid of %lld workgroups leaves int", what, M, H, (long long)blocks);
    p.blocks = int(blocks);
    p.part_ld = (QK_SLOTS + 4) * hp;
    p.ws_bytes = blocks * p.part_ld * int64_t(sizeof(float));
    return p;
}

static bool bad_eps(float eps) { return !(eps >= 0.f) || !std::isfinite(eps); }

QkNormPlan qk_norm_fwd_plan(const void *qkv, const void *raw, const void *params, int M, int H, int hd, int hp, float eps) {
    const char *what = "qk_norm_fwd";
    QkNormPlan p;
    if (!qkv || !raw || !params) REFUSE(SFCVIT_EINVAL, "%s: null pointer (qkv / raw / params)", what);
    p = qk_norm_geometry(M, H, hp, what);
    if (p.err) return p;
    if (hd < 1 || hd > hp) REFUSE(SFCVIT_EINVAL, "%s: hd=%d (1 <= hd <= hp = %d)", what, hd, hp);
    if (bad_eps(eps)) REFUSE(SFCVIT_EINVAL, "%s: eps=%g (finite, >= 0)", what, eps);
    if (!aligned16(qkv) || !aligned16(raw) || !aligned16(params))
        REFUSE(SFCVIT_EINVAL, "%s: qkv, raw and params must be 16-byte aligned", what);
    const uint64_t Da = uint64_t(H) * hp;
    if (overlap(qkv, uint64_t(M) * 3 * Da * 2, raw, uint64_t(M) * 2 * Da * 2))
        REFUSE(SFCVIT_EINVAL, "%s: raw overlaps qkv (raw keeps what the in-place pass replaces)", what);
    p.hd = hd;
    return p;
}

QkNormPlan qk_norm_bwd_plan(const void *dqkv, const void *raw, const void *params, const void *dparams, const void *colsum,
                            const void *vsum, const void *ws, int M, int H, int hd, int hp, float eps) {
    const char *what = "qk_norm_bwd";
    QkNormPlan p;
    if (!dqkv || !raw || !params || !dparams) REFUSE(SFCVIT_EINVAL, "%s: null pointer (dqkv / raw / params / dparams)", what);
    if (!ws) REFUSE(SFCVIT_EINVAL, "%s: the workspace is missing (null pointer): sfcvit_qk_norm_bwd_ws(M, H, hp) bytes", what);
    if (vsum && !colsum) REFUSE(SFCVIT_EINVAL, "%s: vsum without colsum (null pointer): the v sums have nowhere to go", what);
    p = qk_norm_geometry(M, H, hp, what);
    if (p.err) return p;
    if (hd < 1 || hd > hp) REFUSE(SFCVIT_EINVAL, "%s: hd=%d (1 <= hd <= hp = %d)", what, hd, hp);
    if (bad_eps(eps)) REFUSE(SFCVIT_EINVAL, "%s: eps=%g (finite, >= 0)", what, eps);
    if (!aligned16(dqkv) || !aligned16(raw) || !aligned16(params) || !aligned16(dparams) || !aligned16(colsum) || !aligned16(vsum) ||
        !aligned16(ws))
        REFUSE(SFCVIT_EINVAL, "%s: dqkv, raw, params, dparams, colsum, vsum and ws must be 16-byte aligned", what);
    const uint64_t Da = uint64_t(H) * hp;
    if (overlap(dqkv, uint64_t(M) * 3 * Da * 2, raw, uint64_t(M) * 2 * Da * 2))
        REFUSE(SFCVIT_EINVAL, "%s: raw overlaps dqkv", what);
    p.hd = hd;
    p.reduce_blocks = (colsum ? int(2 * Da / 16) : 0) + 4 * hp / 16 + (vsum ? int(ceil_div(int64_t(Da), 1024)) : 0);
    return p;
}

}  // namespace sfcvit
