// Argument checks and launch geometry of sfcvit_rope_fwd / sfcvit_rope_bwd (rope.h), on the scaffold of plan.h.
// Plain host code: no HIP call, no allocation, so every refusal is testable on a machine without a GPU.
#include "rope.h"

#include <climits>

namespace sfcvit {

RopePlan rope_geometry(int B, int N, int H, int hp, const char *what) {
    RopePlan p;
    if (B <= 0 || N <= 0 || H <= 0) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d H=%d (B, N, H >= 1)", what, B, N, H);
    if (hp != 64 && hp != 128 && hp != 192 && hp != 256)
        REFUSE(SFCVIT_EINVAL, "%s: hp=%d is not a kernel head dim (64, 128, 192, 256)", what, hp);
    if (int64_t(3) * H * hp > INT_MAX) REFUSE(SFCVIT_EINVAL, "%s: H=%d hp=%d: the row width 3 * H * hp leaves int", what, H, hp);
    if (int64_t(B) * N > INT_MAX) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d: the row count B * N leaves int", what, B, N);
    p.B = B;
    p.N = N;
    p.H = H;
    p.hp = hp;
    p.vpl = hp / 64;
    p.slot_groups = int(ceil_div(int64_t(2) * H, ROPE_SLOTS));
    p.token_blocks = int(ceil_div(N, ROPE_WAVES));
    p.batch_chunks = int(ceil_div(B, ROPE_BATCH_PER_WG));
    const int64_t blocks = int64_t(p.slot_groups) * p.token_blocks * p.batch_chunks;
    if (blocks > INT_MAX)
        REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d H=%d: the grid of %lld workgroups leaves int", what, B, N, H, (long long)blocks);
    p.blocks = int(blocks);
    p.part_ld = ROPE_SLOTS * hp;
    p.ws_bytes = blocks * p.part_ld * int64_t(sizeof(float));
    return p;
}

static bool bad_hd(int hd, int hp) { return hd < 2 || hd > hp || (hd & 1); }

RopePlan rope_fwd_plan(const void *qkv, const void *table, int B, int N, int H, int hd, int hp) {
    const char *what = "rope_fwd";
    RopePlan p;
    if (!qkv || !table) REFUSE(SFCVIT_EINVAL, "%s: null pointer (qkv / table)", what);
    p = rope_geometry(B, N, H, hp, what);
    if (p.err) return p;
    if (bad_hd(hd, hp)) REFUSE(SFCVIT_EINVAL, "%s: hd=%d (even, 2 <= hd <= hp = %d: channels rotate in pairs)", what, hd, hp);
    if (!aligned16(qkv) || !aligned16(table)) REFUSE(SFCVIT_EINVAL, "%s: qkv and table must be 16-byte aligned", what);
    p.hd = hd;
    return p;
}

RopePlan rope_bwd_plan(const void *dqkv, const void *table, const void *colsum, const void *vsum, const void *ws, int B, int N, int H,
                       int hd, int hp) {
    const char *what = "rope_bwd";
    RopePlan p;
    if (!dqkv || !table) REFUSE(SFCVIT_EINVAL, "%s: null pointer (dqkv / table)", what);
    if (colsum && !ws)
        REFUSE(SFCVIT_EINVAL, "%s: colsum without a workspace (null pointer): sfcvit_rope_bwd_ws(B, N, H, hp) bytes", what);
    if (vsum && !colsum) REFUSE(SFCVIT_EINVAL, "%s: vsum without colsum (null pointer): the v sums have nowhere to go", what);
    p = rope_geometry(B, N, H, hp, what);
    if (p.err) return p;
    if (bad_hd(hd, hp)) REFUSE(SFCVIT_EINVAL, "%s: hd=%d (even, 2 <= hd <= hp = %d: channels rotate in pairs)", what, hd, hp);
    if (!aligned16(dqkv) || !aligned16(table) || !aligned16(colsum) || !aligned16(vsum) || !aligned16(ws))
        REFUSE(SFCVIT_EINVAL, "%s: dqkv, table, colsum, vsum and ws must be 16-byte aligned", what);
    p.hd = hd;
    p.sums = colsum != nullptr;
    const int64_t Da = int64_t(H) * hp;
    p.reduce_blocks = p.sums ? int(2 * Da / 16) + (vsum ? int(ceil_div(Da, 1024)) : 0) : 0;
    return p;
}

}  // namespace sfcvit
