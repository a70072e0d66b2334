// Argument checks and launch geometry of sfcvit_pos_embed_fwd / _bwd (pos_embed.h), on the scaffold of plan.h.  Plain host
// code: no HIP call, no allocation, so every refusal is testable on a machine without a GPU.
#include "pos_embed.h"

#include "common_host.h"

namespace sfcvit {

thread_local KernelNote g_pos_embed;

PosEmbedPlan pos_embed_plan(const char *what, int B, int N, int D) {
    PosEmbedPlan p;
    if (B <= 0 || N <= 0) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d (B, N >= 1)", what, B, N);
    if (D < 8 || D % 8) REFUSE(SFCVIT_EINVAL, "%s: D=%d must be a positive multiple of 8 (16-byte vectors)", what, D);
    const int64_t nd = int64_t(N) * D;                          // < 2^62
    if (nd > (INT64_MAX / 4) / B) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d D=%d: the byte counts leave int64", what, B, N, D);
    p.vecs = nd / 8;
    const int64_t fwd_blocks = ceil_div(p.vecs, PE_THREADS), slabs = ceil_div(p.vecs, PE_CV);
    if (slabs > INT32_MAX) REFUSE(SFCVIT_EINVAL, "%s: N=%d D=%d beyond the launch grid", what, N, D);
    p.fwd_blocks = int(fwd_blocks);
    p.slabs = int(slabs);
    // forward: as many images per lane as still leave ~1024 workgroups, at most PE_MAX_IMGS
    int64_t imgs = fwd_blocks * B / 1024;
    p.imgs = imgs < 1 ? 1 : imgs > PE_MAX_IMGS ? PE_MAX_IMGS : int(imgs);
    const int64_t groups = ceil_div(B, p.imgs);
    if (groups > 65535) REFUSE(SFCVIT_EINVAL, "%s: B=%d beyond the launch grid", what, B);
    p.fwd_groups = int(groups);
    // backward: the batch is split only where the table alone gives too few workgroups and a lane keeps >= 4 images
    const int64_t want = ceil_div(PE_MIN_WGS, slabs), most = B / (PE_RL * 4) > 1 ? B / (PE_RL * 4) : 1;
    const int64_t splits = want < most ? want : most;
    p.rows = int(ceil_div(ceil_div(B, splits), PE_RL) * PE_RL);
    p.splits = int(ceil_div(B, p.rows));
    p.ws_bytes = p.splits > 1 ? int64_t(p.splits) * nd * int64_t(sizeof(float)) : 0;
    return p;
}

int pos_embed_check_fwd(const PosEmbedPlan &p, const void *x, const void *pos, const void *y) {
    if (p.err) return fail(p.err, "%s", p.msg);
    if (!x || !pos || !y) return fail(SFCVIT_EINVAL, "pos_embed_fwd: null pointer (x / pos / y)");
    if (!aligned16(x) || !aligned16(pos) || !aligned16(y)) return fail(SFCVIT_EINVAL, "pos_embed_fwd: x, pos and y must be 16-byte aligned");
    return SFCVIT_OK;
}

int pos_embed_check_bwd(const PosEmbedPlan &p, const void *dy, const void *dpos, const void *workspace, int64_t workspace_bytes) {
    if (p.err) return fail(p.err, "%s", p.msg);
    if (!dy || !dpos) return fail(SFCVIT_EINVAL, "pos_embed_bwd: null pointer (dy / dpos)");
    if (!aligned16(dy) || !aligned16(workspace)) return fail(SFCVIT_EINVAL, "pos_embed_bwd: dy and the workspace must be 16-byte aligned");
    if (p.ws_bytes && (!workspace || workspace_bytes < p.ws_bytes))
        return fail(SFCVIT_EINVAL, "pos_embed_bwd: workspace of %lld bytes needed", (long long)p.ws_bytes);
    return SFCVIT_OK;
}

}  // namespace sfcvit

extern "C" int64_t sfcvit_pos_embed_bwd_workspace(int B, int N, int D) {
    const sfcvit::PosEmbedPlan p = sfcvit::pos_embed_plan("pos_embed_bwd_workspace", B, N, D);
    return p.err ? 0 : p.ws_bytes;
}

extern "C" int sfcvit_last_pos_embed_kernel(char *buf, int n) { return sfcvit::g_pos_embed.read(buf, n); }
