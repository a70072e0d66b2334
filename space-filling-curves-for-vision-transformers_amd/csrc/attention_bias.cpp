// Host side of attention with a relative position bias (attention_bias.h): index validation with the block map and the
// inverted index, the workspace size, and the argument checks of the two entry points.  Plain host code: no HIP call,
// no allocation, so every refusal is testable on a machine without a GPU.
#include "attention_bias.h"

#include "common_host.h"

namespace sfcvit {

int attn_bias_check(const sfcvit_attn_bias_args *a, bool bwd, const char *what) {
    if (!a) return fail(SFCVIT_EINVAL, "%s: null pointer", what);
    if (!a->qkv || !a->out || !a->lse) return fail(SFCVIT_EINVAL, "%s: null pointer (qkv / out / lse)", what);
    if (bwd && (!a->dout || !a->dqkv || !a->delta)) return fail(SFCVIT_EINVAL, "%s: null pointer (dout / dqkv / delta)", what);
    if (!a->index || !a->table || !a->block_map) return fail(SFCVIT_EINVAL, "%s: null pointer (index / table / block_map)", what);
    const bool table_grad = bwd && a->dtable;             // dtable == NULL: a frozen table, its gradient is not computed
    if (table_grad && (!a->offsets || !a->positions)) return fail(SFCVIT_EINVAL, "%s: null pointer (offsets / positions)", what);
    if (a->hd != 64) return fail(SFCVIT_EINVAL, "%s: head dim %d not supported: the bias kernels exist for head dim 64 only", what, a->hd);
    if (!(a->dropout_p >= 0.f && a->dropout_p < 1.f)) return fail(SFCVIT_EINVAL, "%s: dropout_p=%g out of [0, 1)", what, a->dropout_p);
    if (a->B <= 0 || a->H <= 0 || a->B > 65535 || a->H > 65535) return fail(SFCVIT_EINVAL, "%s: B=%d H=%d (1 .. 65535)", what, a->B, a->H);
    if (a->N < 1 || a->N > RELB_MAX_N) return fail(SFCVIT_EINVAL, "%s: N=%d out of 1 .. %d", what, a->N, RELB_MAX_N);
    if (a->T < 1 || a->T > RELB_MAX_T) return fail(SFCVIT_EINVAL, "%s: T=%d out of 1 .. %d", what, a->T, RELB_MAX_T);
    if (!aligned16(a->qkv) || !aligned16(a->out) || (bwd && (!aligned16(a->dout) || !aligned16(a->dqkv))))
        return fail(SFCVIT_EINVAL, "%s: tensors must be 16-byte aligned", what);
    if (!aligned16(a->index)) return fail(SFCVIT_EINVAL, "%s: index must be 16-byte aligned", what);
    if (!table_grad) return SFCVIT_OK;
    const int nb = bias_blocks(a->N);
    if (a->visited_blocks < 1 || a->visited_blocks > nb * nb)
        return fail(SFCVIT_EINVAL, "%s: visited_blocks=%d out of 1 .. %d", what, a->visited_blocks, nb * nb);
    const int64_t need = sfcvit_attention_bias_workspace(a->B, a->N, a->H, a->visited_blocks);
    if (!a->workspace || !aligned16(a->workspace) || a->workspace_bytes < need)
        return fail(SFCVIT_EINVAL, "%s: workspace of %lld bytes, 16-byte aligned, needed (sfcvit_attention_bias_workspace), got %lld",
                    what, static_cast<long long>(need), static_cast<long long>(a->workspace ? a->workspace_bytes : 0));
    return SFCVIT_OK;
}

}  // namespace sfcvit

using namespace sfcvit;

extern "C" int64_t sfcvit_attention_bias_workspace(int B, int N, int H, int visited_blocks) {
    if (B < 1 || H < 1 || N < 1 || N > RELB_MAX_N || visited_blocks < 1) return 0;
    const BiasChunks c = bias_chunks(B, H, visited_blocks);
    return int64_t(c.chunks) * H * visited_blocks * RELB_BLK * RELB_BLK * int64_t(sizeof(float));
}

extern "C" int sfcvit_attention_bias_blocks(const int32_t *index_host, int N, int T, uint8_t *map_host, int32_t *offsets_host,
                                            int32_t *positions_host) {
    if (!index_host || !map_host || !offsets_host || !positions_host) return fail(SFCVIT_EINVAL, "attention_bias_blocks: null pointer");
    if (N < 1 || N > RELB_MAX_N) return fail(SFCVIT_EINVAL, "attention_bias_blocks: N=%d out of 1 .. %d", N, RELB_MAX_N);
    if (T < 1 || T > RELB_MAX_T) return fail(SFCVIT_EINVAL, "attention_bias_blocks: T=%d out of 1 .. %d", T, RELB_MAX_T);
    const int nb = bias_blocks(N);
    for (int i = 0; i < nb * nb; i++) map_host[i] = 0;
    // Counting sort by bucket.  The counts go two slots up, so that after the prefix sum offsets[t + 1] is the START of
    // bucket t; filling advances it to the bucket's end = the start of bucket t + 1, which is what offsets[t + 1] means.
    for (int t = 0; t <= T; t++) offsets_host[t] = 0;
    for (int r = 0; r < N; r++) {
        const int32_t *row = index_host + size_t(r) * N;
        bool any = false;
        for (int c = 0; c < N; c++) {
            const int32_t v = row[c];
            if (v < -1 || v >= T) return fail(SFCVIT_EINVAL, "attention_bias_blocks: entry %d at row %d, column %d is outside -1 .. %d", v, r, c, T - 1);
            if (v < 0) continue;
            any = true;
            map_host[(r / RELB_BLK) * nb + c / RELB_BLK] = 1;
            if (v + 2 <= T) offsets_host[v + 2]++;
        }
        if (!any) return fail(SFCVIT_EINVAL, "attention_bias_blocks: row %d has no visible entry (every key hidden)", r);
    }
    for (int t = 1; t <= T; t++) offsets_host[t] += offsets_host[t - 1];
    for (int r = 0; r < N; r++)
        for (int c = 0; c < N; c++) {
            const int32_t v = index_host[size_t(r) * N + c];
            if (v >= 0) positions_host[offsets_host[v + 1]++] = r * N + c;
        }
    return SFCVIT_OK;
}
