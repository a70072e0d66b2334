// Host side of masked attention (attention_masked.h): mask validation with the block map, and the argument checks of the
// two entry points.  Plain host code: no HIP call, no allocation, so every refusal is testable on a machine without a GPU.
#include "attention_masked.h"

#include <cmath>

#include "common_host.h"

namespace sfcvit {

int attn_masked_check(const sfcvit_attn_mask_args *a, bool bwd, const char *what) {
    if (!a) return fail(SFCVIT_EINVAL, "%s: null pointer", what);
    if (!a->qkv || !a->out || !a->lse) return fail(SFCVIT_EINVAL, "%s: null pointer (qkv / out / lse)", what);
    if (bwd && (!a->dout || !a->dqkv || !a->delta)) return fail(SFCVIT_EINVAL, "%s: null pointer (dout / dqkv / delta)", what);
    if (!a->mask || !a->block_map) return fail(SFCVIT_EINVAL, "%s: null pointer (mask / block_map)", what);
    if (a->hd != 64) return fail(SFCVIT_EINVAL, "%s: head dim %d not supported: the masked kernels exist for head dim 64 only", what, a->hd);
    if (!(a->dropout_p >= 0.f && a->dropout_p < 1.f)) return fail(SFCVIT_EINVAL, "%s: dropout_p=%g out of [0, 1)", what, a->dropout_p);
    if (a->B <= 0 || a->H <= 0 || a->B > 65535 || a->H > 65535) return fail(SFCVIT_EINVAL, "%s: B=%d H=%d (1 .. 65535)", what, a->B, a->H);
    if (a->N < 1 || a->N > MASK_MAX_N) return fail(SFCVIT_EINVAL, "%s: N=%d out of 1 .. %d", what, a->N, MASK_MAX_N);
    if (!aligned16(a->qkv) || !aligned16(a->out) || (bwd && (!aligned16(a->dout) || !aligned16(a->dqkv))))
        return fail(SFCVIT_EINVAL, "%s: tensors must be 16-byte aligned", what);
    if (!aligned16(a->mask)) return fail(SFCVIT_EINVAL, "%s: mask must be 16-byte aligned", what);
    return SFCVIT_OK;
}

}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_attention_mask_blocks(const float *mask_host, int N, uint8_t *map_host) {
    if (!mask_host || !map_host) return fail(SFCVIT_EINVAL, "attention_mask_blocks: null pointer");
    if (N < 1 || N > MASK_MAX_N) return fail(SFCVIT_EINVAL, "attention_mask_blocks: N=%d out of 1 .. %d", N, MASK_MAX_N);
    const int nb = mask_blocks(N);
    // per block: bit 0 = a finite entry seen, bit 1 = an entry other than 0.0f seen (-0.0f counts as 0: it adds nothing)
    for (int i = 0; i < nb * nb; i++) map_host[i] = 0;
    for (int r = 0; r < N; r++) {
        const float *row = mask_host + size_t(r) * N;
        bool any = false;
        for (int c = 0; c < N; c++) {
            const float v = row[c];
            if (std::isnan(v)) return fail(SFCVIT_EINVAL, "attention_mask_blocks: NaN at row %d, column %d", r, c);
            if (std::isinf(v) && v > 0.f) return fail(SFCVIT_EINVAL, "attention_mask_blocks: +inf at row %d, column %d", r, c);
            uint8_t &m = map_host[(r / MASK_BLK) * nb + c / MASK_BLK];
            if (!std::isinf(v)) {
                any = true;
                m |= 1;
            }
            if (v != 0.f) m |= 2;
        }
        if (!any) return fail(SFCVIT_EINVAL, "attention_mask_blocks: row %d has no finite entry (every key hidden)", r);
    }
    for (int i = 0; i < nb * nb; i++) {
        const uint8_t m = map_host[i];
        map_host[i] = !(m & 1) ? MASK_SKIP : (m & 2) ? MASK_MIXED : MASK_ZERO;
    }
    return SFCVIT_OK;
}
