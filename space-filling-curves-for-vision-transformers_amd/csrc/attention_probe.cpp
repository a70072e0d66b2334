// Argument checks and launch geometry of sfcvit_attention_probs / sfcvit_attention_stats (dispatch.h), on the scaffold of
// plan.h.  Plain host code: no HIP call, no allocation; checked on the CPU by hostcheck/host_check.cpp.
#include "dispatch.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

namespace sfcvit {

ProbePlan attn_probe_plan(const sfcvit_attn_probe_args &a, bool stats) {
    ProbePlan p;
    p.stats = stats;
    const char *what = stats ? "attention_stats" : "attention_probs";
    if (!a.qkv || !a.lse) REFUSE(SFCVIT_EINVAL, "%s: null pointer (qkv / lse)", what);
    if (a.hd != 64 && a.hd != 128 && a.hd != 192 && a.hd != 256)
        REFUSE(SFCVIT_EINVAL, "%s: head dim %d not supported (64, 128, 192, 256)", what, a.hd);
    if (a.B <= 0 || a.N <= 0 || a.H <= 0 || a.B > 65535 || a.H > 65535) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d H=%d", what, a.B, a.N, a.H);
    if (!std::isfinite(a.scale) || a.scale == 0.f) REFUSE(SFCVIT_EINVAL, "%s: scale=%g must be finite and nonzero", what, double(a.scale));
    if (!aligned16(a.qkv) || !aligned16(a.lse)) REFUSE(SFCVIT_EINVAL, "%s: tensors must be 16-byte aligned", what);
    p.inst = a.hd / ATTN_HD;
    p.blocks = (a.N + ATTN_BLK - 1) / ATTN_BLK;
    p.lds = size_t(p.inst) * ATTN_BLK * 128;
    if (stats) {
        if (!a.dist_rows && !a.seq_rows && !a.ent_rows && !a.mass_rows)
            REFUSE(SFCVIT_EINVAL, "%s: every output is NULL: nothing to compute", what);
        if (a.dist_rows && !a.pos) REFUSE(SFCVIT_EINVAL, "%s: dist_rows needs pos (the [N, 2] token centres)", what);
        if (!aligned16(a.pos) || !aligned16(a.dist_rows) || !aligned16(a.seq_rows) || !aligned16(a.ent_rows) || !aligned16(a.mass_rows))
            REFUSE(SFCVIT_EINVAL, "%s: tensors must be 16-byte aligned", what);
        p.grid_z = a.B;
        p.lds += PROBE_POS_BYTES;
        return p;
    }
    if (!a.probs) REFUSE(SFCVIT_EINVAL, "%s: null pointer (probs)", what);
    if (!aligned16(a.probs)) REFUSE(SFCVIT_EINVAL, "%s: tensors must be 16-byte aligned", what);
    if ((a.probs_is_bf16 != 0 && a.probs_is_bf16 != 1) || (a.head_mean != 0 && a.head_mean != 1))
        REFUSE(SFCVIT_EINVAL, "%s: probs_is_bf16=%d head_mean=%d must be 0 or 1", what, a.probs_is_bf16, a.head_mean);
    p.mean = a.head_mean != 0;
    if (p.blocks > 65535 || (!p.mean && int64_t(a.B) * a.H > 65535))
        REFUSE(SFCVIT_EINVAL, "%s: N=%d or B*H=%lld beyond the launch grid (65535 key blocks, 65535 maps)", what, a.N, (long long)(int64_t(a.B) * a.H));
    p.grid_z = p.mean ? a.B : a.B * a.H;
    return p;
}

void kernel_name(const ProbePlan &p, char *buf, size_t n) {
    if (p.stats) snprintf(buf, n, "attn_probe_stats_kernel<%d>", p.inst);
    else snprintf(buf, n, "attn_probe_map_kernel<%d, %s>", p.inst, p.mean ? "true" : "false");
}

}  // namespace sfcvit
