// Argument checks and grids of sfcvit_grad_accum / sfcvit_grad_accum_finish (grad_accum.h).  Plain host code: no HIP call, no
// allocation, so every refusal is testable on a machine without a GPU.
#include "grad_accum.h"

#include <cmath>
#include <cstdint>

namespace sfcvit {

GradAccumPlan grad_accum_plan(const void *grad, const float *acc, int64_t n, const RowwiseKnobs &k, const char *what) {
    GradAccumPlan p;
    if (!grad) REFUSE(SFCVIT_EINVAL, "%s: null pointer (grad)", what);
    if (!acc) REFUSE(SFCVIT_EINVAL, "%s: null pointer (acc)", what);
    if (n <= 0) REFUSE(SFCVIT_EINVAL, "%s: n=%lld", what, (long long)n);
    if (n > INT64_MAX / 4) REFUSE(SFCVIT_EINVAL, "%s: n=%lld: n fp32 values leave the address space", what, (long long)n);
    if (!aligned16(grad)) REFUSE(SFCVIT_EINVAL, "%s: grad must be 16-byte aligned", what);
    if (!aligned16(acc)) REFUSE(SFCVIT_EINVAL, "%s: acc must be 16-byte aligned", what);
    // a lane reads its group of grad after other lanes may already have stored theirs of acc (and the other way round in finish)
    if (overlap(acc, uint64_t(n) * 4, grad, uint64_t(n) * 2)) REFUSE(SFCVIT_EINVAL, "%s: acc overlaps grad", what);
    p.grid = optim_grid(n);
    p.nt = k.adamw_nt & 3;
    return p;
}

GradAccumPlan grad_accum_finish_plan(const void *grad, const float *acc, int64_t n, float scale, const float *sumsq, const void *workspace,
                                     const RowwiseKnobs &k) {
    const char *what = "grad_accum_finish";
    const GradAccumPlan base = grad_accum_plan(grad, acc, n, k, what);
    if (base.err) return base;
    GradAccumPlan p;                                                          // a refusal below carries no geometry
    if (!std::isfinite(scale) || !(scale > 0.f)) REFUSE(SFCVIT_EINVAL, "%s: scale=%g must be finite and > 0", what, scale);
    if (!sumsq) return base;                                                  // no sum of squares: the workspace is not looked at
    if (!workspace) REFUSE(SFCVIT_EINVAL, "%s: sumsq without workspace (SFCVIT_SUMSQ_WORKSPACE_BYTES)", what);
    if (!aligned(sumsq, 4)) REFUSE(SFCVIT_EINVAL, "%s: sumsq must be 4-byte aligned", what);
    if (!aligned(workspace, 4)) REFUSE(SFCVIT_EINVAL, "%s: workspace must be 4-byte aligned", what);
    const struct { const void *ptr; uint64_t bytes; const char *name; } outs[] = {{sumsq, 4, "sumsq"}, {workspace, SFCVIT_SUMSQ_WORKSPACE_BYTES, "workspace"}},
                                                                        bufs[] = {{grad, uint64_t(n) * 2, "grad"}, {acc, uint64_t(n) * 4, "acc"}};
    for (const auto &o : outs)
        for (const auto &b : bufs)
            if (overlap(o.ptr, o.bytes, b.ptr, b.bytes)) REFUSE(SFCVIT_EINVAL, "%s: %s overlaps %s", what, o.name, b.name);
    p = base;
    const int max_parts = SFCVIT_SUMSQ_WORKSPACE_BYTES / int(sizeof(float));      // one partial per workgroup, as sumsq_plan
    if (p.grid > max_parts) p.grid = max_parts;
    return p;
}

}  // namespace sfcvit
