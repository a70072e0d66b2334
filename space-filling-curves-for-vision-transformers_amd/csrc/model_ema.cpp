// Argument checks of sfcvit_adamw_ema_step (model_ema.h): the plan of sfcvit_adamw_step (rowwise.cpp) plus the refusals of the
// weight average.  Plain host code: no HIP call, no allocation, so every refusal is testable on a machine without a GPU.
#include "model_ema.h"

#include <cstdint>

namespace sfcvit {

AdamwEmaPlan adamw_ema_plan(const sfcvit_adamw_args *a, const sfcvit_ema_args *e, const RowwiseKnobs &k) {
    const char *what = "adamw_ema";
    const AdamwEmaPlan step = adamw_plan(a, k, what);
    if (step.err) return step;
    AdamwEmaPlan p;                                                           // a refusal below carries no geometry
    if (!e) REFUSE(SFCVIT_EINVAL, "%s: null pointer (e)", what);
    if (!e->ema) REFUSE(SFCVIT_EINVAL, "%s: null pointer (ema)", what);
    if (a->n > INT64_MAX / 4) REFUSE(SFCVIT_EINVAL, "%s: n=%lld: n fp32 values leave the address space", what, (long long)a->n);
    if (!aligned16(e->ema)) REFUSE(SFCVIT_EINVAL, "%s: ema must be 16-byte aligned", what);
    if (!(e->decay >= 0.f && e->decay < 1.f)) REFUSE(SFCVIT_EINVAL, "%s: decay=%g outside [0, 1)", what, e->decay);
    // a lane stores its group of ema after other lanes may already have stored theirs of the other buffers
    const uint64_t b32 = uint64_t(a->n) * 4, b16 = uint64_t(a->n) * 2;
    const struct { const void *ptr; uint64_t bytes; const char *name; } others[] = {
        {a->param, b16, "param"}, {a->master, b32, "master"}, {a->grad, b16, "grad"}, {a->m, b32, "m"}, {a->v, b32, "v"}};
    for (const auto &o : others)
        if (overlap(e->ema, b32, o.ptr, o.bytes)) REFUSE(SFCVIT_EINVAL, "%s: ema overlaps %s", what, o.name);
    return step;
}

}  // namespace sfcvit
