// Argument checks and launch geometry of sfcvit_adamw_ema_step (model_ema.h), on the scaffold of plan.h.  Plain host code:
// no HIP call, no allocation, so every refusal is testable on a machine without a GPU.
#include "model_ema.h"

#include <cstdint>

namespace sfcvit {

namespace {
// [a, a + a_bytes) and [b, b + b_bytes) share a byte
bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
}  // namespace

AdamwEmaPlan adamw_ema_plan(const sfcvit_adamw_args *a, const sfcvit_ema_args *e) {
    AdamwEmaPlan p;
    const char *what = "adamw_ema";
    if (!a) REFUSE(SFCVIT_EINVAL, "%s: null pointer (a)", what);
    if (!e) REFUSE(SFCVIT_EINVAL, "%s: null pointer (e)", what);
    if (!a->param || !a->master || !a->grad || !a->m || !a->v)
        REFUSE(SFCVIT_EINVAL, "%s: null pointer (param / master / grad / m / v)", what);
    if (!e->ema) REFUSE(SFCVIT_EINVAL, "%s: null pointer (ema)", what);
    if (a->n <= 0 || (a->step < 1 && !a->dev_state)) REFUSE(SFCVIT_EINVAL, "%s: n=%lld step=%d", what, (long long)a->n, a->step);
    if (a->n > INT64_MAX / 4) REFUSE(SFCVIT_EINVAL, "%s: n=%lld: n fp32 values leave the address space", what, (long long)a->n);
    if (!aligned16(a->param) || !aligned16(a->master) || !aligned16(a->grad) || !aligned16(a->m) || !aligned16(a->v))
        REFUSE(SFCVIT_EINVAL, "%s: buffers must be 16-byte aligned", what);
    if (!aligned16(e->ema)) REFUSE(SFCVIT_EINVAL, "%s: ema must be 16-byte aligned", what);
    if (!(e->decay >= 0.f && e->decay < 1.f)) REFUSE(SFCVIT_EINVAL, "%s: decay=%g outside [0, 1)", what, e->decay);
    // a lane stores its group of ema after other lanes may already have stored theirs of the other buffers
    const uint64_t b32 = uint64_t(a->n) * 4, b16 = uint64_t(a->n) * 2;
    const struct { const void *ptr; uint64_t bytes; const char *name; } others[] = {
        {a->param, b16, "param"}, {a->master, b32, "master"}, {a->grad, b16, "grad"}, {a->m, b32, "m"}, {a->v, b32, "v"}};
    for (const auto &o : others)
        if (overlap(e->ema, b32, o.ptr, o.bytes)) REFUSE(SFCVIT_EINVAL, "%s: ema overlaps %s", what, o.name);
    const int64_t blocks = ceil_div(ceil_div(a->n, 8), ADAMW_THREADS);       // a->n >= 1: at least one
    p.grid = int(blocks > ADAMW_MAX_BLOCKS ? ADAMW_MAX_BLOCKS : blocks);
    return p;
}

}  // namespace sfcvit
