// Gradient accumulation next to the optimizer (include/sfcvit.h, "Gradient accumulation"): the plans of sfcvit_grad_accum and
// sfcvit_grad_accum_finish, shared by the host checks (grad_accum.cpp) and the launchers in optim.hip.  Every refusal is
// decided here, before any HIP call; no pointer is dereferenced.
#pragma once
#include <cstdint>

#include "../../include/sfcvit.h"
#include "model_ema.h"

namespace sfcvit {

struct GradAccumPlan : PlanStatus {
    int grid = 0;                           // adamw_plan's formula and cap; with sumsq also capped by the partials the workspace holds
    int nt = 0;                             // grad_accum[_finish]_kernel<.., nt>: SFCVIT_ADAMW_NT, as adamw_plan reads it
};

// Refused: a null grad or acc, n <= 0 (or n fp32 values that leave the address space), a grad or acc that is not 16-byte
// aligned, an acc that shares a byte with grad.
GradAccumPlan grad_accum_plan(const void *grad, const float *acc, int64_t n, const RowwiseKnobs &k, const char *what = "grad_accum");

// grad_accum_plan plus: a scale that is not finite or <= 0, a sumsq without a workspace, a sumsq or workspace that is not
// 4-byte aligned or shares a byte with grad or acc.
GradAccumPlan grad_accum_finish_plan(const void *grad, const float *acc, int64_t n, float scale, const float *sumsq, const void *workspace,
                                     const RowwiseKnobs &k);

}  // namespace sfcvit
