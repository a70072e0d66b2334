// Stochastic depth (DropPath) on the two residual sites of an encoder layer (include/sfcvit.h, "Stochastic depth"): the plans
// of sfcvit_add_layernorm_path_fwd and sfcvit_layernorm_bwd_path, shared by the host checks (drop_path.cpp) and the launchers
// in layernorm.hip: the LayerNorm geometry of rowwise.h plus the refusals of their own.  Every refusal is decided here, before
// any HIP call; no pointer is dereferenced.
#pragma once
#include <cstdint>

#include "../../include/sfcvit.h"
#include "rowwise.h"

namespace sfcvit {

struct AddLnPathPlan : PlanStatus {
    int M = 0;                          // B * N rows
    int vpl = 0;                        // 16-byte vectors per lane: 1, 2, 4 or 8 (D <= 512 * vpl)
    int blocks = 0;                     // ceil(M / 4)
};

using LnBwdPathPlan = LnBwdPlan;        // M = B * rows_per_image rows, D: the geometry of sfcvit_layernorm_bwd_drop's plan

AddLnPathPlan add_ln_path_plan(const void *branch, const void *x, const void *gamma, const void *beta, const void *s, const void *y,
                               const float *mean, const float *rstd, int B, int N, int D, float rate);
LnBwdPathPlan ln_bwd_path_plan(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma,
                               const void *dx_add, const void *dx, const void *dx_drop, float p, const void *dgamma,
                               const void *dbeta, int B, int rows_per_image, int D, const void *ws, float path_rate,
                               const RowwiseKnobs &k);

}  // namespace sfcvit
