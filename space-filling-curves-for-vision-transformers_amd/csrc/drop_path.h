// Stochastic depth (DropPath) on the two residual sites of an encoder layer (include/sfcvit.h, "Stochastic depth"): the plans
// of sfcvit_add_layernorm_path_fwd and sfcvit_layernorm_bwd_path, shared by the host checks (drop_path.cpp) and the launchers
// in rowwise.hip.  Every refusal is decided here, before any HIP call; no pointer is dereferenced.
#pragma once
#include <cstdint>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

constexpr int DP_WAVES = 4;             // rows of a 256-lane workgroup of the forward kernel (one wave per row)
constexpr int DP_FWD_MAX_D = 4096;      // sfcvit_layernorm_fwd's limit: 8 vectors of 8 columns per lane
constexpr int DP_BWD_MAX_D = 2048;      // sfcvit_layernorm_bwd_drop's limit

struct AddLnPathPlan : PlanStatus {
    int M = 0;                          // B * N rows
    int vpl = 0;                        // 16-byte vectors per lane: 1, 2, 4 or 8 (D <= 512 * vpl)
    int blocks = 0;                     // ceil(M / 4)
};

struct LnBwdPathPlan : PlanStatus {
    int M = 0;                          // B * rows_per_image rows
};

AddLnPathPlan add_ln_path_plan(const void *branch, const void *x, const void *gamma, const void *beta, const void *s, const void *y,
                               const float *mean, const float *rstd, int B, int N, int D, float rate);
LnBwdPathPlan ln_bwd_path_plan(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma,
                               const void *dx_add, const void *dx, const void *dx_drop, float p, const void *dgamma,
                               const void *dbeta, int B, int rows_per_image, int D, const void *ws, float path_rate);

}  // namespace sfcvit
