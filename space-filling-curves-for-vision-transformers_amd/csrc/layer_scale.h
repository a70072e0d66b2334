// LayerScale on the two residual sites of a pre-norm encoder layer (include/sfcvit.h, "LayerScale residual site"): the plans of
// sfcvit_add_layernorm_scale_fwd and sfcvit_layernorm_bwd_scale, shared by the host checks (layer_scale.cpp) and the launchers in
// layer_scale.hip: the LayerNorm geometry of rowwise.h plus the refusals of their own.  Every refusal is decided here, before
// any HIP call; no pointer is dereferenced.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"
#include "rowwise.h"

namespace sfcvit {

struct AddLnScalePlan : PlanStatus {
    int M = 0;                          // B * N rows
    int vpl = 0;                        // 16-byte vectors per lane: 1, 2, 4 or 8 (D <= 512 * vpl)
    int blocks = 0;                     // ceil(M / 4)
};

// ln_bwd_scale_kernel<inst, add> / ln_bwd_cols_scale_kernel<inst, add>: the form and the grid of ln_bwd_geometry, so dgamma / dbeta
// / dx keep the summation order of the LayerNorm backward of that width.  lds is the three-sum region [ROW_WAVES][3][D] (the fourth
// sum, dlam, goes through it in a second round); ws_bytes holds FOUR partial rows per workgroup: [blocks][4][D] fp32.
using LnBwdScalePlan = LnBwdPlan;

AddLnScalePlan add_ln_scale_plan(const void *branch, const void *x, const void *lam, const void *gamma, const void *beta,
                                 const void *s, const void *y, const float *mean, const float *rstd, int B, int N, int D, float rate);
// Form and launch geometry alone, no refusal: sfcvit_layernorm_bwd_scale_ws sizes the workspace from it.
LnBwdScalePlan ln_bwd_scale_geometry(int M, int D, bool add, const RowwiseKnobs &k);
LnBwdScalePlan ln_bwd_scale_plan(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma,
                                 const void *dx_add, const void *branch, const void *lam, const void *dx, const void *dx_drop,
                                 float p, const void *dgamma, const void *dbeta, const void *dlam, int B, int rows_per_image, int D,
                                 const void *ws, float path_rate, const RowwiseKnobs &k);
// "ln_bwd_scale_kernel<2, true>", "ln_bwd_cols_scale_kernel<3, false>": what sfcvit_last_rowwise_kernel reports.
void scale_kernel_name(const LnBwdScalePlan &p, char *buf, size_t n);

}  // namespace sfcvit
