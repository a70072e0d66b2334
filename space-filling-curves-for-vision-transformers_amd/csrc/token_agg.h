// Depth-wise conv1d along the token sequence (include/sfcvit.h, "TokenAggregator"): the plan shared by the host checks
// (token_agg.cpp) and the kernels (token_agg.hip).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

constexpr int DWC_CV = 32;        // lanes across channels: a workgroup's D-slab is 32 x 8 = 256 channels
constexpr int DWC_RL = 8;         // lanes across rows: a workgroup walks 8 consecutive runs of one image
constexpr int DWC_THREADS = DWC_CV * DWC_RL;
constexpr int DWC_MAX_K = 9, DWC_MAX_S = 4;
constexpr int DWC_MAX_RUN = 32;   // rows a lane walks at most; longer sequences take more workgroups per image

struct DwconvPlan : PlanStatus {
    bool spec = false;            // k = 3, s = 1: the register-window kernels
    int pad = 0, Nout = 0;
    int slabs = 0;                // grid.x: ceil(D / 256)
    int groups = 0;               // grid.y: workgroups per image (grid.z = B)
    int run_out = 0, run_in = 0;  // rows per lane over the Nout output rows / the N input rows
    int ld = 0;                   // floats per partial row: D * k (dw, [d][t]) then D (db)
    int64_t ws_bytes = 0;         // B * groups partial rows
};

// Shape checks and launch geometry; no HIP call, no pointer is looked at.
DwconvPlan dwconv_plan(const char *what, int B, int N, int D, int k, int s);
// The pointer / workspace checks of the two entry points, after the plan: SFCVIT_OK or the refusal (message recorded).
int dwconv_check_fwd(const DwconvPlan &p, const void *x, const void *w, const void *u);
int dwconv_check_bwd(const DwconvPlan &p, const void *du, const void *x, const void *w, const void *dx, const void *dw, const void *db,
                     const void *workspace, int64_t workspace_bytes);
// Which kernel of this family the calling thread launched last (sfcvit_last_dwconv_kernel).
extern thread_local KernelNote g_dwconv;

}  // namespace sfcvit
