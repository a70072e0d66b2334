// Token-axis GEMMs of the MixerBlock token-mix branch (include/sfcvit.h, "Token mixing"): the plans shared by the host
// checks (token_mix.cpp) and the kernels (token_mix.hip).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

constexpr int TMX_TILE = 128;          // output tile (gemm_core: 128 x 128 x 64)
constexpr int TMX_SLOTS = 512;         // workgroup slots of the device: 256 CUs x 2 (what the range count of wgrad aims at)
constexpr int TMX_MAX_RANGES = 64;

struct TokmixPlan : PlanStatus {
    int tiles_m = 0, tiles_n = 0;      // left: M x D tiles of one image;  wgrad: M x K tiles of dW
    int grid = 0;                      // left: tiles * B;  wgrad: tiles * ranges
    int wunit = 1;                     // left: elements per load of the weight loader (8, 4, 2 or 1)
    int ranges = 0, per_range = 0;     // wgrad: image ranges and images per range
    int ld = 0;                        // wgrad: floats per partial row: M * K (dW) then M (db)
    int64_t ws_bytes = 0;
};

// Shape checks and launch geometry; no HIP call, no pointer is dereferenced.
TokmixPlan tokmix_left_plan(const sfcvit_tokmix_args *a);
TokmixPlan tokmix_wgrad_plan(const char *what, int B, int M, int K, int D);
// The pointer / workspace checks of sfcvit_tokmix_wgrad, after the plan: SFCVIT_OK or the refusal (message recorded).
int tokmix_check_wgrad(const TokmixPlan &p, const void *g, const void *x, const void *dw, const void *db, const void *workspace,
                       int64_t workspace_bytes);
// Which kernel of this family the calling thread launched last (sfcvit_last_tokmix_kernel).
extern thread_local KernelNote g_tokmix;

}  // namespace sfcvit
