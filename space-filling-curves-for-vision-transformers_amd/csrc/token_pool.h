// CLS token and pooled read-outs of a [B, N, D] bf16 activation (include/sfcvit.h, "CLS token and token pooling"): the plans
// shared by the host checks (token_pool.cpp) and the kernels (token_pool.hip).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

constexpr int TP_THREADS = 256;
constexpr int CP_MAX_IMGS = 8;      // prepend copies: images a lane moves its vector of (1, 2, 4 or 8 independent 16-byte loads in flight)
constexpr int CP_CV = 8;            // dcls: lanes across columns, a workgroup's slab is 8 x 8 = 64 columns of the CLS row
constexpr int CP_RL = 32;           // dcls: lanes across images; lane rl sums images rl, rl + 32, ... of its workgroup's range
constexpr int CP_MAX_ROWS = 2048;   // dcls: images of one range (64 per lane) before the batch is split into ranges
constexpr int TP_MAX_CV = 32;       // pool: lanes across columns, 32, 16 or 8; the other 256 / cv lanes split the token range
constexpr int TP_MIN_CV = 8;
constexpr int TP_MIN_WGS = 1024;    // pool: four workgroups per CU of the MI355X before the column slab stops narrowing

struct ClsPrependPlan : PlanStatus {
    int dv = 0;                     // D / 8: 16-byte vectors of a token row
    int64_t xv = 0;                 // N * D / 8: vectors of an image of x (y has xv + dv)
    // copies: grid.x blocks of 256 lanes over the vectors of one image, grid.y groups of `imgs` consecutive images
    int fwd_blocks = 0, bwd_blocks = 0, groups = 0, imgs = 0;
    // dcls: `slabs` 64-column slabs x `splits` ranges of `rows` images (a multiple of 32)
    int slabs = 0, splits = 0, rows = 0;
    int64_t ws_bytes = 0;           // splits > 1 (B > 2048): [splits][D] fp32 partial sums; one range writes dcls itself
};

struct TokenPoolPlan : PlanStatus {
    int dv = 0;                     // D / 8
    int cv = 0, tl = 0;             // a workgroup is cv column lanes x tl token lanes, cv * tl = 256
    int slabs = 0;                  // grid (B, slabs); the count == 1 forward copy: grid (B, row_blocks), a lane per vector
    int row_blocks = 0;
    bool row_copy = false;          // count == 1: the read-out of one token moves bits
};

// Shape checks and launch geometry; no HIP call, no pointer is looked at.
ClsPrependPlan cls_prepend_plan(const char *what, int B, int N, int D);
TokenPoolPlan token_pool_plan(const char *what, int B, int T, int D, int first, int count);
// The pointer / workspace checks of the entry points, after the plan: SFCVIT_OK or the refusal (message recorded).
int cls_prepend_check_fwd(const ClsPrependPlan &p, const void *x, const void *cls, const void *y, int B, int N, int D);
int cls_prepend_check_bwd(const ClsPrependPlan &p, const void *dy, const void *dx, const void *dcls, const void *workspace,
                          int64_t workspace_bytes);
int token_pool_check(const TokenPoolPlan &p, const char *what, const void *a, const void *b);
// Which kernel of this family the calling thread launched last (sfcvit_last_token_pool_kernel).
extern thread_local KernelNote g_token_pool;

}  // namespace sfcvit
