// The plans of the row-wise family (layernorm.hip, optim.hip, rowwise.hip) on the scaffold of plan.h: every refusal, which
// kernel form a shape gets, its grid, LDS and workspace.  Plain host C++ (rowwise.cpp): no HIP include, no getenv, no
// pointer dereferenced beyond the argument structs themselves; hostcheck/host_check.cpp (check_rowwise) pins them on the CPU.
// The stochastic-depth and EMA plans (drop_path.h, model_ema.h) are these plus their own refusals.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

constexpr int ROW_THREADS = 256;            // lanes of a workgroup of every kernel of the family (THREADS of the .hip files)
constexpr int ROW_WAVES = ROW_THREADS / 64; // rows of a workgroup of the one-wave-per-row kernels
constexpr int LN_FWD_MAX_D = 4096;          // LayerNorm forward: 8 vectors of 8 columns per lane
constexpr int LN_BWD_MAX_D = 2048;          // LayerNorm backward: 4

// Tuning switches, read once per process by read_rowwise_knobs (common.cpp; the table in dispatch.h).
struct RowwiseKnobs {
    int ln_cols = 1;                        // SFCVIT_LN_COLS: 0 = the 16-byte-vector LayerNorm backward also at D = 768 / 1 024
    int ln_blocks = 0;                      // SFCVIT_LN_BLOCKS: workgroups of the LayerNorm backward (0: the plan's caps)
    int ln_fwd_two_rows = 1;                // SFCVIT_LN_FWD_TWO_ROWS: 0 = one row per wave in the LayerNorm forward
    int adamw_nt = 3;                       // SFCVIT_ADAMW_NT: nontemporal loads (1) / stores (2) of the optimizer state
};
const RowwiseKnobs &read_rowwise_knobs();

// ---- LayerNorm ----
struct LnFwdPlan : PlanStatus {
    bool two_rows = false;                  // ln_fwd2_kernel<vpl> (vpl 3 | 4), else ln_fwd_kernel<vpl> (1 | 2 | 4 | 8)
    int vpl = 0;                            // 16-byte vectors per lane
    int blocks = 0;
};
// The one-row-per-wave form, which add_ln_path_kernel shares: D <= 512 * vpl, ceil(M / 4) workgroups.
void ln_fwd_rows(int M, int D, int &vpl, int &blocks);
LnFwdPlan ln_fwd_plan(const void *x, const void *gamma, const void *beta, const void *y, const float *mean, const float *rstd,
                      int M, int D, const RowwiseKnobs &k);

struct LnBwdPlan : PlanStatus {
    int M = 0, D = 0;
    bool cols = false, add = false;         // ln_bwd_cols[_path]_kernel<inst, add> (D = 256 inst), else ln_bwd[_path]_kernel<inst, add>
    int inst = 0;                           // CH (3 | 4) or VPL (1 | 2 | 4)
    int blocks = 0;
    size_t lds = 0;                         // dynamic LDS: [ROW_WAVES][3][D] fp32
    int64_t ws_bytes = 0;                   // the partials: [blocks][3][D] fp32
};
// Form and launch geometry alone, no refusal: sfcvit_layernorm_bwd_ws sizes the workspace from it before the pointers exist.
LnBwdPlan ln_bwd_geometry(int M, int D, bool add, const RowwiseKnobs &k);
LnBwdPlan ln_bwd_plan(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma, const void *dx_add,
                      const void *dx, const void *dx_drop, float p, const void *dgamma, const void *dbeta, int M, int D,
                      const void *ws, const RowwiseKnobs &k);
// "ln_bwd_cols_kernel<3, true>", with `path` "ln_bwd_cols_path_kernel<3, true>": what sfcvit_last_rowwise_kernel reports.
void kernel_name(const LnBwdPlan &p, bool path, char *buf, size_t n);

// ---- clip + AdamW ----
struct AdamwPlan : PlanStatus {
    int grid = 0;                           // one lane per 8 parameters, rounded up, 1 .. ADAMW_MAX_BLOCKS (model_ema.h)
    int nt = 0;                             // adamw[_ema]_kernel<nt>
};
AdamwPlan adamw_plan(const sfcvit_adamw_args *a, const RowwiseKnobs &k, const char *what = "adamw");
int optim_grid(int64_t n);                  // that grid for n >= 1 elements; sumsq_plan and grad_accum.cpp cap it further

// ---- column sums ----
struct ColsumPlan : PlanStatus {
    int col_blocks = 0, row_blocks = 0, rpb = 0;       // grid (x, y); rows per workgroup, a multiple of 8
    int64_t ws_bytes = 0;                              // [row_blocks][N] fp32 partial sums
};
ColsumPlan colsum_geometry(int M, int N);              // no refusal: sfcvit_colsum_workspace
ColsumPlan colsum_plan(const void *x, int M, int N, int ld, const void *out, const void *workspace, int64_t workspace_bytes);

// ---- the entry points whose plan is refusals + a grid ----
struct RowGridPlan : PlanStatus {
    int grid = 0, grid_y = 1;
};
// GELU and the dropout mask take their grid from grid_for in rowwise.hip, one lane per work item up to its cap: their plans
// are the refusals.  sumsq_plan's grid is the optimizer's (adamw_plan's formula), capped by the partials the workspace holds.
RowGridPlan transpose_plan(const void *src, int R, int C, int lds, const void *dst, int ldd);
RowGridPlan transpose_batched_plan(const void *src_base, const void *dst_base, const void *tiles, int n_tiles);
PlanStatus gelu_plan(bool bwd, const void *dy, const void *x, const void *out, int64_t n);
PlanStatus gelu_drop_plan(bool bwd, const void *dy, const void *x, const void *out, int rows, int cols, float p);
PlanStatus dropout_mask_plan(const void *out, int64_t rows, int cols, float p);
RowGridPlan soft_ce_plan(const void *logits, const float *targets, const float *loss_rows, int B, int C, int ld);
RowGridPlan sumsq_plan(const void *g, int64_t n, const float *out, const void *workspace);
RowGridPlan step_advance_plan(const void *state);

}  // namespace sfcvit
