// QK-norm (include/sfcvit.h, "QK-norm"): a LayerNorm over the head dim on the queries and keys of a packed projection, in place.
// The plans of sfcvit_qk_norm_fwd / sfcvit_qk_norm_bwd, shared by the host checks (qk_norm.cpp) and the launchers in
// qk_norm.hip.  Every refusal is decided here, before any HIP call; no pointer is dereferenced.
//
// Geometry (both directions): a group of 8 lanes owns one head row (hp / 64 16-byte vectors per lane); a wave owns the 8
// consecutive head slots j = 8 * slot_group + (lane >> 3) of the 2 H slots (q heads, then k heads) of a row of the buffer and
// walks tokens; a workgroup of QK_WAVES waves owns one slot group and QK_ROWS_PER_WG consecutive tokens, wave w taking every
// QK_WAVES-th of them.  The grid is slot_groups * chunks: a function of the shape alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

constexpr int QK_THREADS = 256, QK_WAVES = 4, QK_SLOTS = 8, QK_ROWS_PER_WG = 64;

struct QkNormPlan : PlanStatus {
    int M = 0, H = 0, hd = 0, hp = 0;
    int vpl = 0;                        // 16-byte vectors per lane: hp / 64
    int slot_groups = 0;                // ceil(2 H / 8)
    int rows_per_wg = 0;                // QK_ROWS_PER_WG
    int chunks = 0;                     // ceil(M / rows_per_wg)
    int blocks = 0;                     // slot_groups * chunks, workgroup = slot_group * chunks + chunk
    int part_ld = 0;                    // floats per workgroup in the backward's workspace: 8 hp column sums | 4 hp parameter sums
    int64_t ws_bytes = 0;               // blocks * part_ld * 4
    int reduce_blocks = 0;              // second stage: 16 columns per block, then 1024 copied v sums per block
};

// Launch geometry alone (err set only where the shape itself has none): sfcvit_qk_norm_bwd_ws and sfcvit_qk_norm_plan read it.
QkNormPlan qk_norm_geometry(int M, int H, int hp, const char *what);
QkNormPlan qk_norm_fwd_plan(const void *qkv, const void *raw, const void *params, int M, int H, int hd, int hp, float eps);
// colsum, vsum: optional.  vsum (fp32 [H * hp], the v third's column sums of the attention backward) needs colsum, which is then
// [3 H hp] and receives them in its last third.
QkNormPlan qk_norm_bwd_plan(const void *dqkv, const void *raw, const void *params, const void *dparams, const void *colsum,
                            const void *vsum, const void *ws, int M, int H, int hd, int hp, float eps);

}  // namespace sfcvit
