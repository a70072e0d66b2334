// Positional embedding added to a [B, N, D] bf16 activation (include/sfcvit.h, "Positional embedding"): the plan shared by
// the host checks (pos_embed.cpp) and the kernels (pos_embed.hip).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

constexpr int PE_THREADS = 256;
constexpr int PE_MAX_IMGS = 8;      // forward: images a lane adds its table vector to (8 independent 16-byte loads in flight)
constexpr int PE_CV = 32;           // backward: lanes across columns, a workgroup's slab is 32 x 8 = 256 columns of the [N D] table
constexpr int PE_RL = 8;            // backward: lanes across images; lane rl sums images rl, rl + 8, ... of its workgroup's range
constexpr int PE_MIN_WGS = 512;     // two workgroups per CU of the MI355X before the batch is left whole

struct PosEmbedPlan : PlanStatus {
    int64_t vecs = 0;               // N * D / 8: 16-byte vectors of the table
    // forward: grid (fwd_blocks, fwd_groups); a lane owns one table vector and `imgs` consecutive images
    int fwd_blocks = 0, fwd_groups = 0, imgs = 0;
    // backward: grid (slabs, splits); a workgroup sums `rows` images (a multiple of 8) of its 256-column slab
    int slabs = 0, splits = 0, rows = 0;
    int64_t ws_bytes = 0;           // splits > 1: [splits][N * D] fp32 partial sums; one split writes dpos itself
};

// Shape checks and launch geometry; no HIP call, no pointer is looked at.
PosEmbedPlan pos_embed_plan(const char *what, int B, int N, int D);
// The pointer / workspace checks of the two entry points, after the plan: SFCVIT_OK or the refusal (message recorded).
int pos_embed_check_fwd(const PosEmbedPlan &p, const void *x, const void *pos, const void *y);
int pos_embed_check_bwd(const PosEmbedPlan &p, const void *dy, const void *dpos, const void *workspace, int64_t workspace_bytes);
// Which kernel of this family the calling thread launched last (sfcvit_last_pos_embed_kernel).
extern thread_local KernelNote g_pos_embed;

}  // namespace sfcvit
