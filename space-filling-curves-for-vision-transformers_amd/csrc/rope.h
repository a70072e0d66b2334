// Rotary position embedding (include/sfcvit.h, "RoPE"): the 2x2 map [c -s; s c] on the interleaved channel pairs of the queries
// and keys of a packed projection, in place.  The plans of sfcvit_rope_fwd / sfcvit_rope_bwd, shared by the host checks
// (rope.cpp) and the launchers in rope.hip.  Every refusal is decided here, before any HIP call; no pointer is dereferenced.
//
// Geometry (both directions): QK-norm's lane map -- a group of 8 lanes owns one head row (hp / 64 16-byte vectors per lane, each
// 4 whole pairs), a wave owns the 8 consecutive head slots j = 8 * slot_group + (lane >> 3) of the 2 H slots (q heads, then k
// heads).  A wave fixes ONE token n and walks the batch, m = b * N + n, so its lanes' (c, s) are loaded once and stay in
// registers; a workgroup of ROPE_WAVES waves owns one slot group, ROPE_WAVES consecutive tokens (wave w: token
// ROPE_WAVES * token_block + w) and ROPE_BATCH_PER_WG consecutive images.  The grid is slot_groups * token_blocks *
// batch_chunks: a function of the shape alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

constexpr int ROPE_THREADS = 256, ROPE_WAVES = 4, ROPE_SLOTS = 8, ROPE_BATCH_PER_WG = 16;

struct RopePlan : PlanStatus {
    int B = 0, N = 0, H = 0, hd = 0, hp = 0;
    int vpl = 0;                        // 16-byte vectors per lane: hp / 64
    int slot_groups = 0;                // ceil(2 H / 8)
    int token_blocks = 0;               // ceil(N / ROPE_WAVES)
    int batch_chunks = 0;               // ceil(B / ROPE_BATCH_PER_WG)
    int blocks = 0;                     // slot_groups * token_blocks * batch_chunks,
                                        // workgroup = (slot_group * token_blocks + token_block) * batch_chunks + batch_chunk
    int part_ld = 0;                    // floats per workgroup in the backward's workspace: the column sums of its 8 slots, 8 hp
    int64_t ws_bytes = 0;               // blocks * part_ld * 4
    bool sums = false;                  // backward: the column sums are asked for (two launches), else one launch, no workspace
    int reduce_blocks = 0;              // second stage: 16 columns per block, then 1024 copied v sums per block
};

// Launch geometry alone (err set only where the shape itself has none): sfcvit_rope_bwd_ws and sfcvit_rope_plan read it.
RopePlan rope_geometry(int B, int N, int H, int hp, const char *what);
RopePlan rope_fwd_plan(const void *qkv, const void *table, int B, int N, int H, int hd, int hp);
// colsum, vsum, ws: optional.  colsum asks for the column sums of the stored dq | dk and needs ws; vsum (fp32 [H * hp], the v
// third's column sums of the attention backward) needs colsum, which is then [3 H hp] and receives them in its last third.
RopePlan rope_bwd_plan(const void *dqkv, const void *table, const void *colsum, const void *vsum, const void *ws, int B, int N, int H,
                       int hd, int hp);

}  // namespace sfcvit
