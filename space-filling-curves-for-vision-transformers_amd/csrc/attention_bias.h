// Attention with a learned relative position bias (include/sfcvit.h, "Self-attention core with a learned relative
// position bias"): what the host checks (attention_bias.cpp) and the kernels (attention_bias.hip) share.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"

namespace sfcvit {

constexpr int RELB_BLK = 64;                    // the block map's granularity = the tile of one workgroup (attn::BLK)
constexpr int RELB_MAX_N = SFCVIT_BIAS_MAX_N;
constexpr int RELB_MAX_T = SFCVIT_BIAS_MAX_BUCKETS;
constexpr int RELB_MAX_CHUNKS = 32;
constexpr int RELB_TARGET_GROUPS = 2048;        // workgroups of the table-gradient kernel worth splitting the batch for

inline int bias_blocks(int N) { return (N + RELB_BLK - 1) / RELB_BLK; }

// The table-gradient kernel's split of the batch: `per` consecutive images per workgroup, `chunks` workgroups per
// (head, visited block).  Enough chunks to fill the device, few enough to keep the workspace (16 KiB per chunk, head and
// block) small; a function of the shape alone, so the summation order is too.
struct BiasChunks { int per, chunks; };
inline BiasChunks bias_chunks(int B, int H, int visited_blocks) {
    const int64_t groups = int64_t(H) * visited_blocks;
    int want = int((RELB_TARGET_GROUPS + groups - 1) / groups);
    if (want > RELB_MAX_CHUNKS) want = RELB_MAX_CHUNKS;
    if (want > B) want = B;
    if (want < 1) want = 1;
    const int per = (B + want - 1) / want;
    return BiasChunks{per, (B + per - 1) / per};
}

// The argument checks of sfcvit_attention_bias_fwd / _bwd: SFCVIT_OK or the refusal (message recorded).  No HIP call,
// no pointer is dereferenced.
int attn_bias_check(const sfcvit_attn_bias_args *a, bool bwd, const char *what);

}  // namespace sfcvit
