// Masked / windowed attention (include/sfcvit.h, "Masked / windowed self-attention core"): what the host checks
// (attention_masked.cpp) and the kernels (attention_masked.hip) share.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"

namespace sfcvit {

constexpr int MASK_BLK = SFCVIT_MASK_BLOCK;     // the block map's granularity = the tile of one workgroup (attn::BLK)
constexpr int MASK_MAX_N = SFCVIT_MASK_MAX_N;
// block map values
constexpr uint8_t MASK_SKIP = 0, MASK_MIXED = 1, MASK_ZERO = 2;

inline int mask_blocks(int N) { return (N + MASK_BLK - 1) / MASK_BLK; }

// The argument checks of sfcvit_attention_masked_fwd / _bwd: SFCVIT_OK or the refusal (message recorded).  No HIP call,
// no pointer is dereferenced.
int attn_masked_check(const sfcvit_attn_mask_args *a, bool bwd, const char *what);

}  // namespace sfcvit
