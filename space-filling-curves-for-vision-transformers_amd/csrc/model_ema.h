// Model EMA inside the clip + AdamW step (include/sfcvit.h, "Model EMA"): the plan of sfcvit_adamw_ema_step, shared by the
// host checks (model_ema.cpp) and the launcher in optim.hip.  Every refusal is decided here, before any HIP call; no
// pointer is dereferenced beyond the two argument structs themselves.
#pragma once
#include <cstdint>

#include "../../include/sfcvit.h"
#include "rowwise.h"

namespace sfcvit {

constexpr int ADAMW_THREADS = 256;          // lanes of a workgroup of the optimizer's kernels (optim.hip and rowwise.hip assert it)
constexpr int ADAMW_MAX_BLOCKS = 2048;      // their grid cap, in adamw_plan and sumsq_plan (rowwise.cpp): beyond it the kernels stride

using AdamwEmaPlan = AdamwPlan;             // sfcvit_adamw_step's grid and kernel instance

// adamw_plan (what sfcvit_adamw_step refuses: null or misaligned buffers, n <= 0, step < 1 without dev_state) plus a null `e`, a
// null or misaligned e->ema, a decay outside [0, 1) and an ema that shares a byte with param, master, grad, m or v.
AdamwEmaPlan adamw_ema_plan(const sfcvit_adamw_args *a, const sfcvit_ema_args *e, const RowwiseKnobs &k);

}  // namespace sfcvit
