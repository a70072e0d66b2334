// Model EMA inside the clip + AdamW step (include/sfcvit.h, "Model EMA"): the plan of sfcvit_adamw_ema_step, shared by the
// host checks (model_ema.cpp) and the launcher in rowwise.hip.  Every refusal is decided here, before any HIP call; no
// pointer is dereferenced beyond the two argument structs themselves.
#pragma once
#include <cstdint>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

constexpr int ADAMW_THREADS = 256;          // lanes of a workgroup of adamw_kernel / adamw_ema_kernel (rowwise.hip asserts it)
constexpr int ADAMW_MAX_BLOCKS = 2048;      // grid cap of the row-wise launchers: beyond it the kernels stride

struct AdamwEmaPlan : PlanStatus {
    int grid = 0;                           // workgroups: one lane per 8 parameters, rounded up, 1 .. ADAMW_MAX_BLOCKS
};

// Refuses what sfcvit_adamw_step refuses (null or misaligned buffers, n <= 0, step < 1 without dev_state), a null `e`, a null
// or misaligned e->ema, a decay outside [0, 1) and an ema that shares a byte with param, master, grad, m or v.
AdamwEmaPlan adamw_ema_plan(const sfcvit_adamw_args *a, const sfcvit_ema_args *e);

}  // namespace sfcvit
