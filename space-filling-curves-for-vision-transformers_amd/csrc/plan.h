// The host scaffold every plan file shares (dispatch.cpp, attention_probe.cpp, token_agg.cpp, token_mix.cpp, pos_embed.cpp,
// token_pool.cpp, rowwise.cpp, drop_path.cpp, model_ema.cpp, grad_accum.cpp, tokenizer.cpp): the status a plan carries, how it refuses, three small helpers and the "which kernel ran last" note.
// Plain host C++ with no HIP include; refuse, KernelNote::set and KernelNote::read are defined in common.cpp.
#pragma once
#include <cstdint>

#include "../../include/sfcvit.h"

namespace sfcvit {

struct PlanStatus {
    int err = SFCVIT_OK;                                     // else an error code; msg says why
    char msg[256] = "";                                      // the longest refusal (the hierarchical envelope) is 200 characters
};
// Records the refusal in the plan; the entry point hands it to fail() (common_host.h) once the plan comes back.
void refuse(PlanStatus &p, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
// Inside a function that returns its plan `p` by value.
#define REFUSE(...) do { refuse(p, __VA_ARGS__); return p; } while (0)

// In int64_t whatever the operands are, so that a + b - 1 cannot leave the type; callers narrow what they know fits.
constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// bytes: a power of two.  NULL is aligned to everything: optional pointers pass.
inline bool aligned(const void *ptr, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(ptr) & (bytes - 1)) == 0; }
inline bool aligned16(const void *ptr) { return aligned(ptr, 16); }

// [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// The kernel symbol a family's launcher noted last, as rocprofv3 shows it.  One thread_local instance per family, defined in
// the .cpp that owns the family and set by its launcher just before the launch; sfcvit_last_*_kernel reads it.
struct KernelNote {
    char name[96] = "none";
    void set(const char *fmt, ...) __attribute__((format(printf, 2, 3)));
    int read(char *buf, int n) const;                        // SFCVIT_EINVAL on a null buffer or n <= 0
};

}  // namespace sfcvit
