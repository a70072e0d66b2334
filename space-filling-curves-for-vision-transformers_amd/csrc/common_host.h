// Host-side helpers shared by every translation unit of libsfcvit_hip.so (plan.h, through dispatch.h: PlanStatus, refuse,
// ceil_div, aligned / aligned16, KernelNote).
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/sfcvit.h"
#include "dispatch.h"

namespace sfcvit {

namespace tile_desc {          // sfcvit_tile_descriptors (tile_descriptors.cpp) <-> patch_embed_tiled.hip
constexpr int MAXCLS = 8, DESC_HDR = 16;
}

// Records the message for sfcvit_last_error() and returns `code`.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void clear_error();
// hipGetLastError() -> SFCVIT_ELAUNCH with the HIP message, or SFCVIT_OK.
int check_launch(const char *what);
// Compute units of the current device (0 if unknown): the grid of the persistent kernels.
int device_cu_count();
// gemm8p.hip: 16 zero-initialised device words per (device, stream), shared by the persistent kernels (each leaves its words
// zero); allocated at the first call on a device (not inside a hipGraph capture: warm up first).  nullptr if unavailable.
unsigned *stream_counters(void *stream);
// Opt a kernel into `bytes` of dynamic LDS on the current device (once per kernel and device; 0 or an error code).
int raise_lds_limit(const void *kernel, int bytes, const char *what);

// The plan whose main kernel the calling thread's last sfcvit_gemm / sfcvit_attention_fwd / _bwd launched
// (sfcvit_last_gemm_kernel / sfcvit_last_attn_kernel name it as rocprofv3 does).
void note_gemm_kernel(const GemmPlan &p);
void note_attn_kernel(const AttnPlan &p);
void note_attn_kernel(const ProbePlan &p);      // sfcvit_attention_probs / _stats report through sfcvit_last_attn_kernel too
// g_attn: what note_attn_kernel formats into; the masked kernels (attention_masked.hip) have no plan and set it by name.
// g_rowwise: which row-wise kernel the calling thread's last sfcvit_layernorm_bwd* / sfcvit_add_layernorm_path_fwd launched
// (sfcvit_last_rowwise_kernel).  The other families keep theirs with their plans (g_tokenizer: tokenizer.h / tokenizer.cpp).
extern thread_local KernelNote g_attn, g_rowwise;

// rowwise.hip (layernorm.hip and the GEMM launchers call these too): out[n] = sum over `nparts` rows of part[nparts][N] in a
// fixed order; out fp32 or bf16.
int launch_colsum_reduce(const float *part, int nparts, int N, void *out, int out_bf16, void *stream);
// The general form: out[c] = sum_p part[p * ld + c], c < ncols.  Launched now -- or, between sfcvit_reduce_defer(1) and
// sfcvit_reduce_defer(0), queued for ONE batched launch at sfcvit_reduce_flush (every such reduction of a backward pass
// produces a parameter gradient nothing reads before the pass ends: 60 launches of 5 us per ViT-B step become one).
int reduce_cols(const float *part, int nparts, int ld, int ncols, void *out, int out_bf16, void *stream);
bool reduce_deferring();

}  // namespace sfcvit
