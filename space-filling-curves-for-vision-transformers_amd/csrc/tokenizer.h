// The plans of the tokenizer family (patch_embed.hip, patch_embed_tiled.hip, hier_tokenizer.hip, mix.hip) on the scaffold of
// plan.h: every refusal, which kernel form a shape gets, its grid, LDS and workspace.  Plain host C++ (tokenizer.cpp): no HIP
// include, no getenv, no pointer dereferenced beyond the argument structs and the host arrays they carry (desc_cnt, P[],
// n_tokens[], the level pointers); hostcheck/host_check.cpp (check_tokenizer) pins them on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sfcvit.h"
#include "dispatch.h"

namespace sfcvit {

// ---- constants the plans share with the kernels ----
constexpr int GATHER_THREADS = 256, GATHER_IMG = 8;          // token gathers: lanes per token, images per workgroup
constexpr int PATCH_BM = GEN_TILE, PATCH_BN = GEN_TILE, PATCH_BK = GEN_BK, PATCH_THREADS = 256;   // generic patch embed: gemm_core.h's tiles
constexpr int PATCH_TILE_BYTES = 128 * 64 * 2;                  // one operand tile of it in LDS
constexpr int PE2_TM = 128, PE2_TN = 256, PE2_PT = 512;      // tiled forward: token rows, output columns; threads of both tiled kernels
constexpr int PE2_BW_ROWS = 64;                              // tiled backward: token rows per step
constexpr int PE2_MAXCLS = 8;                                // pixel orders inside a tile (tile_descriptors.cpp)
constexpr int PE2_FWD_LDS = 2 * PE2_TM * 128 + 2 * PE2_TN * 128 + PE2_TM * 16;   // two k-tiles of each operand + a 16-byte record per row
constexpr int PE2_BWD_LDS = 2 * 4 * PE2_BW_ROWS * 256;       // two stages of [dY half 0 | dY half 1 | X half 0 | X half 1]
constexpr int HT_ROWS = 64, HT_THREADS = 256, HT_MAXL = SFCVIT_HIER_MAX_LEVELS;   // fused hierarchical tokenizer
constexpr int HT_LDS_LIMIT = 160 * 1024;
constexpr int RS_MAXL = 8;                                   // levels of the resampling concatenation
constexpr int MIX_THREADS = 256, MIX_WAVES = MIX_THREADS / 64;

// Tuning switches, read once per process by read_tokenizer_knobs (common.cpp; the table in dispatch.h).
struct TokenizerKnobs {
    int gather_u = 1;                       // SFCVIT_GATHER_U: images per wave of the tile gather, 1 or 2
    int gather_nt = 3;                      // SFCVIT_GATHER_NT: nontemporal loads (1) / stores (2) of the tile gather
};
const TokenizerKnobs &read_tokenizer_knobs();

// ---- token gathers: sfcvit_tokens_gather, _tiles, _mix ----
enum class GatherForm : unsigned char { TILES, P256, ROWS };
struct GatherPlan : PlanStatus {
    GatherForm form = GatherForm::ROWS;     // tokens_gather_tiles_kernel<C, nt, upw, mix>, tokens_gather_p256_kernel, tokens_gather_kernel
    bool mix = false, x_bf16 = false;
    int C = 0, nt = 0, upw = 1;             // TILES: channels, nontemporal bits, images per wave (1 with a mix)
    int HW = 0;
    int grid_x = 0, grid_y = 0, threads = 0;
    size_t lds = 0;
    uint32_t wmagic = 0;                    // TILES: d / W == umulhi(d, wmagic) for d < 16 W
};
// `what` names the entry point in the messages; perm: the batch mix (the mixing kernels), else NULL.
GatherPlan gather_tiles_plan(const char *what, const void *x, const int32_t *pix, const int32_t *origin, const int32_t *perm, int B,
                             int C, int H, int W, int N, const void *tokens, int ld, const TokenizerKnobs &k);
GatherPlan gather_plan(const char *what, const void *x, int x_is_bf16, const int32_t *pix, const int32_t *perm, int B, int C, int HW,
                       int N, int P, const void *tokens, int ld);
// sfcvit_tokens_gather_mix: its own refusals, then gather_tiles_plan (with a tile origin table) or gather_plan.
GatherPlan gather_mix_plan(const void *x, const int32_t *pix, const int32_t *origin, const int32_t *perm, const uint32_t *rec, int B,
                           int C, int H, int W, int N, int P, const void *tokens, int ld, const TokenizerKnobs &k);

// ---- fused gather + projection: sfcvit_patch_embed_fwd / _bwd ----
enum class PeForm : unsigned char { TILED, GENERIC };
struct PatchEmbedPlan : PlanStatus {
    PeForm form = PeForm::GENERIC;          // pe2_fwd / pe2_bwd_kernel (patch_embed_tiled.hip), else pe_fwd / pe_bwd_kernel
    bool bwd = false, x_bf16 = false;
    int M = 0, K = 0, Kp = 0;               // B * N token rows, C * P features, K rounded up to 8
    int grid = 0;                           // the main kernel's workgroups
    size_t lds = 0;
    int permute_grid = 0;                   // forward: workgroups of the weight permutation
    int64_t wp_bytes = 0;                   // forward: the permuted-W region at the head of the workspace
    int n_row_tiles = 0, groups = 0;        // tiled forward: row tiles of PE2_TM rows, dealt to the 8 XCD slots in groups of 8
    int KR = 0, nz = 0;                     // tiled backward: rows per row range, row ranges over all classes
    int splits = 0, m_per_split = 0, zs = 0;   // generic backward: wanted k-ranges, rows of one, ranges that hold rows
    int64_t slab_bytes = 0;                 // backward: the fp32 slabs at the head of the workspace (tiled: nz; generic: `splits`, zs written)
    int reduce_grid = 0;                    // backward: workgroups of the slab reduction
    bool dbias = false;                     // backward: sfcvit_colsum over dY [M, D] follows
    int64_t ws_bytes = 0;                   // what sfcvit_patch_embed_workspace reports (0: no such shape)
};
// Rows per row range of the tiled backward: the smallest multiple of PE2_BW_ROWS for which the row ranges of all classes
// number at most G = 8 x max(1, 32 / tiles); *nz_out = that number (<= G by construction).  0 <= cnt[c], sum cnt = N.
int pe2_bwd_row_range(int B, int ncls, const int32_t *cnt, int tiles, int *nz_out);
// G slabs [D][C * 256] fp32: what the tiled backward needs at most, whatever the class counts are.
int64_t pe2_bwd_workspace(int C, int D);
// The workspace alone, no refusal: sfcvit_patch_embed_workspace asks it before the pointers exist.
PatchEmbedPlan patch_embed_geometry(int B, int C, int N, int P, int D, bool bwd);
PatchEmbedPlan patch_embed_plan(const sfcvit_patch_embed_args *a, bool bwd);

// ---- hierarchical tokenizer ----
struct HierPlan : PlanStatus {
    bool fuse = false, x_bf16 = false;      // hier_fwd_kernel<x_bf16, fuse>
    int kp_sum = 0, E = 0, M = 0;           // sum of the K_l rounded up to 32; L * D; B * N
    int h_stride = 0, a_stride = 0;         // LDS row strides in bytes
    int lds = 0, grid = 0;
};
// The fused kernel's envelope; E = L * D and kp_sum are valid when it returns true.
bool hier_envelope(int L, int D, int C, const int32_t *P, int &E, int &kp_sum);
HierPlan hier_plan(const sfcvit_hier_args *a);

struct ResamplePlan : PlanStatus {
    bool bwd = false;
    int blocks[RS_MAXL] = {};               // forward: [0]; backward: one launch per level
};
// lev: the level pointers (host array); cat: the concatenation (forward: out, backward: dout).
ResamplePlan resample_plan(bool bwd, const void *const *lev, const int32_t *n_tokens, int L, int B, int N0, int D, const void *cat);

// ---- MixUp / CutMix beside the gather (mix.hip) ----
struct MixPlan : PlanStatus {
    int vec = 1;                            // mix_images_kernel<vec>: pixels per lane, 4 or 1
    int HW = 0;
    int grid = 0, grid_y = 1;
};
MixPlan mix_images_plan(const void *x, const int32_t *perm, const uint32_t *rec, const void *out, int B, int C, int H, int W);
MixPlan soft_ce_pair_plan(const void *logits, const int64_t *y_a, const int64_t *y_b, const uint32_t *rec, const float *loss_rows, int B,
                          int C, int ld);

// What sfcvit_last_tokenizer_kernel reports: "tokens_gather_tiles_kernel<3, mix>", "pe2_bwd_kernel<bf16>",
// "hier_fwd_kernel<fp32, levels>", "hier_resample_concat_bwd_kernel".
void kernel_name(const GatherPlan &p, char *buf, size_t n);
void kernel_name(const PatchEmbedPlan &p, char *buf, size_t n);
void kernel_name(const HierPlan &p, char *buf, size_t n);
void kernel_name(const ResamplePlan &p, char *buf, size_t n);
// Which tokenizer kernel the calling thread launched last (sfcvit_last_tokenizer_kernel): the launchers note the plan's main
// kernel just before the launch.
extern thread_local KernelNote g_tokenizer;
template <class Plan>
void note_tokenizer_kernel(const Plan &p) { kernel_name(p, g_tokenizer.name, sizeof(g_tokenizer.name)); }

}  // namespace sfcvit
