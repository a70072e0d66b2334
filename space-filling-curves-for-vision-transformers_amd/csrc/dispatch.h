// Which kernels a GEMM or attention call runs: plain host C++ (dispatch.cpp), no HIP call, no kernel code.
//
// sfcvit_gemm and sfcvit_attention_fwd / _bwd validate and plan here, then only launch what the plan says; the plans are
// checked on the CPU by hostcheck/host_check.cpp.  kernel_name(plan) is the symbol rocprofv3 shows for the plan's main
// kernel (sfcvit_last_gemm_kernel / sfcvit_last_attn_kernel).
//
// Environment switches, for A/B measurements and tests (never needed in production).  Read by read_knobs and, the four of
// the row-wise family (rowwise.h: RowwiseKnobs) and the two of the tokenizer family (tokenizer.h: TokenizerKnobs),
// read_rowwise_knobs and read_tokenizer_knobs (common.cpp):
//   read per call (tests flip them between calls)
//     SFCVIT_GEMM_2PHASE       1        "0": four-phase k-tile schedule of the persistent GEMMs
//     SFCVIT_GEMM_STAGGER      4,200    "slots,ticks" (10 ns) start-up stagger of the persistent GEMM; "1,0" = off
//     SFCVIT_RESERVE_CUS       0        CUs the weight-gradient split of the persistent GEMM leaves free
//     SFCVIT_ATTN_LONG         1        "0": tiled attention kernels for 256 < N <= 608
//     SFCVIT_ATTN_BWD_FUSED    1        "0": two-kernel attention backward at N <= 224
//     SFCVIT_ATTN_DQSUM        kernel   "pass": dQ column sums from a separate pass over dqkv
//     SFCVIT_ATTN_BWD_PERSIST  1        "0": one workgroup per (batch, head) item in the one-pass backward
//     SFCVIT_ATTN_STAGGER_BWD  1 / 2,450  "slots,ticks" of the one-pass backward (persistent / one item per workgroup)
//     SFCVIT_ATTN_WIDE_STREAM  0        "1": streaming kernels for every any-length call with head dim > 64, also where the
//                                       whole-sequence kernels fit (A/B timing, small-N tests)
//   read once per process
//     SFCVIT_GEMM_WALK         6 if N >= 1792, else 0  tile-walk window width of the persistent GEMM; 0 = row-major
//     SFCVIT_ATTN_BWD_QUEUE    1        "0": fixed item stride in the persistent attention backward
//     SFCVIT_ATTN_NT           0        bit 0: nontemporal LDS-DMA in the attention backward
//     SFCVIT_LN_COLS           1        "0": 16-byte-vector LayerNorm backward also at D = 768 (ln_bwd_plan)
//     SFCVIT_LN_BLOCKS         0 (auto) workgroups of the LayerNorm backward (ln_bwd_plan)
//     SFCVIT_LN_FWD_TWO_ROWS   1        "0": one row per wave in the LayerNorm forward (ln_fwd_plan)
//     SFCVIT_ADAMW_NT          3        nontemporal loads (1) / stores (2) of the optimizer state (adamw_plan, grad_accum_plan)
//     SFCVIT_GATHER_U          1        images per wave of the tile gather, 1 or 2 (gather_tiles_plan)
//     SFCVIT_GATHER_NT         3        nontemporal loads (1) / stores (2) of the tile gather (gather_tiles_plan)
#pragma once
#include <cstddef>

#include "../../include/sfcvit.h"
#include "plan.h"

namespace sfcvit {

// ---- constants the plans share with the kernels ----
constexpr int GEN_TILE = 128, GEN_BK = 64;                   // generic GEMM kernel: 128 x 128 tiles, 64-deep k-tiles
constexpr int P8_LDS_BIAS = 2 * 65536 + 64 + 8 * 2048;       // persistent GEMM: LDS offset of the bias vector
constexpr int P8_LDS_MAX = 160 * 1024;
constexpr int BIAS_MAX_N = (P8_LDS_MAX - P8_LDS_BIAS) / 2;   // the bias vector lives in LDS
enum { P8_RELU = 1, P8_DROP = 2, P8_RES = 4, P8_DACT = 8, P8_CSUM = 16, P8_BITS = 32 };   // gemm8p_kernel MASK bits

constexpr int ATTN_HD = 64, ATTN_BLK = 64;                  // head dim of all but the wide family; tiled kernels' block rows
constexpr int ATTN_LDS_LIMIT = 160 * 1024;
constexpr int SEQ_MAX_N = 256;                               // whole-sequence attention kernels (seq and wide families)
constexpr int SEQ_MAX_LDS = 2 * SEQ_MAX_N * 128 + 3 * SEQ_MAX_N * 4;
constexpr int LONG_MAX_N = 608;                              // 2 images x 608 rows x 128 B = 152 KiB
constexpr int LONG_NPAD_MAX = (LONG_MAX_N + 31) / 32 * 32;
constexpr int LONG_MAX_LDS = 2 * LONG_NPAD_MAX * 128 + 3 * LONG_NPAD_MAX * 4;
constexpr int FUSED_MAX_N = 224;                             // one-pass backward: 7 chunks of 32 rows
constexpr int FUSED_ROW_BYTES = 4 * 128 + 2 * 64 + 6 * 4;    // LDS bytes per padded sequence row: Q, dO, two K images; dS exchange x 2; two sets of lse / delta / row key
constexpr int FUSED_CS_BYTES = 16 * 128 * 4;                 // column-sum staging [FWAVES][dK | dV][64] floats
constexpr int FUSED_POST_BYTES = 8192;                       // own scratch: the [32][64] partial dK / dV of a shared fragment (+ as much again for short sequences, whose K image is too small for the column-sum staging)
constexpr int FUSED_EXTRA = 256 + 64 + 14 * 64 * 4;          // (256 spare) + two item records (3 pointers each, 8-byte slots) + the key waves' shares of the dQ column sums [14][64]
constexpr int FUSED_MAX_LDS = FUSED_MAX_N * FUSED_ROW_BYTES + FUSED_EXTRA + FUSED_POST_BYTES;
// head dims 128 / 192 / 256 (S = hd / 64): Q | K or K | V images of the whole sequence, + lse / delta / row key (dK / dV kernel)
constexpr size_t wide_lds(int S, int npad, bool kv) { return size_t(2) * S * npad * 128 + (kv ? size_t(3) * npad * 4 : 0); }
// head dims 128 / 192 / 256, any N (attention_wide_stream.hip): one 64-row block of K | V or Q | dO, + lse / delta / row key
constexpr size_t stream_lds(int S, bool kv) { return wide_lds(S, ATTN_BLK, kv); }

// ---- switches ----
struct Knobs {
    bool gemm_2phase = true;                                 // SFCVIT_GEMM_2PHASE
    int gemm_stagger_slots = 4, gemm_stagger_ticks = 200;    // SFCVIT_GEMM_STAGGER
    int reserve_cus = 0;                                     // SFCVIT_RESERVE_CUS
    bool attn_long = true;                                   // SFCVIT_ATTN_LONG
    bool attn_bwd_fused = true;                              // SFCVIT_ATTN_BWD_FUSED
    bool attn_dq_in_kernel = true;                           // SFCVIT_ATTN_DQSUM
    bool attn_bwd_persist = true;                            // SFCVIT_ATTN_BWD_PERSIST
    int attn_stagger_slots = 0, attn_stagger_ticks = 450;    // SFCVIT_ATTN_STAGGER_BWD (slots 0: the plan's default)
    bool attn_wide_stream = false;                           // SFCVIT_ATTN_WIDE_STREAM
    int gemm_walk = -1;                                      // SFCVIT_GEMM_WALK (-1: the plan's default)
    bool attn_bwd_queue = true;                              // SFCVIT_ATTN_BWD_QUEUE
    int attn_nt = 0;                                         // SFCVIT_ATTN_NT
};
// The per-call switches of one entry point (the others keep their defaults) + the read-once ones.
enum KnobScope { KNOBS_GEMM, KNOBS_ATTN_FWD, KNOBS_ATTN_BWD };
Knobs read_knobs(KnobScope scope);
// getenv, parsed: the integer value (def if unset); whether the value starts with '0'; its first character (0 if unset);
// "a,b" into *a and *b as far as it parses (returns the number of fields parsed).
int env_int(const char *name, int def);
char env_first(const char *name);
inline bool env_off(const char *name) { return env_first(name) == '0'; }
int env_pair(const char *name, int *a, int *b);

// ---- GEMM ----
enum class GemmFamily : unsigned char { P8, P8_KM, RING, GENERIC };
struct GemmPlan : PlanStatus {
    GemmFamily family = GemmFamily::GENERIC;
    bool a_km = false, b_km = false, heavy = false;          // ring / generic template arguments (heavy: GELU epilogue)
    int ni = 0, mask = 0;                                    // persistent kernels: tile rows / 32, epilogue MASK
    bool p2 = true;                                          // persistent kernels: two-phase k-tile schedule
    int bn = 0;                                              // ring: 128 or 256
    int grid = 0;                                            // workgroups along x (ring: z = splits)
    int splits = 1, k_per_split = 0;                         // k-ranges of the main launch; k per range (P8_KM: k-tiles of 64)
    int walk = 0, stag_slots = 1, stag_ticks = 0;            // P8: tile walk and start-up stagger
    int k_done = 0, tail_slab = -1;                          // P8_KM: rows k_done.. K-1 as one more generic launch into slab tail_slab
    int colsum_parts = 0;                                    // post: launch_colsum_reduce over the P8 epilogue's partial rows
    int reduce_slabs = 0;                                    // post: splitk_reduce over this many slabs
    bool actmask_pass = false;                               // post: relu_bits_kernel over C
    bool colsum_pass = false;                                // post: sfcvit_colsum over C
};
GemmPlan gemm_plan(const sfcvit_gemm_args &a, int cus, const Knobs &k);

// ---- attention ----
enum class AttnFamily : unsigned char { WIDE, SEQ, LONG, TILED, FUSED, STREAM };
enum class Colsum : unsigned char { NONE, PARTIALS, PARTIALS_QPASS, PASS };
struct AttnPlan : PlanStatus {
    AttnFamily family = AttnFamily::TILED;
    bool bwd = false, drop = false;
    int inst = 0;                                            // template instance: NFC (13 / 36 / 0) or, wide, S = hd / 64
    int npad = 0, npad2 = 0;                                 // padded rows of the (first, second) kernel
    size_t lds = 0, lds2 = 0;                                // dynamic LDS of the (first, second) kernel
    int grid = 0;                                            // FUSED: workgroups; TILED, STREAM: query / key blocks
    bool queue = false;                                      // FUSED: items dealt from the stream's counters
    int round = 0, per = 0, ticks = 0, nt = 0, dq_sums = 0;  // FUSED: stagger, nontemporal DMA, dQ column sums in the kernel
    Colsum colsum = Colsum::NONE;                            // bwd: where the column sums of dqkv come from
};
// any_length (sfcvit_attention_fwd_any / _bwd_any): head dims 128 / 192 / 256 run on the STREAM kernels where the
// whole-sequence ones would refuse for LDS (or always, with SFCVIT_ATTN_WIDE_STREAM=1); every other plan is unchanged.
AttnPlan attn_fwd_plan(const sfcvit_attn_args &a, const Knobs &k, bool any_length = false);
AttnPlan attn_bwd_plan(const sfcvit_attn_args &a, int cus, const Knobs &k, bool any_length = false);

// ---- attention maps / statistics (attention_probe.cpp plans, attention_probe.hip launches) ----
constexpr int PROBE_POS_BYTES = 2 * ATTN_BLK * 4;            // stats kernel: (row, col) of the staged block's 64 keys
struct ProbePlan : PlanStatus {
    bool stats = false;                                      // sfcvit_attention_stats, else sfcvit_attention_probs
    int inst = 0;                                            // S = hd / 64
    bool mean = false;                                       // map kernel: heads summed inside the workgroup
    int blocks = 0;                                          // 64-row blocks along N (queries; the map kernel: keys too)
    int grid_z = 0;                                          // stats: B (y = H); map: B, or B * H without head_mean
    size_t lds = 0;                                          // one 64-key block of K (+ its positions)
};
ProbePlan attn_probe_plan(const sfcvit_attn_probe_args &a, bool stats);
void kernel_name(const ProbePlan &p, char *buf, size_t n);

// The symbol of the plan's main kernel, e.g. "gemm8p_kernel<7, 35, true>" or "attn_seq_bwd_fused_kernel<13, true>".
void kernel_name(const GemmPlan &p, char *buf, size_t n);
void kernel_name(const AttnPlan &p, char *buf, size_t n);

}  // namespace sfcvit
