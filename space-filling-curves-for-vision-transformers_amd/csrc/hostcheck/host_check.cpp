// Sanitizer driver for the HOST-ONLY code of libsfcvit_hip.so ("Race detection / sanitizers": GPU ASan is not
// available on this pool, so the native host code gets a CPU-side -fsanitize=address,undefined build of its own):
//   sfcvit_curve_table / _rc (curves.cpp), sfcvit_pixel_table (curves.cpp), sfcvit_tile_descriptors (patch_embed_tiled.hip,
//   host part), the error path of common.cpp, the mask validation and block map of attention_masked.cpp (check_mask_blocks),
//   the index validation, inverted index, workspace and argument checks of attention_bias.cpp (check_attention_bias),
//   the plans and refusals of pos_embed.cpp (check_pos_embed), token_pool.cpp (check_token_pool), token_agg.cpp (check_dwconv),
//   token_mix.cpp (check_tokmix), rowwise.cpp (check_rowwise), tokenizer.cpp (check_tokenizer), drop_path.cpp (check_drop_path), layer_scale.cpp (check_layer_scale), qk_norm.cpp (check_qk_norm), rope.cpp (check_rope), model_ema.cpp (check_model_ema) and grad_accum.cpp (check_grad_accum), and the kernel selection of dispatch.cpp (check_dispatch: which kernel, grid, splits
//   and post passes each GEMM / attention shape of the benchmarked models gets).
// Every buffer is a heap block of EXACTLY the documented size, so that an off-by-one in a generator or in the descriptor
// writer is a heap-buffer-overflow report instead of silent corruption.
// Built and run by `make asan` (tests/test_host_cpu.py::test_host_code_is_clean_under_address_sanitizer).  No GPU call.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../../../include/sfcvit.h"
#include "../attention_bias.h"
#include "../dispatch.h"
#include "../drop_path.h"
#include "../grad_accum.h"
#include "../layer_scale.h"
#include "../model_ema.h"
#include "../pos_embed.h"
#include "../qk_norm.h"
#include "../rope.h"
#include "../rowwise.h"
#include "../token_agg.h"
#include "../token_mix.h"
#include "../token_pool.h"
#include "../tokenizer.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "host_check: " __VA_ARGS__); std::fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); g_fail++; } } while (0)

static bool is_permutation(const int32_t *t, int n2) {
    std::vector<char> seen(n2, 0);
    for (int i = 0; i < n2; i++) {
        if (t[i] < 0 || t[i] >= n2 || seen[t[i]]) return false;
        seen[t[i]] = 1;
    }
    return true;
}

// ---- kernel selection (dispatch.cpp), cus = 256 as on the MI355X; the plans read no pointer, so fake aligned ones serve ----
using namespace sfcvit;
static void *ptr(int i) { return reinterpret_cast<void *>(uintptr_t(0x100000) * uintptr_t(i + 1)); }

struct G {                  // one sfcvit_gemm call as sfcvit.ops makes it
    int M, N, K, akm, bkm, fg;
    unsigned epi;           // E_* below
    int splitk;
    const char *name;       // expected kernel_name, or an error message prefix when it starts with "gemm:"
    int grid, splits, post; // expected grid / splits (0: not checked); post: P_* bits that must be on (all others off)
};
enum { E_BIAS = 1, E_RES = 2, E_DROP = 4, E_RELU = 8, E_DACT = 16, E_CSUM = 32, E_BITS = 64, E_GELU = 128 };
enum { P_PARTS = 1, P_REDUCE = 2, P_ACTMASK = 4, P_COLSUM = 8, P_TAIL = 16 };

static sfcvit_gemm_args gemm_args(const G &g) {
    sfcvit_gemm_args a{};
    a.a = ptr(0); a.b = ptr(1); a.c = ptr(2);
    a.M = g.M; a.N = g.N; a.K = g.K;
    a.lda = g.akm ? g.M : g.K; a.ldb = g.bkm ? g.N : g.K; a.ldc = g.N;
    a.a_kmajor = g.akm; a.b_kmajor = g.bkm;
    a.force_generic = g.fg;
    a.splitk = g.splitk;
    if (g.splitk > 1) { a.workspace = ptr(3); a.workspace_bytes = int64_t((g.splitk + 7) / 8 * 8) * g.M * g.N * 4; }
    if (g.epi & E_BIAS) a.bias = ptr(4);
    if (g.epi & E_RES) { a.residual = ptr(5); a.ldr = g.N; }
    if (g.epi & E_DROP) { a.dropout_p = 0.1f; a.dropout_seed = 7; }
    if (g.epi & E_RELU) a.act = SFCVIT_ACT_RELU;
    if (g.epi & E_GELU) a.act = SFCVIT_ACT_GELU;
    if (g.epi & E_DACT) { a.dact = SFCVIT_ACT_RELU; a.aux_in = ptr(6); a.ldaux = g.N; a.dact_scale = 1.f / 0.9f; }
    if (g.epi & E_CSUM) { a.colsum_out = ptr(7); a.workspace = ptr(3); a.workspace_bytes = int64_t(1) << 30; }
    if (g.epi & E_BITS) { a.actmask = ptr(8); a.ld_actmask = g.N / 8; }
    return a;
}

static void check_gemm(const G &g, const Knobs &k, const char *what) {
    const sfcvit_gemm_args a = gemm_args(g);
    const GemmPlan p = gemm_plan(a, 256, k);
    if (!std::strncmp(g.name, "gemm:", 5)) {
        CHECK(p.err == SFCVIT_EINVAL && std::strstr(p.msg, g.name), "%s: want error '%s', got %d '%s'", what, g.name, p.err, p.msg);
        return;
    }
    char name[96];
    kernel_name(p, name, sizeof(name));
    CHECK(p.err == SFCVIT_OK && !std::strcmp(name, g.name), "%s: want %s, got %s (%s)", what, g.name, name, p.msg);
    if (g.grid) CHECK(p.grid == g.grid, "%s: grid %d, want %d", what, p.grid, g.grid);
    if (g.splits) CHECK(p.splits == g.splits, "%s: splits %d, want %d", what, p.splits, g.splits);
    const int post = (p.colsum_parts ? P_PARTS : 0) | (p.reduce_slabs ? P_REDUCE : 0) | (p.actmask_pass ? P_ACTMASK : 0) |
                     (p.colsum_pass ? P_COLSUM : 0) | (p.tail_slab >= 0 ? P_TAIL : 0);
    CHECK(post == g.post, "%s: post passes %#x, want %#x", what, post, g.post);
}

// attention maps / statistics (attention_probe.cpp): accepted argument sets with their kernel and launch geometry, and the
// refusals of include/sfcvit.h
static void check_probe() {
    auto base = [](int B, int N, int H, int hd) {
        sfcvit_attn_probe_args a{};
        a.qkv = ptr(0); a.lse = static_cast<float *>(ptr(1));
        a.B = B; a.N = N; a.H = H; a.hd = hd; a.scale = 0.125f;
        return a;
    };
    char name[96];
    {
        sfcvit_attn_probe_args a = base(256, 196, 12, 64);
        a.probs = ptr(2);
        ProbePlan p = attn_probe_plan(a, false);
        kernel_name(p, name, sizeof(name));
        CHECK(p.err == SFCVIT_OK && !std::strcmp(name, "attn_probe_map_kernel<1, false>") && p.blocks == 4 && p.grid_z == 3072 && p.lds == 8192,
              "probe map: %s blocks %d z %d lds %zu (%s)", name, p.blocks, p.grid_z, p.lds, p.msg);
        a.head_mean = 1; a.probs_is_bf16 = 1; a.hd = 256; a.N = 577;
        p = attn_probe_plan(a, false);
        kernel_name(p, name, sizeof(name));
        CHECK(p.err == SFCVIT_OK && !std::strcmp(name, "attn_probe_map_kernel<4, true>") && p.blocks == 10 && p.grid_z == 256 && p.lds == 32768,
              "probe mean map: %s blocks %d z %d lds %zu (%s)", name, p.blocks, p.grid_z, p.lds, p.msg);
        a.head_mean = 0; a.B = 8192;                                 // B * H maps beyond the launch grid
        CHECK(attn_probe_plan(a, false).err == SFCVIT_EINVAL, "probe map: B * H = 98304 accepted");
        a = base(1, 1, 1, 128);
        a.mass_rows = static_cast<float *>(ptr(3));
        p = attn_probe_plan(a, true);
        kernel_name(p, name, sizeof(name));
        CHECK(p.err == SFCVIT_OK && !std::strcmp(name, "attn_probe_stats_kernel<2>") && p.blocks == 1 && p.grid_z == 1 && p.lds == 2 * 8192 + 512,
              "probe stats: %s blocks %d z %d lds %zu (%s)", name, p.blocks, p.grid_z, p.lds, p.msg);
        a.pos = static_cast<float *>(ptr(4)); a.dist_rows = static_cast<float *>(ptr(5));
        CHECK(attn_probe_plan(a, true).err == SFCVIT_OK, "probe stats with pos + dist_rows refused");
    }
    for (int stats = 0; stats < 2; stats++) {
        auto full = [&](int B, int N, int H, int hd) {
            sfcvit_attn_probe_args a = base(B, N, H, hd);
            a.probs = ptr(2); a.pos = static_cast<float *>(ptr(4)); a.dist_rows = static_cast<float *>(ptr(5));
            return a;
        };
        auto refused = [&](const sfcvit_attn_probe_args &a, const char *frag, const char *what) {
            const ProbePlan p = attn_probe_plan(a, stats != 0);
            CHECK(p.err == SFCVIT_EINVAL && std::strstr(p.msg, frag), "probe %d %s: want '%s', got %d '%s'", stats, what, frag, p.err, p.msg);
        };
        CHECK(attn_probe_plan(full(2, 65, 3, 192), stats != 0).err == SFCVIT_OK, "probe %d: valid arguments refused", stats);
        sfcvit_attn_probe_args a = full(2, 65, 3, 64);
        a.qkv = nullptr; refused(a, "null", "null qkv");
        a = full(2, 65, 3, 64); a.lse = nullptr; refused(a, "null", "null lse");
        refused(full(2, 65, 3, 48), "head dim 48 not supported", "hd 48");
        refused(full(2, 0, 3, 64), "N=0", "N = 0");
        refused(full(0, 65, 3, 64), "B=0", "B = 0");
        a = full(2, 65, 3, 64); a.qkv = reinterpret_cast<void *>(uintptr_t(0x100008)); refused(a, "aligned", "misaligned qkv");
        a = full(2, 65, 3, 64); a.scale = 0.f; refused(a, "scale", "scale 0");
        if (stats) {
            a = full(2, 65, 3, 64); a.dist_rows = nullptr; refused(a, "every output is NULL", "no output");
            a = full(2, 65, 3, 64); a.pos = nullptr; refused(a, "needs pos", "dist_rows without pos");
            a = full(2, 65, 3, 64); a.dist_rows = reinterpret_cast<float *>(uintptr_t(0x600004)); refused(a, "aligned", "misaligned output");
        } else {
            a = full(2, 65, 3, 64); a.probs = nullptr; refused(a, "null", "null probs");
            a = full(2, 65, 3, 64); a.probs = reinterpret_cast<void *>(uintptr_t(0x300002)); refused(a, "aligned", "misaligned probs");
            a = full(2, 65, 3, 64); a.head_mean = 2; refused(a, "must be 0 or 1", "head_mean 2");
        }
    }
}

static void check_dispatch() {
    const Knobs dflt;
    // ViT-B/16 @ 224, batch 256 (M = 256 x 196 tokens), training (dropout 0.1) -- the benched step
    const int M = 50176;
    const G vit_b[] = {
        {M, 2304, 768, 0, 0, 0, E_BIAS, 1, "gemm8p_kernel<8, 0, true>", 256, 1, 0},                               // in_proj
        {M, 768, 768, 0, 0, 0, E_BIAS | E_RES | E_DROP, 1, "gemm8p_kernel<7, 6, true>", 256, 1, 0},              // out_proj
        {M, 3072, 768, 0, 0, 0, E_BIAS | E_RELU | E_DROP | E_BITS, 1, "gemm8p_kernel<8, 35, true>", 256, 1, 0},   // linear1
        {M, 768, 3072, 0, 0, 0, E_BIAS | E_RES | E_DROP, 1, "gemm8p_kernel<7, 6, true>", 256, 1, 0},             // linear2
        {M, 3072, 768, 0, 0, 0, E_DACT | E_CSUM | E_BITS, 1, "gemm8p_kernel<8, 56, true>", 256, 1, P_PARTS},      // linear2 dX (+ db1)
        {M, 768, 3072, 0, 0, 0, E_RES, 1, "gemm8p_kernel<7, 4, true>", 256, 1, 0},                               // linear1 dX
        {M, 768, 768, 0, 0, 0, 0, 1, "gemm8p_kernel<7, 0, true>", 256, 1, 0},                                    // out_proj dX
        {M, 768, 2304, 0, 0, 0, E_RES, 1, "gemm8p_kernel<7, 4, true>", 256, 1, 0},                               // in_proj dX
        {2304, 768, M, 1, 1, 0, 0, 9, "gemm8p_km_kernel<true>", 248, 9, P_REDUCE},                                // dW in_proj
        {768, 768, M, 1, 1, 0, 0, 28, "gemm8p_km_kernel<true>", 256, 28, P_REDUCE},                              // dW out_proj
        {3072, 768, M, 1, 1, 0, 0, 7, "gemm8p_km_kernel<true>", 256, 7, P_REDUCE},                               // dW linear1
        {768, 3072, M, 1, 1, 0, 0, 7, "gemm8p_km_kernel<true>", 256, 7, P_REDUCE},                               // dW linear2
        // eval / no dropout
        {M, 768, 768, 0, 0, 0, E_BIAS | E_RES, 1, "gemm8p_kernel<7, 4, true>", 256, 1, 0},
        {M, 3072, 768, 0, 0, 0, E_BIAS | E_RELU | E_BITS, 1, "gemm8p_kernel<8, 33, true>", 256, 1, 0},
        {M, 3072, 768, 0, 0, 0, E_BIAS | E_RELU, 1, "gemm8p_kernel<8, 1, true>", 256, 1, 0},
        // RELU + RES has no persistent epilogue: the ring kernel, and the bits from a pass over C
        {M, 768, 768, 0, 0, 0, E_RES | E_RELU | E_BITS, 1, "gemm256_kernel<false, false, 128, false>", 1176, 1, P_ACTMASK},
        // batch 64 (M = 64 x 196), the shape the GPU tests assert (test_dropout_gpu BENCHED_KERNELS, test_parity_gpu
        // vit_b_hilbert224_b64; both ignore the tile height): 224-row tiles at N = 2 304 / 3 072, 192-row at N = 768
        {12544, 2304, 768, 0, 0, 0, E_BIAS, 1, "gemm8p_kernel<7, 0, true>", 256, 1, 0},
        {12544, 768, 768, 0, 0, 0, E_BIAS | E_RES | E_DROP, 1, "gemm8p_kernel<6, 6, true>", 256, 1, 0},
        {12544, 3072, 768, 0, 0, 0, E_BIAS | E_RELU | E_DROP | E_BITS, 1, "gemm8p_kernel<7, 35, true>", 256, 1, 0},
        {12544, 3072, 768, 0, 0, 0, E_BIAS | E_RELU | E_BITS, 1, "gemm8p_kernel<7, 33, true>", 256, 1, 0},
        {12544, 3072, 768, 0, 0, 0, E_DACT | E_CSUM | E_BITS, 1, "gemm8p_kernel<7, 56, true>", 256, 1, P_PARTS},
        {12544, 768, 3072, 0, 0, 0, E_RES, 1, "gemm8p_kernel<6, 4, true>", 256, 1, 0},
        {12544, 768, 768, 0, 0, 0, 0, 1, "gemm8p_kernel<6, 0, true>", 256, 1, 0},
        {2304, 768, 12544, 1, 1, 0, 0, 9, "gemm8p_km_kernel<true>", 248, 9, P_REDUCE},
        // the head (rank 64, 1 536 outputs, 1 000 classes): off the persistent kernels
        {M, 64, 768, 0, 0, 0, 0, 1, "gemm_kernel<false, false, false>", 392, 1, 0},                              // h = z W_emb^T
        {256, 1536, 12544, 0, 0, 0, 0, 8, "gemm256_kernel<false, false, 128, false>", 12, 8, P_REDUCE},         // y1
        {256, 1000, 1536, 0, 0, 0, E_BIAS, 1, "gemm_kernel<false, false, false>", 16, 1, 0},                     // logits
        {1000, 1536, 256, 1, 1, 0, 0, 1, "gemm_kernel<true, true, false>", 96, 1, 0},                            // dW classifier
        {256, 1536, 1000, 0, 1, 0, 0, 1, "gemm_kernel<false, true, false>", 24, 1, 0},                           // d(a)
        {1536, 12544, 256, 1, 1, 0, 0, 1, "gemm_kernel<true, true, false>", 0, 1, 0},                            // dW_seq
        {256, 12544, 1536, 0, 1, 0, 0, 1, "gemm_kernel<false, true, false>", 0, 1, 0},                           // dh
        {64, 768, M, 1, 1, 0, 0, 56, "gemm_kernel<true, true, false>", 336, 56, P_REDUCE},                       // dW_emb
        {M, 768, 64, 0, 0, 0, 0, 1, "gemm256_kernel<false, false, 128, false>", 1176, 1, 0},                     // dz
        // ViT-Tiny widths (D = 192, MLP 768, 4 tokens at 32 px): no persistent-kernel shape
        {1024, 576, 192, 0, 0, 0, E_BIAS, 1, "gemm_kernel<false, false, false>", 0, 1, 0},                       // in_proj
        {1024, 768, 192, 0, 0, 0, E_BIAS | E_RELU, 1, "gemm256_kernel<false, false, 128, false>", 24, 1, 0},    // linear1
        {1024, 768, 192, 0, 0, 0, E_BIAS | E_GELU, 1, "gemm256_kernel<false, false, 128, true>", 24, 1, 0},     // GELU epilogue
        // weight gradient with K % 128 != 0 (batch 100): the last 16 rows as one more slab
        {768, 768, 19600, 1, 1, 0, 0, 28, "gemm8p_km_kernel<true>", 0, 26, P_REDUCE | P_TAIL},
        // every force_generic value
        {M, 768, 768, 0, 0, SFCVIT_GEMM_GENERIC, 0, 1, "gemm_kernel<false, false, false>", 2352, 1, 0},
        {M, 768, 768, 0, 0, SFCVIT_GEMM_RING, 0, 1, "gemm256_kernel<false, false, 128, false>", 1176, 1, 0},
        {M, 2304, 768, 0, 0, SFCVIT_GEMM_RING, 0, 1, "gemm256_kernel<false, false, 256, false>", 1764, 1, 0},
        {M, 2304, 768, 0, 0, SFCVIT_GEMM_RING_256x128, 0, 1, "gemm256_kernel<false, false, 128, false>", 3528, 1, 0},
        {M, 768, 768, 0, 0, SFCVIT_GEMM_RING_256x256, 0, 1, "gemm256_kernel<false, false, 256, false>", 588, 1, 0},
        {M, 768, 768, 0, 1, SFCVIT_GEMM_RING, 0, 1, "gemm256_kernel<false, true, 128, false>", 0, 1, 0},
        {M, 768, 768, 0, 0, SFCVIT_GEMM_P8_256, 0, 1, "gemm8p_kernel<8, 0, true>", 256, 1, 0},
        {M, 768, 768, 0, 0, SFCVIT_GEMM_P8_224, 0, 1, "gemm8p_kernel<7, 0, true>", 256, 1, 0},
        {M, 768, 768, 0, 0, SFCVIT_GEMM_P8_192, 0, 1, "gemm8p_kernel<6, 0, true>", 256, 1, 0},
        {2304, 768, M, 1, 1, SFCVIT_GEMM_P8_256, 0, 9, "gemm8p_km_kernel<true>", 248, 9, P_REDUCE},
        {M, 64, 768, 0, 0, SFCVIT_GEMM_P8_256, 0, 1, "gemm: shape / options not eligible for the persistent 8-phase kernel", 0, 0, 0},
        {M, 768, 768, 0, 0, SFCVIT_GEMM_AUTO, E_GELU | E_BIAS, 1, "gemm256_kernel<false, false, 128, true>", 0, 1, 0},
        // argument checks
        {M, 768, 770, 0, 0, 0, 0, 1, "gemm: K=770 must be a multiple of 8", 0, 0, 0},
        {M, 768, 768, 0, 0, 0, E_BIAS, 4, "gemm: split-K supports no epilogue", 0, 0, 0},
    };
    char what[64];
    for (const G &g : vit_b) {
        std::snprintf(what, sizeof(what), "gemm %dx%dx%d fg %d epi %#x", g.M, g.N, g.K, g.fg, g.epi);
        check_gemm(g, dflt, what);
    }
    {   // SFCVIT_GEMM_2PHASE=0: the four-phase schedule of both persistent forms
        Knobs k;
        k.gemm_2phase = false;
        check_gemm({M, 768, 768, 0, 0, 0, 0, 1, "gemm8p_kernel<7, 0, false>", 256, 1, 0}, k, "2PHASE=0 gemm8p");
        check_gemm({2304, 768, M, 1, 1, 0, 0, 9, "gemm8p_km_kernel<false>", 248, 9, P_REDUCE}, k, "2PHASE=0 km");
    }
    {   // persistent GEMM: tile walk, start-up stagger and SFCVIT_GEMM_WALK / _STAGGER / SFCVIT_RESERVE_CUS
        auto plan = [](const G &g, const Knobs &k) { return gemm_plan(gemm_args(g), 256, k); };
        const G qkv = {M, 2304, 768, 0, 0, 0, E_BIAS, 1, "", 0, 0, 0}, proj = {M, 768, 768, 0, 0, 0, 0, 1, "", 0, 0, 0};
        const G one_tile = {256, 256, 256, 0, 0, 0, 0, 1, "", 0, 0, 0}, dwo = {768, 768, M, 1, 1, 0, 0, 28, "", 0, 0, 0};
        GemmPlan p = plan(qkv, dflt);
        CHECK(p.walk == 6 && p.stag_slots == 4 && p.stag_ticks == 200, "qkv: walk %d stagger %d,%d", p.walk, p.stag_slots, p.stag_ticks);
        p = plan(proj, dflt);
        CHECK(p.walk == 0 && p.stag_slots == 4 && p.stag_ticks == 200, "out_proj: walk %d stagger %d,%d", p.walk, p.stag_slots, p.stag_ticks);
        p = plan(one_tile, dflt);
        CHECK(p.stag_ticks == 0, "one tile per workgroup: stagger ticks %d", p.stag_ticks);
        Knobs k;
        k.gemm_walk = 0;
        k.gemm_stagger_slots = 0;
        k.gemm_stagger_ticks = 100;
        p = plan(qkv, k);
        CHECK(p.walk == 0 && p.stag_slots == 1 && p.stag_ticks == 100, "WALK=0 STAGGER=0,100: walk %d stagger %d,%d", p.walk, p.stag_slots, p.stag_ticks);
        k = Knobs();
        k.reserve_cus = 16;                                     // 240 CUs / 9 tiles: 26 k-ranges of 32 k-tiles -> 25
        p = plan(dwo, k);
        CHECK(p.splits == 25 && p.k_per_split == 32 && p.grid == 232, "RESERVE_CUS=16: splits %d kps %d grid %d", p.splits, p.k_per_split, p.grid);
        k.reserve_cus = 200;                                    // more than half the CUs: ignored
        p = plan(dwo, k);
        CHECK(p.splits == 28 && p.k_per_split == 28 && p.grid == 256, "RESERVE_CUS=200: splits %d kps %d grid %d", p.splits, p.k_per_split, p.grid);
    }
    {   // null operand: the message the Python test reads
        sfcvit_gemm_args a{};
        const GemmPlan p = gemm_plan(a, 256, dflt);
        CHECK(p.err == SFCVIT_EINVAL && std::strstr(p.msg, "null"), "gemm null operand: %d '%s'", p.err, p.msg);
    }

    // attention: (B, N, H, hd, p, bwd, knobs) -> kernel
    struct A { int B, N, H, hd; float p; bool bwd; int knob; const char *name; Colsum colsum; };
    enum { K_NONE, K_LONG0, K_FUSED0, K_DQPASS, K_PERSIST0 };
    const A attn[] = {
        {256, 196, 12, 64, 0.1f, false, K_NONE, "attn_seq_fwd_kernel<13, true>", Colsum::NONE},            // ViT-B / 256
        {256, 196, 12, 64, 0.f, false, K_NONE, "attn_seq_fwd_kernel<13, false>", Colsum::NONE},
        {256, 196, 12, 64, 0.1f, true, K_NONE, "attn_seq_bwd_fused_kernel<13, true>", Colsum::PARTIALS},
        {64, 196, 12, 64, 0.1f, false, K_NONE, "attn_seq_fwd_kernel<13, true>", Colsum::NONE},              // batch 64
        {64, 196, 12, 64, 0.1f, true, K_NONE, "attn_seq_bwd_fused_kernel<13, true>", Colsum::PARTIALS},
        {256, 196, 12, 64, 0.f, true, K_NONE, "attn_seq_bwd_fused_kernel<13, false>", Colsum::PARTIALS},
        {256, 196, 12, 64, 0.1f, true, K_DQPASS, "attn_seq_bwd_fused_kernel<13, true>", Colsum::PARTIALS_QPASS},
        {256, 196, 12, 64, 0.1f, true, K_FUSED0, "attn_seq_bwd_kv_kernel<13>", Colsum::PASS},
        {64, 576, 16, 64, 0.1f, false, K_NONE, "attn_long_fwd_kernel<36>", Colsum::NONE},                  // ViT-L/16 @ 384
        {64, 576, 16, 64, 0.1f, true, K_NONE, "attn_long_bwd_kv_kernel", Colsum::PARTIALS},
        {64, 577, 16, 64, 0.1f, false, K_NONE, "attn_long_fwd_kernel<0>", Colsum::NONE},
        {64, 576, 16, 64, 0.1f, false, K_LONG0, "attn_fwd_kernel", Colsum::NONE},
        {64, 576, 16, 64, 0.1f, true, K_LONG0, "attn_bwd_kv_kernel", Colsum::PASS},
        {256, 4, 3, 64, 0.1f, false, K_NONE, "attn_seq_fwd_kernel<0, true>", Colsum::NONE},               // ViT-Tiny @ 32
        {256, 4, 3, 64, 0.1f, true, K_NONE, "attn_seq_bwd_fused_kernel<0, true>", Colsum::PARTIALS},
        {8, 240, 4, 64, 0.f, true, K_NONE, "attn_seq_bwd_kv_kernel<0>", Colsum::PASS},                     // 224 < N <= 256
        {8, 1024, 4, 64, 0.f, false, K_NONE, "attn_fwd_kernel", Colsum::NONE},                             // N > 608: tiled
        {8, 1024, 4, 64, 0.f, true, K_NONE, "attn_bwd_kv_kernel", Colsum::PASS},
        {8, 196, 4, 128, 0.f, false, K_NONE, "attn_wide_fwd_kernel<2>", Colsum::NONE},                      // wide head dims
        {8, 196, 4, 128, 0.1f, true, K_NONE, "attn_wide_bwd_kv_kernel<2>", Colsum::PASS},
        {8, 128, 4, 192, 0.f, false, K_NONE, "attn_wide_fwd_kernel<3>", Colsum::NONE},
        {8, 128, 4, 256, 0.f, true, K_NONE, "attn_wide_bwd_kv_kernel<4>", Colsum::PASS},
        {8, 196, 4, 192, 0.f, false, K_NONE, "attention: head dim 192 with N = 196 needs 168 KiB of LDS", Colsum::NONE},
        {8, 196, 4, 256, 0.f, true, K_NONE, "attention: head dim 256 with N = 196 needs 226 KiB of LDS", Colsum::NONE},
        {8, 300, 4, 128, 0.f, false, K_NONE, "attention: head dim 128 with N = 300 needs", Colsum::NONE},
        {8, 196, 4, 96, 0.f, false, K_NONE, "attention_fwd: head dim 96 not supported", Colsum::NONE},
    };
    for (const A &t : attn) {
        sfcvit_attn_args a{};
        a.qkv = ptr(0); a.out = ptr(1); a.lse = static_cast<float *>(ptr(2));
        a.dout = ptr(3); a.dqkv = ptr(4); a.delta = static_cast<float *>(ptr(5));
        a.B = t.B; a.N = t.N; a.H = t.H; a.hd = t.hd; a.dropout_p = t.p;
        if (t.bwd) { a.colsum_out = ptr(6); a.colsum_part = static_cast<float *>(ptr(7)); a.colsum_part_bytes = int64_t(1) << 40; }
        Knobs k;
        k.attn_long = t.knob != K_LONG0;
        k.attn_bwd_fused = t.knob != K_FUSED0;
        k.attn_dq_in_kernel = t.knob != K_DQPASS;
        k.attn_bwd_persist = t.knob != K_PERSIST0;
        const AttnPlan p = t.bwd ? attn_bwd_plan(a, 256, k) : attn_fwd_plan(a, k);
        std::snprintf(what, sizeof(what), "attention %s B %d N %d H %d hd %d", t.bwd ? "bwd" : "fwd", t.B, t.N, t.H, t.hd);
        if (!std::strncmp(t.name, "attention", 9)) {
            CHECK(p.err == SFCVIT_EINVAL && std::strstr(p.msg, t.name), "%s: want error '%s', got %d '%s'", what, t.name, p.err, p.msg);
            continue;
        }
        char name[96];
        kernel_name(p, name, sizeof(name));
        CHECK(p.err == SFCVIT_OK && !std::strcmp(name, t.name), "%s: want %s, got %s (%s)", what, t.name, name, p.msg);
        CHECK(p.colsum == t.colsum, "%s: column-sum mode %d, want %d", what, int(p.colsum), int(t.colsum));
    }
    {   // the one-pass backward's grid, queue and stagger: persistent (one workgroup per CU, items from the counters, no
        // stagger) and one workgroup per item (SFCVIT_ATTN_BWD_PERSIST=0: two slots)
        sfcvit_attn_args a{};
        a.qkv = ptr(0); a.out = ptr(1); a.lse = static_cast<float *>(ptr(2));
        a.dout = ptr(3); a.dqkv = ptr(4); a.delta = static_cast<float *>(ptr(5));
        a.B = 256; a.N = 196; a.H = 12; a.hd = 64; a.dropout_p = 0.1f;
        AttnPlan p = attn_bwd_plan(a, 256, dflt);
        CHECK(p.grid == 256 && p.queue && p.per == 256 && p.ticks == 450 && p.npad == 224 && p.dq_sums == 1,
              "fused bwd: grid %d queue %d per %d ticks %d npad %d", p.grid, p.queue, p.per, p.ticks, p.npad);
        CHECK(p.lds == size_t(224) * FUSED_ROW_BYTES + FUSED_EXTRA + FUSED_POST_BYTES, "fused bwd: lds %zu", p.lds);
        CHECK(p.colsum == Colsum::NONE, "fused bwd without colsum_out: mode %d", int(p.colsum));
        Knobs k;
        k.attn_bwd_persist = false;
        p = attn_bwd_plan(a, 256, k);
        CHECK(p.grid == 3072 && !p.queue && p.per == 128, "fused bwd, PERSIST=0: grid %d queue %d per %d", p.grid, p.queue, p.per);
    }
    check_probe();
}

// sfcvit_attention_mask_blocks (attention_masked.cpp) with heap buffers of exactly N * N floats and nb * nb bytes.
static void check_mask_blocks() {
    const float ninf = -std::numeric_limits<float>::infinity();
    struct W { int N, w, visited, total; };
    const W windows[] = {{4, 1, 1, 1}, {70, 1, 4, 4}, {130, 40, 7, 9}, {196, 32, 10, 16}, {576, 64, 25, 81}, {4096, 0, 64, 4096}};
    for (const W &q : windows) {
        const int N = q.N, nb = (N + 63) / 64;
        std::unique_ptr<float[]> m(new float[size_t(N) * N]);
        std::unique_ptr<uint8_t[]> map(new uint8_t[size_t(nb) * nb]);
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) m[size_t(i) * N + j] = (i - j <= q.w && j - i <= q.w) ? 0.f : ninf;
        CHECK(sfcvit_attention_mask_blocks(m.get(), N, map.get()) == SFCVIT_OK, "mask blocks N %d w %d: %s", N, q.w, sfcvit_last_error());
        int visited = 0;
        for (int i = 0; i < nb * nb; i++) visited += map[i] != 0;
        CHECK(visited == q.visited && nb * nb == q.total, "mask blocks N %d w %d: %d / %d visited, want %d / %d", N, q.w, visited, nb * nb,
              q.visited, q.total);
        // the diagonal block of a window >= 63 wide is all zero (2) when it is a whole block; a partial or narrower one is mixed
        if (N == 576) CHECK(map[0] == 2 && map[1] == 1 && map[2] == 0, "mask blocks N 576: first row %d %d %d", map[0], map[1], map[2]);
        const size_t last = size_t(N) * N - 1;
        m[last] = std::numeric_limits<float>::quiet_NaN();
        CHECK(sfcvit_attention_mask_blocks(m.get(), N, map.get()) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "NaN"), "mask blocks: NaN accepted");
        m[last] = -ninf;
        CHECK(sfcvit_attention_mask_blocks(m.get(), N, map.get()) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "+inf"), "mask blocks: +inf accepted");
        for (int j = 0; j < N; j++) m[size_t(N - 1) * N + j] = ninf;
        char want[32];
        std::snprintf(want, sizeof(want), "row %d ", N - 1);
        CHECK(sfcvit_attention_mask_blocks(m.get(), N, map.get()) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), want),
              "mask blocks: hidden row %d accepted or not named: '%s'", N - 1, sfcvit_last_error());
    }
    float one = 0.f;
    uint8_t b = 0;
    CHECK(sfcvit_attention_mask_blocks(nullptr, 1, &b) == SFCVIT_EINVAL, "mask blocks: null mask accepted");
    CHECK(sfcvit_attention_mask_blocks(&one, 1, nullptr) == SFCVIT_EINVAL, "mask blocks: null map accepted");
    CHECK(sfcvit_attention_mask_blocks(&one, 0, &b) == SFCVIT_EINVAL, "mask blocks: N = 0 accepted");
    CHECK(sfcvit_attention_mask_blocks(&one, 4097, &b) == SFCVIT_EINVAL, "mask blocks: N = 4097 accepted");
    CHECK(sfcvit_attention_mask_blocks(&one, 1, &b) == SFCVIT_OK && b == 2, "mask blocks: N = 1, zero mask: %d", int(b));
}

// sfcvit_attention_bias_blocks / _workspace and attn_bias_check (attention_bias.cpp) with heap buffers of exactly N * N index
// entries, nb * nb map bytes, T + 1 offsets and as many positions as the index has visible entries.
static void check_attention_bias() {
    struct W { int N, w, visited, total; };
    const W windows[] = {{1, 0, 1, 1}, {4, 1, 1, 1}, {70, 1, 4, 4}, {130, 40, 7, 9}, {196, 32, 10, 16}, {576, 64, 25, 81}, {1024, 0, 16, 256}};
    for (const W &q : windows) {
        const int N = q.N, nb = (N + 63) / 64, T = 2 * q.w + 1;
        std::unique_ptr<int32_t[]> idx(new int32_t[size_t(N) * N]);
        std::unique_ptr<uint8_t[]> map(new uint8_t[size_t(nb) * nb]);
        std::unique_ptr<int32_t[]> off(new int32_t[T + 1]);
        int nnz = 0;
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) nnz += (idx[size_t(i) * N + j] = (i - j <= q.w && j - i <= q.w) ? j - i + q.w : -1) >= 0;
        std::unique_ptr<int32_t[]> pos(new int32_t[nnz]);
        CHECK(sfcvit_attention_bias_blocks(idx.get(), N, T, map.get(), off.get(), pos.get()) == SFCVIT_OK, "bias blocks N %d w %d: %s", N, q.w,
              sfcvit_last_error());
        int visited = 0;
        for (int i = 0; i < nb * nb; i++) visited += map[i] != 0;
        CHECK(visited == q.visited && nb * nb == q.total, "bias blocks N %d w %d: %d / %d visited, want %d / %d", N, q.w, visited, nb * nb,
              q.visited, q.total);
        // the inverted index: bucket t holds the pairs with j - i = t - w, ascending, and every visible pair exactly once
        bool ok = off[0] == 0 && off[T] == nnz;
        for (int t = 0; t < T && ok; t++) {
            const int d = t - q.w, want = N - (d < 0 ? -d : d);
            ok = off[t + 1] - off[t] == (want > 0 ? want : 0);
            for (int k = off[t]; k < off[t + 1] && ok; k++) {
                const int i = pos[k] / N, j = pos[k] % N;
                ok = j - i == d && (k == off[t] || pos[k] > pos[k - 1]);
            }
        }
        CHECK(ok, "bias blocks N %d w %d: inverted index wrong", N, q.w);
        const size_t last = size_t(N) * N - 1;
        const int32_t keep = idx[last];
        idx[last] = T;
        CHECK(sfcvit_attention_bias_blocks(idx.get(), N, T, map.get(), off.get(), pos.get()) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "outside"),
              "bias blocks: entry T accepted");
        idx[last] = -2;
        CHECK(sfcvit_attention_bias_blocks(idx.get(), N, T, map.get(), off.get(), pos.get()) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "outside"),
              "bias blocks: entry -2 accepted");
        idx[last] = keep;
        for (int j = 0; j < N; j++) idx[size_t(N - 1) * N + j] = -1;
        char want[32];
        std::snprintf(want, sizeof(want), "row %d ", N - 1);
        CHECK(sfcvit_attention_bias_blocks(idx.get(), N, T, map.get(), off.get(), pos.get()) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), want),
              "bias blocks: hidden row %d accepted or not named: '%s'", N - 1, sfcvit_last_error());
    }
    int32_t one = 0, off2[2] = {0, 0}, pos1 = 0;
    uint8_t b = 0;
    CHECK(sfcvit_attention_bias_blocks(nullptr, 1, 1, &b, off2, &pos1) == SFCVIT_EINVAL, "bias blocks: null index accepted");
    CHECK(sfcvit_attention_bias_blocks(&one, 1, 1, nullptr, off2, &pos1) == SFCVIT_EINVAL, "bias blocks: null map accepted");
    CHECK(sfcvit_attention_bias_blocks(&one, 1, 1, &b, nullptr, &pos1) == SFCVIT_EINVAL, "bias blocks: null offsets accepted");
    CHECK(sfcvit_attention_bias_blocks(&one, 1, 1, &b, off2, nullptr) == SFCVIT_EINVAL, "bias blocks: null positions accepted");
    CHECK(sfcvit_attention_bias_blocks(&one, 0, 1, &b, off2, &pos1) == SFCVIT_EINVAL, "bias blocks: N = 0 accepted");
    CHECK(sfcvit_attention_bias_blocks(&one, 1025, 1, &b, off2, &pos1) == SFCVIT_EINVAL, "bias blocks: N = 1025 accepted");
    CHECK(sfcvit_attention_bias_blocks(&one, 1, 0, &b, off2, &pos1) == SFCVIT_EINVAL, "bias blocks: T = 0 accepted");
    CHECK(sfcvit_attention_bias_blocks(&one, 1, 4097, &b, off2, &pos1) == SFCVIT_EINVAL, "bias blocks: T = 4097 accepted");
    CHECK(sfcvit_attention_bias_blocks(&one, 1, 1, &b, off2, &pos1) == SFCVIT_OK && b == 1 && off2[1] == 1 && pos1 == 0, "bias blocks: N = 1");

    // the workspace: 16 KiB per (chunk, head, visited block); the chunks cover the batch, at most 32, none empty
    for (int B : {1, 2, 3, 40, 64, 256})
        for (int H : {1, 2, 12, 16})
            for (int vb : {1, 4, 10, 25, 81, 256}) {
                const BiasChunks c = bias_chunks(B, H, vb);
                CHECK(c.per >= 1 && c.chunks >= 1 && c.chunks <= 32 && c.per * c.chunks >= B && c.per * (c.chunks - 1) < B,
                      "bias chunks B %d H %d vb %d: per %d chunks %d", B, H, vb, c.per, c.chunks);
                CHECK(sfcvit_attention_bias_workspace(B, 64, H, vb) == int64_t(c.chunks) * H * vb * 16384, "bias workspace B %d H %d vb %d", B, H, vb);
            }
    CHECK(sfcvit_attention_bias_workspace(0, 64, 1, 1) == 0 && sfcvit_attention_bias_workspace(1, 1025, 1, 1) == 0, "bias workspace: bad shape");

    // the entry points' checks: fake aligned pointers, nothing is dereferenced
    sfcvit_attn_bias_args a{};
    a.qkv = ptr(0); a.out = ptr(1); a.lse = static_cast<float *>(ptr(2)); a.dout = ptr(3); a.dqkv = ptr(4); a.delta = static_cast<float *>(ptr(5));
    a.B = 2; a.N = 130; a.H = 2; a.hd = 64; a.scale = 0.125f;
    a.block_map = static_cast<const uint8_t *>(ptr(6)); a.index = static_cast<const int32_t *>(ptr(7)); a.table = static_cast<const float *>(ptr(8));
    a.T = 81; a.visited_blocks = 7; a.offsets = static_cast<const int32_t *>(ptr(9)); a.positions = static_cast<const int32_t *>(ptr(10));
    a.dtable = static_cast<float *>(ptr(11)); a.workspace = ptr(12); a.workspace_bytes = sfcvit_attention_bias_workspace(2, 130, 2, 7);
    CHECK(attn_bias_check(&a, false, "t") == SFCVIT_OK && attn_bias_check(&a, true, "t") == SFCVIT_OK, "bias check: good arguments refused: %s", sfcvit_last_error());
    auto refused = [&](auto &&change, bool bwd, const char *word) {
        sfcvit_attn_bias_args c = a;
        change(c);
        CHECK(attn_bias_check(&c, bwd, "t") == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), word), "bias check: '%s' not refused: '%s'", word,
              sfcvit_last_error());
    };
    CHECK(attn_bias_check(nullptr, false, "t") == SFCVIT_EINVAL, "bias check: null arguments accepted");
    refused([](sfcvit_attn_bias_args &c) { c.qkv = nullptr; }, false, "qkv / out / lse");
    refused([](sfcvit_attn_bias_args &c) { c.dout = nullptr; }, true, "dout / dqkv / delta");
    refused([](sfcvit_attn_bias_args &c) { c.index = nullptr; }, false, "index / table / block_map");
    refused([](sfcvit_attn_bias_args &c) { c.table = nullptr; }, false, "index / table / block_map");
    refused([](sfcvit_attn_bias_args &c) { c.offsets = nullptr; }, true, "offsets / positions");
    {   // dtable == NULL is a frozen table: nothing of the table gradient is asked for
        sfcvit_attn_bias_args c = a;
        c.dtable = nullptr; c.offsets = nullptr; c.positions = nullptr; c.workspace = nullptr; c.workspace_bytes = 0; c.visited_blocks = 0;
        CHECK(attn_bias_check(&c, true, "t") == SFCVIT_OK, "bias check: frozen table refused: %s", sfcvit_last_error());
    }
    refused([](sfcvit_attn_bias_args &c) { c.hd = 128; }, false, "head dim 128");
    refused([](sfcvit_attn_bias_args &c) { c.dropout_p = 1.f; }, false, "dropout_p");
    refused([](sfcvit_attn_bias_args &c) { c.B = 0; }, false, "B=0");
    refused([](sfcvit_attn_bias_args &c) { c.N = 1025; }, false, "N=1025");
    refused([](sfcvit_attn_bias_args &c) { c.T = 0; }, false, "T=0");
    refused([](sfcvit_attn_bias_args &c) { c.T = 4097; }, false, "T=4097");
    refused([](sfcvit_attn_bias_args &c) { c.qkv = static_cast<const char *>(c.qkv) + 2; }, false, "16-byte aligned");
    refused([](sfcvit_attn_bias_args &c) { c.index = c.index + 1; }, false, "index must be 16-byte aligned");
    refused([](sfcvit_attn_bias_args &c) { c.visited_blocks = 0; }, true, "visited_blocks=0");
    refused([](sfcvit_attn_bias_args &c) { c.visited_blocks = 10; }, true, "visited_blocks=10");
    refused([](sfcvit_attn_bias_args &c) { c.workspace = nullptr; }, true, "workspace");
    refused([](sfcvit_attn_bias_args &c) { c.workspace_bytes -= 1; }, true, "workspace");
}

// pos_embed_plan / pos_embed_check_* (pos_embed.cpp): the geometry at the workload shapes and the edge shapes of the tests, and
// every refusal, with heap buffers of exactly B N D bf16 (x, y, dy), N D bf16 (pos), N D fp32 (dpos) and the workspace the plan
// names.  The checks read no byte of them; what is pinned is that every accepted geometry stays inside them.
static void check_pos_embed() {
    struct S { int B, N, D; };
    const S shapes[] = {{1, 1, 8}, {2, 1, 8}, {3, 5, 72}, {2, 65, 200}, {67, 3, 8}, {5, 4, 192}, {2, 197, 768}, {2, 196, 1024},
                        {256, 196, 768}, {64, 576, 1024}, {4096, 1, 8}, {100000, 2, 8}};
    for (const S &q : shapes) {
        const PosEmbedPlan p = pos_embed_plan("host_check", q.B, q.N, q.D);
        CHECK(p.err == SFCVIT_OK, "pos_embed %d %d %d refused: %s", q.B, q.N, q.D, p.msg);
        if (p.err) continue;
        const int64_t nd = int64_t(q.N) * q.D, total = nd * q.B;
        CHECK(p.vecs * 8 == nd, "pos_embed: vecs");
        // forward: every table vector has a lane, every image a group, a lane's images end inside the batch or are clamped
        CHECK(int64_t(p.fwd_blocks) * PE_THREADS >= p.vecs && int64_t(p.fwd_blocks - 1) * PE_THREADS < p.vecs, "pos_embed fwd blocks");
        CHECK(p.imgs >= 1 && p.imgs <= PE_MAX_IMGS && int64_t(p.fwd_groups) * p.imgs >= q.B && int64_t(p.fwd_groups - 1) * p.imgs < q.B,
              "pos_embed fwd groups %d x %d for B %d", p.fwd_groups, p.imgs, q.B);
        CHECK(p.fwd_groups <= 65535, "pos_embed fwd grid.y");
        // backward: slabs cover the table, ranges cover the batch, no range is empty, rows are whole rounds of the 8 image lanes
        CHECK(int64_t(p.slabs) * PE_CV >= p.vecs && int64_t(p.slabs - 1) * PE_CV < p.vecs, "pos_embed bwd slabs");
        CHECK(p.rows % PE_RL == 0 && int64_t(p.splits) * p.rows >= q.B && int64_t(p.splits - 1) * p.rows < q.B && p.splits <= 65535,
              "pos_embed bwd ranges %d x %d for B %d", p.splits, p.rows, q.B);
        CHECK(p.ws_bytes == (p.splits > 1 ? int64_t(p.splits) * nd * 4 : 0), "pos_embed workspace %lld", (long long)p.ws_bytes);
        CHECK(p.splits == 1 || nd <= INT32_MAX, "pos_embed: a split table beyond the column reduction's int");
        CHECK(sfcvit_pos_embed_bwd_workspace(q.B, q.N, q.D) == p.ws_bytes, "pos_embed workspace entry point");
        if (total > (int64_t(1) << 24)) continue;              // the workload shapes: geometry only
        void *x = std::aligned_alloc(16, size_t((total * 2 + 15) / 16 * 16)), *pos = std::aligned_alloc(16, size_t((nd * 2 + 15) / 16 * 16));
        std::unique_ptr<float[]> dpos(new float[size_t(nd)]);
        void *ws = p.ws_bytes ? std::aligned_alloc(16, size_t(p.ws_bytes)) : nullptr;
        CHECK(pos_embed_check_fwd(p, x, pos, x) == SFCVIT_OK, "pos_embed fwd check: %s", sfcvit_last_error());
        CHECK(pos_embed_check_bwd(p, x, dpos.get(), ws, p.ws_bytes) == SFCVIT_OK, "pos_embed bwd check: %s", sfcvit_last_error());
        CHECK(pos_embed_check_bwd(p, x, reinterpret_cast<char *>(dpos.get()) + 2, ws, p.ws_bytes) == SFCVIT_OK, "pos_embed: dpos needs no alignment");
        CHECK(pos_embed_check_fwd(p, nullptr, pos, x) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "null"), "pos_embed: null x accepted");
        CHECK(pos_embed_check_fwd(p, x, nullptr, x) == SFCVIT_EINVAL, "pos_embed: null pos accepted");
        CHECK(pos_embed_check_fwd(p, x, pos, nullptr) == SFCVIT_EINVAL, "pos_embed: null y accepted");
        CHECK(pos_embed_check_fwd(p, static_cast<char *>(x) + 2, pos, x) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "aligned"),
              "pos_embed: misaligned x accepted");
        CHECK(pos_embed_check_bwd(p, nullptr, dpos.get(), ws, p.ws_bytes) == SFCVIT_EINVAL, "pos_embed: null dy accepted");
        CHECK(pos_embed_check_bwd(p, x, nullptr, ws, p.ws_bytes) == SFCVIT_EINVAL, "pos_embed: null dpos accepted");
        CHECK(pos_embed_check_bwd(p, static_cast<char *>(x) + 8, dpos.get(), ws, p.ws_bytes) == SFCVIT_EINVAL, "pos_embed: misaligned dy accepted");
        if (p.ws_bytes) {
            CHECK(pos_embed_check_bwd(p, x, dpos.get(), ws, p.ws_bytes - 1) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "workspace"),
                  "pos_embed: short workspace accepted");
            CHECK(pos_embed_check_bwd(p, x, dpos.get(), nullptr, p.ws_bytes) == SFCVIT_EINVAL, "pos_embed: null workspace accepted");
            CHECK(pos_embed_check_bwd(p, x, dpos.get(), static_cast<char *>(ws) + 4, p.ws_bytes) == SFCVIT_EINVAL, "pos_embed: misaligned workspace accepted");
        }
        std::free(x);
        std::free(pos);
        std::free(ws);
    }
    const PosEmbedPlan b = pos_embed_plan("host_check", 256, 196, 768), l = pos_embed_plan("host_check", 64, 576, 1024);
    CHECK(b.splits == 1 && b.slabs == 588 && b.imgs == 8 && b.fwd_blocks * b.fwd_groups == 74 * 32, "pos_embed ViT-B geometry");
    CHECK(l.splits == 1 && l.slabs == 2304 && l.imgs == 8 && l.fwd_blocks * l.fwd_groups == 288 * 8, "pos_embed ViT-L geometry");
    CHECK(pos_embed_plan("host_check", 67, 3, 8).splits == 2, "pos_embed: (67, 3, 8) must split the batch");
    const S bad[] = {{0, 1, 8}, {1, 0, 8}, {-1, 1, 8}, {1, 1, 0}, {1, 1, 4}, {1, 1, 12}, {1, 1, -8}, {INT32_MAX, INT32_MAX, INT32_MAX - 7},
                     {INT32_MAX, 1, 8}};
    for (const S &q : bad) {
        const PosEmbedPlan p = pos_embed_plan("host_check", q.B, q.N, q.D);
        CHECK(p.err == SFCVIT_EINVAL && std::strlen(p.msg) > 0, "pos_embed %d %d %d accepted", q.B, q.N, q.D);
        CHECK(sfcvit_pos_embed_bwd_workspace(q.B, q.N, q.D) == 0, "pos_embed: workspace of a refused shape");
    }
    char name[96];
    CHECK(sfcvit_last_pos_embed_kernel(name, sizeof(name)) == SFCVIT_OK && !std::strcmp(name, "none"), "pos_embed: last kernel '%s'", name);
    CHECK(sfcvit_last_pos_embed_kernel(nullptr, 4) == SFCVIT_EINVAL, "pos_embed: null name buffer accepted");
}

// cls_prepend_plan / token_pool_plan and their pointer checks (token_pool.cpp): the geometry at the workload shapes and the
// edge shapes of the tests, and every refusal, with heap buffers of exactly the documented sizes.  The checks read no byte
// of them; what is pinned is that every accepted geometry stays inside them.
static void check_token_pool() {
    struct S { int B, N, D; };
    const S shapes[] = {{1, 1, 8}, {2, 1, 8}, {3, 5, 72}, {2, 65, 200}, {67, 3, 8}, {5, 4, 192}, {2, 196, 768}, {2, 576, 1024},
                        {256, 196, 768}, {64, 576, 1024}, {4096, 1, 8}, {100000, 2, 8}};
    for (const S &q : shapes) {
        const ClsPrependPlan p = cls_prepend_plan("host_check", q.B, q.N, q.D);
        CHECK(p.err == SFCVIT_OK, "cls_prepend %d %d %d refused: %s", q.B, q.N, q.D, p.msg);
        if (p.err) continue;
        const int64_t xn = int64_t(q.B) * q.N * q.D, yn = int64_t(q.B) * (q.N + 1) * q.D;
        CHECK(p.dv * 8 == q.D && p.xv == int64_t(q.N) * p.dv, "cls_prepend: vectors");
        CHECK(int64_t(p.fwd_blocks) * TP_THREADS >= p.xv + p.dv && int64_t(p.fwd_blocks - 1) * TP_THREADS < p.xv + p.dv, "cls_prepend fwd blocks");
        CHECK(int64_t(p.bwd_blocks) * TP_THREADS >= p.xv && int64_t(p.bwd_blocks - 1) * TP_THREADS < p.xv, "cls_prepend bwd blocks");
        CHECK((p.imgs == 1 || p.imgs == 2 || p.imgs == 4 || p.imgs == 8) && int64_t(p.groups) * p.imgs >= q.B &&
              int64_t(p.groups - 1) * p.imgs < q.B && p.groups <= 65535, "cls_prepend groups %d x %d for B %d", p.groups, p.imgs, q.B);
        CHECK(int64_t(p.slabs) * CP_CV >= p.dv && int64_t(p.slabs - 1) * CP_CV < p.dv, "cls_prepend dcls slabs");
        CHECK(p.rows % CP_RL == 0 && p.rows <= CP_MAX_ROWS && int64_t(p.splits) * p.rows >= q.B && int64_t(p.splits - 1) * p.rows < q.B &&
              p.splits <= 65535, "cls_prepend dcls ranges %d x %d for B %d", p.splits, p.rows, q.B);
        CHECK(p.ws_bytes == (p.splits > 1 ? int64_t(p.splits) * q.D * 4 : 0), "cls_prepend workspace %lld", (long long)p.ws_bytes);
        CHECK(sfcvit_cls_prepend_bwd_workspace(q.B, q.N, q.D) == p.ws_bytes, "cls_prepend workspace entry point");
        // pool: every (first, count) of the tests
        const int T = q.N + 1;
        const int fc[][2] = {{0, 1}, {0, T}, {1, T - 1}, {T - 1, 1}};
        for (const auto &r : fc) {
            if (r[1] < 1) continue;
            const TokenPoolPlan t = token_pool_plan("host_check", q.B, T, q.D, r[0], r[1]);
            CHECK(t.err == SFCVIT_OK, "token_pool %d %d %d [%d, +%d) refused: %s", q.B, T, q.D, r[0], r[1], t.msg);
            CHECK((t.cv == 8 || t.cv == 16 || t.cv == 32) && t.cv * t.tl == TP_THREADS && t.dv * 8 == q.D, "token_pool lanes %d x %d", t.cv, t.tl);
            CHECK(int64_t(t.slabs) * t.cv >= t.dv && int64_t(t.slabs - 1) * t.cv < t.dv && t.slabs <= 65535, "token_pool slabs");
            CHECK(int64_t(t.row_blocks) * TP_THREADS >= t.dv && int64_t(t.row_blocks - 1) * TP_THREADS < t.dv, "token_pool row blocks");
            CHECK(t.row_copy == (r[1] == 1), "token_pool: count == 1 is the row copy");
        }
        if (yn > (int64_t(1) << 24)) continue;                 // the workload shapes: geometry only
        void *x = std::aligned_alloc(16, size_t((xn * 2 + 15) / 16 * 16)), *y = std::aligned_alloc(16, size_t((yn * 2 + 15) / 16 * 16));
        void *cls = std::aligned_alloc(16, size_t(q.D) * 2);
        std::unique_ptr<float[]> dcls(new float[size_t(q.D)]);
        void *ws = p.ws_bytes ? std::aligned_alloc(16, size_t(p.ws_bytes)) : nullptr;
        CHECK(cls_prepend_check_fwd(p, x, cls, y, q.B, q.N, q.D) == SFCVIT_OK, "cls_prepend fwd check: %s", sfcvit_last_error());
        CHECK(cls_prepend_check_bwd(p, y, x, dcls.get(), ws, p.ws_bytes) == SFCVIT_OK, "cls_prepend bwd check: %s", sfcvit_last_error());
        CHECK(cls_prepend_check_bwd(p, y, nullptr, dcls.get(), ws, p.ws_bytes) == SFCVIT_OK, "cls_prepend: dx may be null");
        CHECK(cls_prepend_check_bwd(p, y, x, reinterpret_cast<char *>(dcls.get()) + 2, ws, p.ws_bytes) == SFCVIT_OK, "cls_prepend: dcls needs no alignment");
        CHECK(cls_prepend_check_fwd(p, nullptr, cls, y, q.B, q.N, q.D) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "null"), "cls_prepend: null x accepted");
        CHECK(cls_prepend_check_fwd(p, x, nullptr, y, q.B, q.N, q.D) == SFCVIT_EINVAL, "cls_prepend: null cls accepted");
        CHECK(cls_prepend_check_fwd(p, x, cls, nullptr, q.B, q.N, q.D) == SFCVIT_EINVAL, "cls_prepend: null y accepted");
        CHECK(cls_prepend_check_fwd(p, static_cast<char *>(x) + 2, cls, y, q.B, q.N, q.D) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "aligned"),
              "cls_prepend: misaligned x accepted");
        CHECK(cls_prepend_check_fwd(p, y, cls, y, q.B, q.N, q.D) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "overlaps"), "cls_prepend: y == x accepted");
        CHECK(cls_prepend_check_fwd(p, static_cast<char *>(y) + 16, cls, y, q.B, q.N, q.D) == SFCVIT_EINVAL, "cls_prepend: x inside y accepted");
        CHECK(cls_prepend_check_bwd(p, nullptr, x, dcls.get(), ws, p.ws_bytes) == SFCVIT_EINVAL, "cls_prepend: null dy accepted");
        CHECK(cls_prepend_check_bwd(p, y, x, nullptr, ws, p.ws_bytes) == SFCVIT_EINVAL, "cls_prepend: null dcls accepted");
        CHECK(cls_prepend_check_bwd(p, static_cast<char *>(y) + 8, x, dcls.get(), ws, p.ws_bytes) == SFCVIT_EINVAL, "cls_prepend: misaligned dy accepted");
        CHECK(cls_prepend_check_bwd(p, y, static_cast<char *>(x) + 8, dcls.get(), ws, p.ws_bytes) == SFCVIT_EINVAL, "cls_prepend: misaligned dx accepted");
        if (p.ws_bytes) {
            CHECK(cls_prepend_check_bwd(p, y, x, dcls.get(), ws, p.ws_bytes - 1) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "workspace"),
                  "cls_prepend: short workspace accepted");
            CHECK(cls_prepend_check_bwd(p, y, x, dcls.get(), nullptr, p.ws_bytes) == SFCVIT_EINVAL, "cls_prepend: null workspace accepted");
            CHECK(cls_prepend_check_bwd(p, y, x, dcls.get(), static_cast<char *>(ws) + 4, p.ws_bytes) == SFCVIT_EINVAL, "cls_prepend: misaligned workspace accepted");
        }
        const TokenPoolPlan t = token_pool_plan("host_check", q.B, T, q.D, 0, T);
        CHECK(token_pool_check(t, "token_pool_fwd", y, x) == SFCVIT_OK, "token_pool check: %s", sfcvit_last_error());
        CHECK(token_pool_check(t, "token_pool_fwd", nullptr, x) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "null"), "token_pool: null x accepted");
        CHECK(token_pool_check(t, "token_pool_bwd", y, nullptr) == SFCVIT_EINVAL, "token_pool: null dx accepted");
        CHECK(token_pool_check(t, "token_pool_fwd", static_cast<char *>(y) + 2, x) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "aligned"),
              "token_pool: misaligned x accepted");
        std::free(x);
        std::free(y);
        std::free(cls);
        std::free(ws);
    }
    const ClsPrependPlan b = cls_prepend_plan("host_check", 256, 196, 768), l = cls_prepend_plan("host_check", 64, 576, 1024);
    CHECK(b.splits == 1 && b.slabs == 12 && b.imgs == 8 && b.fwd_blocks == 74 && b.groups == 32 && b.ws_bytes == 0, "cls_prepend ViT-B geometry");
    CHECK(l.splits == 1 && l.slabs == 16 && l.imgs == 8 && l.fwd_blocks == 289 && l.groups == 8 && l.ws_bytes == 0, "cls_prepend ViT-L geometry");
    CHECK(cls_prepend_plan("host_check", 4096, 1, 8).splits == 2 && cls_prepend_plan("host_check", 2049, 1, 8).splits == 2 &&
          cls_prepend_plan("host_check", 2048, 1, 8).splits == 1, "cls_prepend: the batch splits above 2048 images");
    const TokenPoolPlan tb = token_pool_plan("host_check", 256, 197, 768, 1, 196), tl = token_pool_plan("host_check", 64, 577, 1024, 1, 576);
    CHECK(tb.cv == 16 && tb.tl == 16 && tb.slabs == 6, "token_pool ViT-B geometry %d x %d, %d slabs", tb.cv, tb.tl, tb.slabs);
    CHECK(tl.cv == 8 && tl.tl == 32 && tl.slabs == 16, "token_pool ViT-L geometry %d x %d, %d slabs", tl.cv, tl.tl, tl.slabs);
    const S bad[] = {{0, 1, 8}, {1, 0, 8}, {-1, 1, 8}, {1, 1, 0}, {1, 1, 4}, {1, 1, 12}, {1, 1, -8}, {INT32_MAX, INT32_MAX, INT32_MAX - 7},
                     {INT32_MAX, 1, 8}};
    for (const S &q : bad) {
        const ClsPrependPlan p = cls_prepend_plan("host_check", q.B, q.N, q.D);
        CHECK(p.err == SFCVIT_EINVAL && std::strlen(p.msg) > 0, "cls_prepend %d %d %d accepted", q.B, q.N, q.D);
        CHECK(sfcvit_cls_prepend_bwd_workspace(q.B, q.N, q.D) == 0, "cls_prepend: workspace of a refused shape");
        if (q.B == INT32_MAX && q.N == 1) continue;            // (the pool puts the batch on grid.x: accepted)
        const TokenPoolPlan t = token_pool_plan("host_check", q.B, q.N, q.D, 0, 1);
        CHECK(t.err == SFCVIT_EINVAL && std::strlen(t.msg) > 0, "token_pool %d %d %d accepted", q.B, q.N, q.D);
    }
    const int badr[][2] = {{-1, 1}, {0, 0}, {0, -1}, {0, 6}, {5, 1}, {3, 3}, {INT32_MAX, INT32_MAX}};
    for (const auto &r : badr) {
        const TokenPoolPlan t = token_pool_plan("host_check", 2, 5, 8, r[0], r[1]);
        CHECK(t.err == SFCVIT_EINVAL && std::strstr(t.msg, "range"), "token_pool: tokens [%d, +%d) of 5 accepted", r[0], r[1]);
    }
    char name[96];
    CHECK(sfcvit_last_token_pool_kernel(name, sizeof(name)) == SFCVIT_OK && !std::strcmp(name, "none"), "token_pool: last kernel '%s'", name);
    CHECK(sfcvit_last_token_pool_kernel(nullptr, 4) == SFCVIT_EINVAL, "token_pool: null name buffer accepted");
    CHECK(sfcvit_last_tokenizer_kernel(name, sizeof(name)) == SFCVIT_OK && !std::strcmp(name, "none") &&
          sfcvit_last_tokenizer_kernel(nullptr, 4) == SFCVIT_EINVAL && sfcvit_last_tokenizer_kernel(name, 0) == SFCVIT_EINVAL, "tokenizer: last kernel '%s'", name);
}

// dwconv_plan and its pointer checks (token_agg.cpp): every bound of the envelope one step inside and one step outside, the
// geometry against a brute-force count of the window positions, and the pointer rules with heap buffers of exactly the
// documented sizes (the checks read no byte of them).
static void check_dwconv() {
    const auto plan = [](int B, int N, int D, int k, int s) { return dwconv_plan("host_check", B, N, D, k, s); };
    const auto refused = [&](int B, int N, int D, int k, int s, const char *why) {
        const DwconvPlan p = plan(B, N, D, k, s);
        CHECK(p.err == SFCVIT_EINVAL && std::strstr(p.msg, why), "dwconv B=%d N=%d D=%d k=%d s=%d: '%s' lacks '%s'", B, N, D, k, s, p.msg, why);
        CHECK(sfcvit_dwconv1d_bwd_workspace(B, N, D, k, s) == 0, "dwconv: workspace of a refused shape");
    };
    const auto accepted = [&](int B, int N, int D, int k, int s) {
        const DwconvPlan p = plan(B, N, D, k, s);
        CHECK(p.err == SFCVIT_OK, "dwconv B=%d N=%d D=%d k=%d s=%d refused: %s", B, N, D, k, s, p.msg);
        return p;
    };
    for (int k : {1, 3, DWC_MAX_K}) accepted(2, 5, 16, k, 1);
    for (int k : {0, DWC_MAX_K + 1, -1, INT32_MAX}) refused(2, 5, 16, k, 1, "kernel size");
    for (int s : {1, DWC_MAX_S}) accepted(2, 5, 16, 3, s);
    for (int s : {0, DWC_MAX_S + 1, -1, INT32_MAX}) refused(2, 5, 16, 3, s, "stride");
    accepted(2, 5, 8, 3, 1);
    for (int D : {0, 12, -8, INT32_MAX}) refused(2, 5, D, 3, 1, "multiple of 8");
    for (int k : {1, 3, DWC_MAX_K}) {                              // ld = D (k + 1) is an int
        const int dmax = INT32_MAX / (k + 1) / 8 * 8;
        const DwconvPlan p = accepted(1, 1, dmax, k, 1);
        CHECK(p.ld == int64_t(dmax) * (k + 1) && p.ws_bytes == int64_t(p.ld) * 4 && int64_t(p.slabs) * DWC_CV * 8 >= dmax, "dwconv: widest D, k=%d", k);
        refused(1, 1, dmax + 8, k, 1, "too wide");
        refused(1, 1, INT32_MAX / 8 * 8, k, 1, "too wide");        // D + 255 leaves int: the slab count must not
    }
    accepted(1, 5, 16, 3, 1);
    accepted(65535, 5, 16, 3, 1);
    for (int B : {0, 65536, -1, INT32_MAX}) refused(B, 5, 16, 3, 1, "B=");
    for (int N : {0, -1}) refused(2, N, 16, 3, 1, "B=");
    for (int k : {2, 3}) {                                          // the longest sequence: 65535 workgroups of 8 x 32 rows
        const int nmax = 65535 * DWC_RL * DWC_MAX_RUN - (k % 2 ? 0 : 1);   // an even k makes Nout = N + 1 rows
        for (int N : {1, 2, nmax}) {
            const DwconvPlan p = accepted(1, N, 8, k, 1);
            CHECK(p.groups == (N == nmax ? 65535 : 1) && p.run_out <= DWC_MAX_RUN && p.run_in <= DWC_MAX_RUN, "dwconv N=%d k=%d: groups %d", N, k, p.groups);
        }
        refused(1, nmax + 1, 8, k, 1, "launch grid");
    }
    refused(1, INT32_MAX / 2 - 2 * DWC_MAX_K, 8, 3, 1, "launch grid");
    refused(1, INT32_MAX / 2 - 2 * DWC_MAX_K + 1, 8, 3, 1, "too long");
    refused(1, INT32_MAX, 8, 3, 1, "too long");
    // B x groups is grid.z x grid.y and one int in the reduction: 65535 x 32768 fits, 65535 x 32769 does not
    CHECK(accepted(65535, 32768 * DWC_RL * DWC_MAX_RUN, 8, 3, 1).ws_bytes == int64_t(65535) * 32768 * 32 * 4, "dwconv: largest B x groups");
    refused(65535, 32768 * DWC_RL * DWC_MAX_RUN + 1, 8, 3, 1, "launch grid");
    refused(65535, 65535 * DWC_RL * DWC_MAX_RUN, 8, 3, 1, "launch grid");
    refused(65535, 32768 * DWC_RL * DWC_MAX_RUN, INT32_MAX / 4 / 8 * 8, 3, 1, "int64");   // every extent at its bound: 2^64 bytes

    for (int N = 1; N <= 40; N++)
        for (int k = 1; k <= DWC_MAX_K; k++)
            for (int s = 1; s <= DWC_MAX_S; s++) {
                const int B = 3, D = 24;
                const DwconvPlan p = accepted(B, N, D, k, s);
                int count = 0;                                     // windows [n s - pad, n s - pad + k) inside the padded sequence
                while (count * s + k <= N + 2 * (k / 2)) count++;
                CHECK(p.pad == k / 2 && p.Nout == count, "dwconv N=%d k=%d s=%d: Nout %d, counted %d", N, k, s, p.Nout, count);
                CHECK(p.groups >= 1 && p.groups * DWC_RL * p.run_out >= p.Nout && p.groups * DWC_RL * p.run_in >= N, "dwconv N=%d k=%d s=%d: runs", N, k, s);
                CHECK(p.run_out <= DWC_MAX_RUN && p.run_in <= DWC_MAX_RUN && p.slabs == 1 && p.spec == (k == 3 && s == 1), "dwconv N=%d k=%d s=%d: geometry", N, k, s);
                CHECK(p.ld == D * (k + 1) && p.ws_bytes == int64_t(B) * p.groups * p.ld * 4, "dwconv N=%d k=%d s=%d: workspace", N, k, s);
                CHECK(sfcvit_dwconv1d_out_len(N, k, s) == p.Nout && sfcvit_dwconv1d_bwd_workspace(B, N, D, k, s) == p.ws_bytes, "dwconv N=%d k=%d s=%d: entry points", N, k, s);
            }
    CHECK(sfcvit_dwconv1d_out_len(5, 0, 1) == -1 && std::strstr(sfcvit_last_error(), "kernel size"), "dwconv: out_len of a refused k");

    const int B = 2, N = 5, D = 16, k = 3;
    const DwconvPlan p = accepted(B, N, D, k, 2);
    const size_t xb = size_t(B) * N * D * 2, ub = size_t(B) * p.Nout * D * 2;
    void *x = std::aligned_alloc(16, xb), *dx = std::aligned_alloc(16, xb), *u = std::aligned_alloc(16, ub), *ws = std::aligned_alloc(16, size_t(p.ws_bytes));
    std::unique_ptr<uint16_t[]> w(new uint16_t[D * k]);
    std::unique_ptr<float[]> dw(new float[D * k]), db(new float[D]);
    char *const u2 = static_cast<char *>(u) + 2;
    CHECK(dwconv_check_fwd(p, x, w.get(), u) == SFCVIT_OK, "dwconv fwd check: %s", sfcvit_last_error());
    CHECK(dwconv_check_fwd(p, nullptr, w.get(), u) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "null"), "dwconv: null x accepted");
    CHECK(dwconv_check_fwd(p, x, nullptr, u) == SFCVIT_EINVAL && dwconv_check_fwd(p, x, w.get(), nullptr) == SFCVIT_EINVAL, "dwconv: null w / u accepted");
    CHECK(dwconv_check_fwd(p, x, w.get(), u2) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "aligned"), "dwconv: misaligned u accepted");
    CHECK(dwconv_check_fwd(plan(B, N, 12, k, 2), x, w.get(), u) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "D=12"), "dwconv: the plan's refusal is the call's");
    CHECK(dwconv_check_bwd(p, u, x, w.get(), dx, dw.get(), db.get(), ws, p.ws_bytes) == SFCVIT_OK, "dwconv bwd check: %s", sfcvit_last_error());
    CHECK(dwconv_check_bwd(p, u, nullptr, w.get(), dx, nullptr, nullptr, nullptr, 0) == SFCVIT_OK, "dwconv: dx alone needs neither x nor a workspace");
    CHECK(dwconv_check_bwd(p, u, nullptr, nullptr, nullptr, nullptr, db.get(), ws, p.ws_bytes) == SFCVIT_OK, "dwconv: db alone needs neither x nor w");
    CHECK(dwconv_check_bwd(p, nullptr, x, w.get(), dx, dw.get(), db.get(), ws, p.ws_bytes) == SFCVIT_EINVAL, "dwconv: null du accepted");
    CHECK(dwconv_check_bwd(p, u, x, w.get(), nullptr, nullptr, nullptr, ws, p.ws_bytes) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "nothing to compute"),
          "dwconv: no output accepted");
    CHECK(dwconv_check_bwd(p, u, x, nullptr, dx, nullptr, nullptr, ws, p.ws_bytes) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "needed for dx"),
          "dwconv: dx without w accepted");
    CHECK(dwconv_check_bwd(p, u, nullptr, w.get(), nullptr, dw.get(), nullptr, ws, p.ws_bytes) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "needed for dw"),
          "dwconv: dw without x accepted");
    CHECK(dwconv_check_bwd(p, u, x, w.get(), dx, dw.get(), db.get(), ws, p.ws_bytes - 1) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "workspace of"),
          "dwconv: short workspace accepted");
    CHECK(dwconv_check_bwd(p, u, x, w.get(), dx, dw.get(), db.get(), nullptr, p.ws_bytes) == SFCVIT_EINVAL, "dwconv: null workspace accepted");
    CHECK(dwconv_check_bwd(p, u2, x, w.get(), dx, dw.get(), db.get(), ws, p.ws_bytes) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "aligned"),
          "dwconv: misaligned du accepted");
    CHECK(dwconv_check_bwd(p, u, x, w.get(), dx, dw.get(), db.get(), static_cast<char *>(ws) + 4, p.ws_bytes) == SFCVIT_EINVAL, "dwconv: misaligned workspace accepted");
    std::free(x);
    std::free(dx);
    std::free(u);
    std::free(ws);
    char name[96];
    CHECK(sfcvit_last_dwconv_kernel(name, sizeof(name)) == SFCVIT_OK && !std::strcmp(name, "none"), "dwconv: last kernel '%s'", name);
    CHECK(sfcvit_last_dwconv_kernel(nullptr, 4) == SFCVIT_EINVAL && sfcvit_last_dwconv_kernel(name, 0) == SFCVIT_EINVAL, "dwconv: null / empty name buffer accepted");
}

// tokmix_left_plan, tokmix_wgrad_plan and tokmix_check_wgrad (token_mix.cpp): the shared envelope with its three int guards
// one step inside and outside, the weight loader's vector width, the image ranges of wgrad, and the pointer rules.
static void check_tokmix() {
    const auto args = [](int B, int M, int K, int D) {
        sfcvit_tokmix_args a{};
        a.w = ptr(0); a.x = ptr(1); a.c = ptr(2);
        a.B = B; a.M = M; a.K = K; a.D = D;
        return a;
    };
    // both plans share the envelope: a shape is accepted or refused by both, with the same reason
    const auto refused = [&](int B, int M, int K, int D, const char *why) {
        const sfcvit_tokmix_args a = args(B, M, K, D);
        const TokmixPlan l = tokmix_left_plan(&a), g = tokmix_wgrad_plan("host_check", B, M, K, D);
        CHECK(l.err == SFCVIT_EINVAL && std::strstr(l.msg, why), "tokmix_left B=%d M=%d K=%d D=%d: '%s' lacks '%s'", B, M, K, D, l.msg, why);
        CHECK(g.err == SFCVIT_EINVAL && std::strstr(g.msg, why), "tokmix_wgrad B=%d M=%d K=%d D=%d: '%s' lacks '%s'", B, M, K, D, g.msg, why);
        CHECK(sfcvit_tokmix_wgrad_workspace(B, M, K, D) == 0, "tokmix: workspace of a refused shape");
    };
    const auto accepted = [&](int B, int M, int K, int D) {
        const sfcvit_tokmix_args a = args(B, M, K, D);
        const TokmixPlan l = tokmix_left_plan(&a), g = tokmix_wgrad_plan("host_check", B, M, K, D);
        CHECK(l.err == SFCVIT_OK, "tokmix_left B=%d M=%d K=%d D=%d refused: %s", B, M, K, D, l.msg);
        CHECK(g.err == SFCVIT_OK, "tokmix_wgrad B=%d M=%d K=%d D=%d refused: %s", B, M, K, D, g.msg);
        if (l.err || g.err) return g;
        CHECK(int64_t(l.tiles_m) * TMX_TILE >= M && int64_t(l.tiles_n) * TMX_TILE >= D && l.grid == int64_t(l.tiles_m) * l.tiles_n * B, "tokmix_left: tiles");
        CHECK(int64_t(g.tiles_m) * TMX_TILE >= M && int64_t(g.tiles_n) * TMX_TILE >= K && g.grid == int64_t(g.tiles_m) * g.tiles_n * g.ranges, "tokmix_wgrad: tiles");
        CHECK(g.ranges >= 1 && g.ranges <= TMX_MAX_RANGES && int64_t(g.ranges) * g.per_range >= B && int64_t(g.ranges - 1) * g.per_range < B,
              "tokmix_wgrad B=%d: %d ranges of %d images", B, g.ranges, g.per_range);
        CHECK(g.ld == int64_t(M) * K + M && g.ws_bytes == int64_t(g.ranges) * g.ld * 4, "tokmix_wgrad: workspace");
        CHECK(sfcvit_tokmix_wgrad_workspace(B, M, K, D) == g.ws_bytes, "tokmix_wgrad: workspace entry point");
        return g;
    };
    const TokmixPlan null_plan = tokmix_left_plan(nullptr);
    CHECK(null_plan.err == SFCVIT_EINVAL && std::strstr(null_plan.msg, "null argument block"), "tokmix_left: null argument block accepted");
    accepted(1, 8, 1, 8);
    accepted(1, 1, 8, 8);
    accepted(2, 32, 5, 16);
    refused(0, 8, 8, 8, "every extent");
    refused(1, 0, 8, 8, "every extent");
    refused(1, 8, 0, 8, "every extent");
    refused(-1, 8, 8, 8, "every extent");
    refused(1, 1, 1, 8, "hidden width");
    refused(2, 12, 5, 16, "hidden width");
    refused(2, 36, 5, 16, "hidden width");
    for (int D : {0, 12, -8, INT32_MAX}) refused(2, 32, 5, D, "multiple of 8");
    // M K + M, M D and K D are ints (2^31 - 1 is prime: no product lands on it)
    CHECK(accepted(1, 32768, 65534, 8).ld == 32768 * 65535, "tokmix: largest M K + M");
    refused(1, 32768, 65535, 8, "too large");
    accepted(1, 16, 8, INT32_MAX / 16 / 8 * 8);                  // M D
    refused(1, 16, 8, INT32_MAX / 16 / 8 * 8 + 8, "too large");
    accepted(1, 8, 16, INT32_MAX / 16 / 8 * 8);                  // K D
    refused(1, 8, 16, INT32_MAX / 16 / 8 * 8 + 8, "too large");
    refused(1, INT32_MAX / 8 * 8, INT32_MAX / 8 * 8, 8, "too large");
    // the batch has no bound of its own: wgrad splits it into at most 64 ranges, left puts it on the grid
    for (int B = 1; B <= 200; B++) accepted(B, 32, 5, 16);
    CHECK(accepted(2, 32, 5, 16).ws_bytes == 2 * (32 * 5 + 32) * 4 && accepted(4096, 32, 5, 16).ws_bytes == 64 * (32 * 5 + 32) * 4, "tokmix_wgrad: the pinned workspaces");
    CHECK(accepted(INT32_MAX, 8, 8, 8).ranges == TMX_MAX_RANGES, "tokmix: the largest batch");
    {
        const sfcvit_tokmix_args a = args(INT32_MAX, 136, 8, 8);   // two row tiles: 2 (2^31 - 1) workgroups
        const TokmixPlan l = tokmix_left_plan(&a);
        CHECK(l.err == SFCVIT_EINVAL && std::strstr(l.msg, "launch grid"), "tokmix_left: a grid beyond int accepted: %s", l.msg);
        CHECK(tokmix_wgrad_plan("host_check", INT32_MAX, 136, 8, 8).err == SFCVIT_OK, "tokmix_wgrad: the same shape keeps 64 ranges");
    }
    for (int act : {int(SFCVIT_ACT_NONE), int(SFCVIT_ACT_RELU), int(SFCVIT_ACT_GELU), -1, 3}) {
        sfcvit_tokmix_args a = args(2, 32, 5, 16);
        a.act = act;
        const TokmixPlan l = tokmix_left_plan(&a);
        if (act == SFCVIT_ACT_NONE || act == SFCVIT_ACT_GELU) CHECK(l.err == SFCVIT_OK, "tokmix_left: act=%d refused: %s", act, l.msg);
        else CHECK(l.err == SFCVIT_EINVAL && std::strstr(l.msg, "act="), "tokmix_left: act=%d accepted", act);
    }
    // weight loader: the widest of 8 / 4 / 2 / 1 elements that divides the row pitch and whose bytes the pointer is aligned to
    const int M = 8, KMAX = 12;
    void *wblk = std::aligned_alloc(16, size_t(M) * KMAX * 2 + 16), *blk = std::aligned_alloc(16, 32);
    for (int pitch : {8, 12, 6, 5})
        for (int off : {0, 8, 4, 2})
            for (int tr = 0; tr < 2; tr++) {
                sfcvit_tokmix_args a = tr ? args(2, pitch, M, 16) : args(2, M, pitch, 16);
                a.w = static_cast<char *>(wblk) + off;
                a.w_transposed = tr;
                int want = 1;
                for (int u : {2, 4, 8})
                    if (pitch % u == 0 && off % (2 * u) == 0) want = u;
                const TokmixPlan l = tokmix_left_plan(&a);
                CHECK(l.err == SFCVIT_OK && l.wunit == want, "tokmix_left pitch %d, w at +%d, transposed %d: wunit %d, expected %d (%s)", pitch, off, tr, l.wunit, want, l.msg);
            }
    {
        sfcvit_tokmix_args a = args(2, 32, 5, 16);
        a.w = static_cast<char *>(wblk) + 1;
        CHECK(tokmix_left_plan(&a).err == SFCVIT_EINVAL, "tokmix_left: odd w accepted");
        a.w = wblk;
        a.bias = static_cast<char *>(blk) + 1;
        CHECK(tokmix_left_plan(&a).err == SFCVIT_EINVAL, "tokmix_left: odd bias accepted");
        a.bias = static_cast<char *>(blk) + 2;
        CHECK(tokmix_left_plan(&a).err == SFCVIT_OK, "tokmix_left: a 2-byte aligned bias refused");
        a.residual = static_cast<char *>(blk) + 8;
        CHECK(tokmix_left_plan(&a).err == SFCVIT_EINVAL && std::strstr(tokmix_left_plan(&a).msg, "16-byte"), "tokmix_left: misaligned residual accepted");
        a.residual = nullptr;
        a.x = nullptr;
        CHECK(tokmix_left_plan(&a).err == SFCVIT_EINVAL && std::strstr(tokmix_left_plan(&a).msg, "null pointer"), "tokmix_left: null x accepted");
    }
    std::free(wblk);
    std::free(blk);

    const int B = 2, Mw = 32, K = 5, D = 16;
    const TokmixPlan p = accepted(B, Mw, K, D);
    void *g = std::aligned_alloc(16, size_t(B) * Mw * D * 2), *x = std::aligned_alloc(16, size_t(B) * K * D * 2), *ws = std::aligned_alloc(16, size_t(p.ws_bytes));
    std::unique_ptr<float[]> dw(new float[Mw * K]), db(new float[Mw]);
    CHECK(tokmix_check_wgrad(p, g, x, dw.get(), db.get(), ws, p.ws_bytes) == SFCVIT_OK, "tokmix_wgrad check: %s", sfcvit_last_error());
    CHECK(tokmix_check_wgrad(p, g, nullptr, nullptr, db.get(), ws, p.ws_bytes) == SFCVIT_OK, "tokmix_wgrad: db alone needs no x");
    CHECK(tokmix_check_wgrad(p, nullptr, x, dw.get(), db.get(), ws, p.ws_bytes) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "(g)"), "tokmix_wgrad: null g accepted");
    CHECK(tokmix_check_wgrad(p, g, x, nullptr, nullptr, ws, p.ws_bytes) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "nothing to compute"),
          "tokmix_wgrad: no output accepted");
    CHECK(tokmix_check_wgrad(p, g, nullptr, dw.get(), nullptr, ws, p.ws_bytes) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "needed for dw"),
          "tokmix_wgrad: dw without x accepted");
    CHECK(tokmix_check_wgrad(p, static_cast<char *>(g) + 8, x, dw.get(), db.get(), ws, p.ws_bytes) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "aligned"),
          "tokmix_wgrad: misaligned g accepted");
    CHECK(tokmix_check_wgrad(p, g, x, dw.get(), db.get(), static_cast<char *>(ws) + 4, p.ws_bytes) == SFCVIT_EINVAL, "tokmix_wgrad: misaligned workspace accepted");
    CHECK(tokmix_check_wgrad(p, g, x, dw.get(), db.get(), ws, p.ws_bytes - 1) == SFCVIT_EINVAL && std::strstr(sfcvit_last_error(), "workspace of"),
          "tokmix_wgrad: short workspace accepted");
    CHECK(tokmix_check_wgrad(p, g, x, dw.get(), db.get(), nullptr, p.ws_bytes) == SFCVIT_EINVAL, "tokmix_wgrad: null workspace accepted");
    CHECK(tokmix_check_wgrad(tokmix_wgrad_plan("tokmix_wgrad", B, Mw, K, 12), g, x, dw.get(), db.get(), ws, p.ws_bytes) == SFCVIT_EINVAL &&
          std::strstr(sfcvit_last_error(), "D=12"), "tokmix_wgrad: the plan's refusal is the call's");
    std::free(g);
    std::free(x);
    std::free(ws);
    char name[96];
    CHECK(sfcvit_last_tokmix_kernel(name, sizeof(name)) == SFCVIT_OK && !std::strcmp(name, "none"), "tokmix: last kernel '%s'", name);
    CHECK(sfcvit_last_tokmix_kernel(nullptr, 4) == SFCVIT_EINVAL && sfcvit_last_tokmix_kernel(name, 0) == SFCVIT_EINVAL, "tokmix: null / empty name buffer accepted");
}

// add_ln_path_plan / ln_bwd_path_plan (drop_path.cpp): the geometry at the workload shapes and the edge shapes of the tests, and
// every refusal, with heap buffers of exactly B N D bf16 (branch, x, s, y and the gradients), D bf16 (gamma, beta) and B N fp32
// (mean, rstd).  The plans read no byte of them; what is pinned is that every accepted geometry stays inside them.
static void check_drop_path() {
    using namespace sfcvit;
    const RowwiseKnobs k0;
    const struct { int B, N, D, vpl; } ok[] = {{1, 1, 8, 1}, {2, 1, 8, 1}, {5, 3, 72, 1}, {2, 65, 200, 1}, {3, 7, 520, 2}, {2, 9, 1536, 4},
                                               {2, 3, 2048, 4}, {22, 197, 768, 2}, {8, 577, 1024, 2}, {1, 2, 4096, 8},
                                               {256, 196, 768, 2}, {64, 576, 1024, 2}};
    for (const auto &q : ok) {
        const size_t rows = size_t(q.B) * q.N, bytes = rows * q.D * 2;
        std::unique_ptr<char[]> a(new char[bytes + 16]), x(new char[bytes + 16]), s(new char[bytes + 16]), y(new char[bytes + 16]);
        std::unique_ptr<char[]> g(new char[q.D * 2 + 16]), b(new char[q.D * 2 + 16]);
        std::unique_ptr<float[]> mean(new float[rows]), rstd(new float[rows]);
        auto al = [](char *p) { return reinterpret_cast<void *>((reinterpret_cast<uintptr_t>(p) + 15) & ~uintptr_t(15)); };
        void *ap = al(a.get()), *xp = al(x.get()), *sp = al(s.get()), *yp = al(y.get()), *gp = al(g.get()), *bp = al(b.get());
        const AddLnPathPlan p = add_ln_path_plan(ap, xp, gp, bp, sp, yp, mean.get(), rstd.get(), q.B, q.N, q.D, 0.1f);
        CHECK(p.err == SFCVIT_OK, "drop_path fwd %d %d %d refused: %s", q.B, q.N, q.D, p.msg);
        CHECK(p.M == int(rows) && p.vpl == q.vpl && p.vpl * 512 >= q.D, "drop_path fwd %d %d %d: M %d vpl %d", q.B, q.N, q.D, p.M, p.vpl);
        CHECK(int64_t(p.blocks) * ROW_WAVES >= p.M && int64_t(p.blocks - 1) * ROW_WAVES < p.M, "drop_path fwd blocks %d for %d rows", p.blocks, p.M);
        auto fwd = [&](const void *a_, const void *x_, const void *g_, const void *b_, const void *s_, const void *y_, const float *m_,
                       const float *r_, int B, int N, int D, float rate, const char *frag, const char *what) {
            const AddLnPathPlan r = add_ln_path_plan(a_, x_, g_, b_, s_, y_, m_, r_, B, N, D, rate);
            CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag), "drop_path fwd %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
        };
        float *mp = mean.get(), *rp = rstd.get();
        fwd(nullptr, xp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null branch");
        fwd(ap, nullptr, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null x");
        fwd(ap, xp, nullptr, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null gamma");
        fwd(ap, xp, gp, nullptr, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null beta");
        fwd(ap, xp, gp, bp, nullptr, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null s");
        fwd(ap, xp, gp, bp, sp, nullptr, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null y");
        fwd(ap, xp, gp, bp, sp, yp, nullptr, rp, q.B, q.N, q.D, 0.1f, "null", "null mean");
        fwd(ap, xp, gp, bp, sp, yp, mp, nullptr, q.B, q.N, q.D, 0.1f, "null", "null rstd");
        fwd(ap, xp, gp, bp, sp, yp, mp, rp, 0, q.N, q.D, 0.1f, "B=0", "B = 0");
        fwd(ap, xp, gp, bp, sp, yp, mp, rp, q.B, -1, q.D, 0.1f, "N=-1", "N = -1");
        fwd(ap, xp, gp, bp, sp, yp, mp, rp, 65536, 32768, q.D, 0.1f, "leave int", "B * N = 2^31");
        fwd(ap, xp, gp, bp, sp, yp, mp, rp, q.B, q.N, 0, 0.1f, "D=0", "D = 0");
        fwd(ap, xp, gp, bp, sp, yp, mp, rp, q.B, q.N, 12, 0.1f, "D=12", "D = 12");
        fwd(ap, xp, gp, bp, sp, yp, mp, rp, q.B, q.N, 4104, 0.1f, "D=4104", "D = 4104");
        fwd(static_cast<char *>(ap) + 2, xp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "aligned", "misaligned branch");
        fwd(ap, xp, gp, bp, static_cast<char *>(sp) + 8, yp, mp, rp, q.B, q.N, q.D, 0.1f, "aligned", "misaligned s");
        fwd(ap, xp, static_cast<char *>(gp) + 4, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "aligned", "misaligned gamma");
        fwd(ap, xp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 1.f, "rate=1", "rate 1");
        fwd(ap, xp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, -0.25f, "rate=-0.25", "rate < 0");
        fwd(ap, xp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, std::numeric_limits<float>::quiet_NaN(), "rate=", "rate NaN");
        fwd(ap, xp, gp, bp, xp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "overlaps", "s = x");
        fwd(ap, xp, gp, bp, sp, ap, mp, rp, q.B, q.N, q.D, 0.1f, "overlaps", "y = branch");
        fwd(ap, xp, gp, bp, sp, sp, mp, rp, q.B, q.N, q.D, 0.1f, "overlaps", "y = s");
        if (bytes > 16) fwd(ap, xp, gp, bp, static_cast<char *>(xp) + bytes - 16, yp, mp, rp, q.B, q.N, q.D, 0.1f, "overlaps", "s starts in x's last vector");

        if (q.D > LN_BWD_MAX_D) continue;
        std::unique_ptr<float[]> ws(new float[3 * q.D]);
        const LnBwdPathPlan pb = ln_bwd_path_plan(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, ws.get(), 0.5f, k0);
        CHECK(pb.err == SFCVIT_OK && pb.M == int(rows), "drop_path bwd %d %d %d refused: %s", q.B, q.N, q.D, pb.msg);
        CHECK(ln_bwd_path_plan(ap, xp, mp, rp, gp, ap, sp, yp, 0.f, mp, rp, q.B, q.N, q.D, ws.get(), 0.f, k0).err == SFCVIT_OK, "drop_path bwd: dx_add, p = 0, rate = 0 refused");
        auto bwd = [&](const void *dy_, const void *x_, const float *m_, const float *r_, const void *g_, const void *add_, const void *dx_,
                       const void *dd_, float dp, const void *dg_, const void *db_, int B, int N, int D, const void *ws_, float rate,
                       const char *frag, const char *what) {
            const LnBwdPathPlan r = ln_bwd_path_plan(dy_, x_, m_, r_, g_, add_, dx_, dd_, dp, dg_, db_, B, N, D, ws_, rate, k0);
            CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag), "drop_path bwd %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
        };
        const void *w = ws.get();
        bwd(nullptr, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, w, 0.5f, "null", "null dy");
        bwd(ap, nullptr, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, w, 0.5f, "null", "null x");
        bwd(ap, xp, nullptr, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, w, 0.5f, "null", "null mean");
        bwd(ap, xp, mp, nullptr, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, w, 0.5f, "null", "null rstd");
        bwd(ap, xp, mp, rp, nullptr, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, w, 0.5f, "null", "null gamma");
        bwd(ap, xp, mp, rp, gp, nullptr, nullptr, yp, 0.1f, mp, rp, q.B, q.N, q.D, w, 0.5f, "null", "null dx");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, nullptr, 0.1f, mp, rp, q.B, q.N, q.D, w, 0.5f, "dx_drop", "missing dx_drop");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, nullptr, rp, q.B, q.N, q.D, w, 0.5f, "null", "null dgamma");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, nullptr, q.B, q.N, q.D, w, 0.5f, "null", "null dbeta");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, nullptr, 0.5f, "null", "null workspace");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, 0, q.N, q.D, w, 0.5f, "B=0", "B = 0");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, 0, q.D, w, 0.5f, "N=0", "rows_per_image = 0");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, 46341, 46341, q.D, w, 0.5f, "leave int", "B * N > int");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, 2056, w, 0.5f, "D=2056", "D = 2056");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, 4, w, 0.5f, "D=4", "D = 4");
        bwd(ap, xp, mp, rp, gp, static_cast<char *>(ap) + 8, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, w, 0.5f, "aligned", "misaligned dx_add");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, static_cast<char *>(yp) + 2, 0.1f, mp, rp, q.B, q.N, q.D, w, 0.5f, "aligned", "misaligned dx_drop");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 1.f, mp, rp, q.B, q.N, q.D, w, 0.5f, "dropout p=1", "dropout p = 1");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, -0.5f, mp, rp, q.B, q.N, q.D, w, 0.5f, "dropout p=-0.5", "dropout p < 0");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, w, 1.f, "rate=1", "rate 1");
        bwd(ap, xp, mp, rp, gp, nullptr, sp, yp, 0.1f, mp, rp, q.B, q.N, q.D, w, -1.f, "rate=-1", "rate < 0");
    }
}

// add_ln_scale_plan / ln_bwd_scale_plan (layer_scale.cpp): form and vectors per lane per width, the four-row workspace against the
// three-row one of the same grid, and every refusal, with heap buffers of exactly B N D bf16 (branch, x, s, y and the gradients),
// D bf16 (lam, gamma, beta) and B N fp32 (mean, rstd).  The plans read no byte of them.
static void check_layer_scale() {
    using namespace sfcvit;
    const RowwiseKnobs k0;
    const struct { int B, N, D, vpl; } ok[] = {{1, 1, 8, 1}, {2, 1, 8, 1}, {5, 3, 72, 1}, {2, 65, 200, 1}, {3, 7, 520, 2}, {2, 9, 1536, 4},
                                               {2, 3, 2048, 4}, {22, 197, 768, 2}, {8, 577, 1024, 2}, {1, 2, 4096, 8},
                                               {256, 196, 768, 2}, {64, 576, 1024, 2}};
    for (const auto &q : ok) {
        const size_t rows = size_t(q.B) * q.N, bytes = rows * q.D * 2;
        std::unique_ptr<char[]> a(new char[bytes + 16]), x(new char[bytes + 16]), s(new char[bytes + 16]), y(new char[bytes + 16]);
        std::unique_ptr<char[]> g(new char[q.D * 2 + 16]), b(new char[q.D * 2 + 16]), l(new char[q.D * 2 + 16]);
        std::unique_ptr<float[]> mean(new float[rows]), rstd(new float[rows]);
        auto al = [](char *p) { return reinterpret_cast<void *>((reinterpret_cast<uintptr_t>(p) + 15) & ~uintptr_t(15)); };
        void *ap = al(a.get()), *xp = al(x.get()), *sp = al(s.get()), *yp = al(y.get()), *gp = al(g.get()), *bp = al(b.get()), *lp = al(l.get());
        float *mp = mean.get(), *rp = rstd.get();
        const AddLnScalePlan p = add_ln_scale_plan(ap, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f);
        CHECK(p.err == SFCVIT_OK, "layer_scale fwd %d %d %d refused: %s", q.B, q.N, q.D, p.msg);
        CHECK(p.M == int(rows) && p.vpl == q.vpl && p.vpl * 512 >= q.D, "layer_scale fwd %d %d %d: M %d vpl %d", q.B, q.N, q.D, p.M, p.vpl);
        CHECK(int64_t(p.blocks) * ROW_WAVES >= p.M && int64_t(p.blocks - 1) * ROW_WAVES < p.M, "layer_scale fwd blocks %d for %d rows", p.blocks, p.M);
        CHECK(add_ln_scale_plan(ap, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.f).err == SFCVIT_OK, "layer_scale fwd: rate 0 refused");
        auto fwd = [&](const void *a_, const void *x_, const void *l_, const void *g_, const void *b_, const void *s_, const void *y_,
                       const float *m_, const float *r_, int B, int N, int D, float rate, const char *frag, const char *what) {
            const AddLnScalePlan r = add_ln_scale_plan(a_, x_, l_, g_, b_, s_, y_, m_, r_, B, N, D, rate);
            CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag), "layer_scale fwd %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
        };
        fwd(nullptr, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null branch");
        fwd(ap, nullptr, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null x");
        fwd(ap, xp, nullptr, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null lam");
        fwd(ap, xp, lp, nullptr, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null gamma");
        fwd(ap, xp, lp, gp, nullptr, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null beta");
        fwd(ap, xp, lp, gp, bp, nullptr, yp, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null s");
        fwd(ap, xp, lp, gp, bp, sp, nullptr, mp, rp, q.B, q.N, q.D, 0.1f, "null", "null y");
        fwd(ap, xp, lp, gp, bp, sp, yp, nullptr, rp, q.B, q.N, q.D, 0.1f, "null", "null mean");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, nullptr, q.B, q.N, q.D, 0.1f, "null", "null rstd");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, rp, 0, q.N, q.D, 0.1f, "B=0", "B = 0");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, rp, q.B, -1, q.D, 0.1f, "N=-1", "N = -1");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, rp, 65536, 32768, q.D, 0.1f, "leave int", "B * N = 2^31");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, 0, 0.1f, "D=0", "D = 0");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, 12, 0.1f, "D=12", "D = 12");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, 4104, 0.1f, "D=4104", "D = 4104");
        fwd(static_cast<char *>(ap) + 2, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "aligned", "misaligned branch");
        fwd(ap, xp, static_cast<char *>(lp) + 8, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "aligned", "misaligned lam");
        fwd(ap, xp, lp, gp, bp, static_cast<char *>(sp) + 8, yp, mp, rp, q.B, q.N, q.D, 0.1f, "aligned", "misaligned s");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, 1.f, "rate=1", "rate 1");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, -0.25f, "rate=-0.25", "rate < 0");
        fwd(ap, xp, lp, gp, bp, sp, yp, mp, rp, q.B, q.N, q.D, std::numeric_limits<float>::quiet_NaN(), "rate=", "rate NaN");
        fwd(ap, xp, lp, gp, bp, xp, yp, mp, rp, q.B, q.N, q.D, 0.1f, "overlaps", "s = x");
        fwd(ap, xp, lp, gp, bp, sp, ap, mp, rp, q.B, q.N, q.D, 0.1f, "overlaps", "y = branch");
        fwd(ap, xp, lp, gp, bp, sp, sp, mp, rp, q.B, q.N, q.D, 0.1f, "overlaps", "y = s");

        if (q.D > LN_BWD_MAX_D) continue;
        std::unique_ptr<float[]> ws(new float[4 * q.D]);
        const void *w = ws.get();
        const LnBwdScalePlan pb = ln_bwd_scale_plan(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, k0);
        const LnBwdPlan three = ln_bwd_geometry(int(rows), q.D, false, k0);
        const bool cols = q.D == 768 || q.D == 1024;
        CHECK(pb.err == SFCVIT_OK && pb.M == int(rows) && pb.cols == cols && !pb.add, "layer_scale bwd %d %d %d refused: %s", q.B, q.N, q.D, pb.msg);
        CHECK(pb.inst == (cols ? q.D / 256 : q.D <= 512 ? 1 : q.D <= 1024 ? 2 : 4), "layer_scale bwd D %d: form %d inst %d", q.D, int(pb.cols), pb.inst);
        RowwiseKnobs kv;
        kv.ln_cols = 0;                                       // SFCVIT_LN_COLS=0: the 16-byte-vector form at every width
        const LnBwdScalePlan pv = ln_bwd_scale_geometry(int(rows), q.D, false, kv);
        CHECK(!pv.cols && pv.inst == (q.D <= 512 ? 1 : q.D <= 1024 ? 2 : 4) && pv.ws_bytes == int64_t(pv.blocks) * 4 * q.D * 4, "layer_scale bwd D %d without cols: inst %d", q.D, pv.inst);
        CHECK(pb.blocks == three.blocks && pb.lds == three.lds, "layer_scale bwd %d %d: grid %d / lds %zu are not ln_bwd_geometry's", int(rows), q.D, pb.blocks, pb.lds);
        CHECK(pb.ws_bytes * 3 == three.ws_bytes * 4 && pb.ws_bytes == int64_t(pb.blocks) * 4 * q.D * 4, "layer_scale bwd: workspace %lld", (long long)pb.ws_bytes);
        CHECK(ln_bwd_scale_geometry(int(rows), q.D, false, k0).ws_bytes == pb.ws_bytes, "layer_scale bwd: the workspace query disagrees");
        char name[96], want[96];
        scale_kernel_name(pb, name, sizeof(name));
        std::snprintf(want, sizeof(want), "ln_bwd%s_scale_kernel<%d, false>", cols ? "_cols" : "", pb.inst);
        CHECK(!std::strcmp(name, want), "layer_scale bwd name '%s'", name);
        const LnBwdScalePlan pa = ln_bwd_scale_plan(ap, xp, mp, rp, gp, ap, ap, lp, sp, yp, 0.f, mp, rp, mp, q.B, q.N, q.D, w, 0.f, k0);
        scale_kernel_name(pa, name, sizeof(name));
        std::snprintf(want, sizeof(want), "ln_bwd%s_scale_kernel<%d, true>", cols ? "_cols" : "", pa.inst);
        CHECK(pa.err == SFCVIT_OK && pa.add && !std::strcmp(name, want), "layer_scale bwd: dx_add, p = 0, rate = 0: '%s' %s", name, pa.msg);
        auto bwd = [&](const void *dy_, const void *x_, const float *m_, const float *r_, const void *g_, const void *add_, const void *br_,
                       const void *l_, const void *dx_, const void *dd_, float dp, const void *dg_, const void *db_, const void *dl_, int B,
                       int N, int D, const void *ws_, float rate, const char *frag, const char *what) {
            const LnBwdScalePlan r = ln_bwd_scale_plan(dy_, x_, m_, r_, g_, add_, br_, l_, dx_, dd_, dp, dg_, db_, dl_, B, N, D, ws_, rate, k0);
            CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag), "layer_scale bwd %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
        };
        bwd(nullptr, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "null", "null dy");
        bwd(ap, nullptr, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "null", "null x");
        bwd(ap, xp, nullptr, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "null", "null mean");
        bwd(ap, xp, mp, nullptr, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "null", "null rstd");
        bwd(ap, xp, mp, rp, nullptr, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "null", "null gamma");
        bwd(ap, xp, mp, rp, gp, nullptr, nullptr, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "null", "null branch");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, nullptr, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "null", "null lam");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, nullptr, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "null", "null dx");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, nullptr, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "dx_drop", "missing dx_drop");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, nullptr, rp, mp, q.B, q.N, q.D, w, 0.5f, "null", "null dgamma");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, nullptr, mp, q.B, q.N, q.D, w, 0.5f, "null", "null dbeta");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, nullptr, q.B, q.N, q.D, w, 0.5f, "null", "null dlam");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, nullptr, 0.5f, "null", "null workspace");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, 0, q.N, q.D, w, 0.5f, "B=0", "B = 0");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, 0, q.D, w, 0.5f, "N=0", "rows_per_image = 0");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, 46341, 46341, q.D, w, 0.5f, "leave int", "B * N > int");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, 2056, w, 0.5f, "D=2056", "D = 2056");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, 4, w, 0.5f, "D=4", "D = 4");
        bwd(ap, xp, mp, rp, gp, static_cast<char *>(ap) + 8, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "aligned", "misaligned dx_add");
        bwd(ap, xp, mp, rp, gp, nullptr, static_cast<char *>(ap) + 4, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "aligned", "misaligned branch");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, static_cast<char *>(lp) + 2, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "aligned", "misaligned lam");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, static_cast<char *>(yp) + 2, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "aligned", "misaligned dx_drop");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 1.f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "dropout p=1", "dropout p = 1");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, -0.5f, mp, rp, mp, q.B, q.N, q.D, w, 0.5f, "dropout p=-0.5", "dropout p < 0");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, 1.f, "rate=1", "rate 1");
        bwd(ap, xp, mp, rp, gp, nullptr, ap, lp, sp, yp, 0.1f, mp, rp, mp, q.B, q.N, q.D, w, -1.f, "rate=-1", "rate < 0");
    }
}

// adamw_ema_plan (model_ema.cpp): the grid at the sizes of the tests and the workloads, and every refusal, with heap buffers of
// exactly n bf16 (param, grad) and n fp32 (master, m, v, ema).  The plan reads the two structs and no byte of the buffers.
// qk_norm_fwd_plan / qk_norm_bwd_plan (qk_norm.cpp): the grid and the workspace per shape, and every refusal.
static void check_qk_norm() {
    // (the buffers of the largest shapes are terabytes: raw sits 2^46 bytes above qkv so that none of them overlaps)
    void *qkv = ptr(8), *raw = reinterpret_cast<void *>(uintptr_t(1) << 46), *P = ptr(3), *dP = ptr(4), *cs = ptr(5), *ws = ptr(6);
    const float *vs = static_cast<const float *>(ptr(7));
    struct Q { int M, H, hd, hp; };
    for (const Q &q : {Q{10, 4, 64, 64}, Q{10, 3, 64, 64}, Q{394, 12, 64, 64}, Q{10, 4, 48, 64}, Q{10, 4, 20, 64}, Q{7, 2, 128, 128},
                       Q{7, 2, 96, 128}, Q{7, 1, 192, 192}, Q{7, 1, 256, 256}, Q{50176, 12, 64, 64}, Q{36864, 16, 64, 64}, Q{1, 1, 1, 64},
                       Q{INT_MAX, 1, 64, 64}}) {
        const QkNormPlan f = qk_norm_fwd_plan(qkv, raw, P, q.M, q.H, q.hd, q.hp, 1e-6f);
        const QkNormPlan b = qk_norm_bwd_plan(qkv, raw, P, dP, cs, vs, ws, q.M, q.H, q.hd, q.hp, 0.f);
        CHECK(f.err == SFCVIT_OK && b.err == SFCVIT_OK, "qk_norm %d %d %d %d refused: %s %s", q.M, q.H, q.hd, q.hp, f.msg, b.msg);
        const int sgs = (2 * q.H + 7) / 8, chunks = int((int64_t(q.M) + QK_ROWS_PER_WG - 1) / QK_ROWS_PER_WG);
        CHECK(f.vpl == q.hp / 64 && f.slot_groups == sgs && f.rows_per_wg == QK_ROWS_PER_WG && f.chunks == chunks && f.blocks == sgs * chunks,
              "qk_norm fwd %d %d %d: vpl %d groups %d chunks %d blocks %d", q.M, q.H, q.hp, f.vpl, f.slot_groups, f.chunks, f.blocks);
        CHECK(b.blocks == f.blocks && b.chunks == f.chunks && b.part_ld == 12 * q.hp && b.ws_bytes == int64_t(b.blocks) * 12 * q.hp * 4,
              "qk_norm bwd %d %d %d: blocks %d ws %lld", q.M, q.H, q.hp, b.blocks, (long long)b.ws_bytes);
        CHECK(int64_t(f.chunks) * f.rows_per_wg >= q.M && int64_t(f.chunks - 1) * f.rows_per_wg < q.M, "qk_norm chunks %d for %d rows", f.chunks, q.M);
        CHECK(qk_norm_geometry(q.M, q.H, q.hp, "t").ws_bytes == b.ws_bytes, "qk_norm: the workspace query disagrees");
        const int Da = q.H * q.hp;
        CHECK(b.reduce_blocks == 2 * Da / 16 + 4 * q.hp / 16 + (Da + 1023) / 1024, "qk_norm bwd reduce blocks %d", b.reduce_blocks);
        const QkNormPlan n = qk_norm_bwd_plan(qkv, raw, P, dP, nullptr, nullptr, ws, q.M, q.H, q.hd, q.hp, 1e-5f);
        CHECK(n.err == SFCVIT_OK && n.reduce_blocks == 4 * q.hp / 16, "qk_norm bwd without colsum: %s, %d reduce blocks", n.msg, n.reduce_blocks);
    }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto fwd = [&](const char *what, const char *frag, void *q_, void *r_, void *p_, int M, int H, int hd, int hp, float eps) {
        const QkNormPlan r = qk_norm_fwd_plan(q_, r_, p_, M, H, hd, hp, eps);
        CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag), "qk_norm fwd %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
    };
    auto bwd = [&](const char *what, const char *frag, void *q_, void *r_, void *p_, void *d_, void *c_, const float *v_, void *w_, int M,
                   int H, int hd, int hp, float eps) {
        const QkNormPlan r = qk_norm_bwd_plan(q_, r_, p_, d_, c_, v_, w_, M, H, hd, hp, eps);
        CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag), "qk_norm bwd %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
    };
    auto off8 = [](const void *p) { return reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(p) + 8); };
    fwd("null qkv", "null", nullptr, raw, P, 10, 4, 64, 64, 1e-6f);
    fwd("null raw", "null", qkv, nullptr, P, 10, 4, 64, 64, 1e-6f);
    fwd("null params", "null", qkv, raw, nullptr, 10, 4, 64, 64, 1e-6f);
    fwd("qkv + 8", "aligned", off8(qkv), raw, P, 10, 4, 64, 64, 1e-6f);
    fwd("raw + 8", "aligned", qkv, off8(raw), P, 10, 4, 64, 64, 1e-6f);
    fwd("params + 8", "aligned", qkv, raw, off8(P), 10, 4, 64, 64, 1e-6f);
    fwd("raw in qkv", "overlaps", qkv, reinterpret_cast<char *>(qkv) + 1024, P, 10, 4, 64, 64, 1e-6f);
    bwd("null dqkv", "null", nullptr, raw, P, dP, cs, vs, ws, 10, 4, 64, 64, 1e-6f);
    bwd("null raw", "null", qkv, nullptr, P, dP, cs, vs, ws, 10, 4, 64, 64, 1e-6f);
    bwd("null params", "null", qkv, raw, nullptr, dP, cs, vs, ws, 10, 4, 64, 64, 1e-6f);
    bwd("null dparams", "null", qkv, raw, P, nullptr, cs, vs, ws, 10, 4, 64, 64, 1e-6f);
    bwd("null ws", "workspace", qkv, raw, P, dP, cs, vs, nullptr, 10, 4, 64, 64, 1e-6f);
    bwd("vsum alone", "vsum without colsum", qkv, raw, P, dP, nullptr, vs, ws, 10, 4, 64, 64, 1e-6f);
    bwd("dqkv + 8", "aligned", off8(qkv), raw, P, dP, cs, vs, ws, 10, 4, 64, 64, 1e-6f);
    bwd("dparams + 8", "aligned", qkv, raw, P, off8(dP), cs, vs, ws, 10, 4, 64, 64, 1e-6f);
    bwd("colsum + 8", "aligned", qkv, raw, P, dP, off8(cs), vs, ws, 10, 4, 64, 64, 1e-6f);
    bwd("vsum + 8", "aligned", qkv, raw, P, dP, cs, static_cast<const float *>(off8(vs)), ws, 10, 4, 64, 64, 1e-6f);
    bwd("ws + 8", "aligned", qkv, raw, P, dP, cs, vs, off8(ws), 10, 4, 64, 64, 1e-6f);
    bwd("raw in dqkv", "overlaps", qkv, reinterpret_cast<char *>(qkv) + 1024, P, dP, cs, vs, ws, 10, 4, 64, 64, 1e-6f);
    for (int hp : {0, 32, 96, 65, 512, -64}) {
        fwd("hp", "not a kernel head dim", qkv, raw, P, 10, 4, 8, hp, 1e-6f);
        bwd("hp", "not a kernel head dim", qkv, raw, P, dP, cs, vs, ws, 10, 4, 8, hp, 1e-6f);
    }
    for (int hd : {0, -1, 65, 1000}) {
        fwd("hd", "hd=", qkv, raw, P, 10, 4, hd, 64, 1e-6f);
        bwd("hd", "hd=", qkv, raw, P, dP, cs, vs, ws, 10, 4, hd, 64, 1e-6f);
    }
    fwd("hd > hp", "hd=129", qkv, raw, P, 10, 4, 129, 128, 1e-6f);
    for (int z : {0, -5}) {
        fwd("M", "M=", qkv, raw, P, z, 4, 64, 64, 1e-6f);
        fwd("H", "H=", qkv, raw, P, 10, z, 64, 64, 1e-6f);
        bwd("M", "M=", qkv, raw, P, dP, cs, vs, ws, z, 4, 64, 64, 1e-6f);
        bwd("H", "H=", qkv, raw, P, dP, cs, vs, ws, 10, z, 64, 64, 1e-6f);
    }
    fwd("row width", "leaves int", qkv, raw, P, 10, 11184811, 64, 64, 1e-6f);               // 3 * H * 64 = 2^31 + 64
    bwd("row width", "leaves int", qkv, raw, P, dP, cs, vs, ws, 10, INT_MAX, 64, 256, 1e-6f);
    CHECK(qk_norm_fwd_plan(qkv, raw, P, 10, 11184810, 64, 64, 1e-6f).err == SFCVIT_OK, "qk_norm: the widest row that fits is refused");
    fwd("grid", "leaves int", qkv, raw, P, INT_MAX, 256, 64, 64, 1e-6f);                   // 64 slot groups * 2^25 chunks
    for (float eps : {-1e-6f, nan, inf, -inf}) {
        fwd("eps", "eps=", qkv, raw, P, 10, 4, 64, 64, eps);
        bwd("eps", "eps=", qkv, raw, P, dP, cs, vs, ws, 10, 4, 64, 64, eps);
    }
    CHECK(qk_norm_fwd_plan(qkv, raw, P, 10, 4, 64, 64, 0.f).err == SFCVIT_OK, "qk_norm: eps = 0 refused");
}

// rope_fwd_plan / rope_bwd_plan (rope.cpp): the grid and the workspace per shape, and every refusal.
static void check_rope() {
    void *qkv = ptr(8), *cs = ptr(5), *ws = ptr(6);
    const float *tab = static_cast<const float *>(ptr(3)), *vs = static_cast<const float *>(ptr(7));
    struct R { int B, N, H, hd, hp; };
    for (const R &r : {R{2, 5, 4, 64, 64}, R{2, 5, 3, 64, 64}, R{2, 197, 12, 64, 64}, R{67, 3, 1, 64, 64}, R{1, 9, 2, 64, 64},
                       R{3, 1, 2, 64, 64}, R{2, 5, 4, 48, 64}, R{2, 5, 4, 20, 64}, R{1, 3, 1, 2, 64}, R{1, 7, 2, 128, 128},
                       R{1, 7, 2, 96, 128}, R{1, 7, 1, 192, 192}, R{1, 7, 1, 256, 256}, R{256, 196, 12, 64, 64}, R{64, 576, 16, 64, 64},
                       R{INT_MAX, 1, 1, 64, 64}, R{1, INT_MAX, 1, 64, 64}}) {
        const RopePlan f = rope_fwd_plan(qkv, tab, r.B, r.N, r.H, r.hd, r.hp);
        const RopePlan b = rope_bwd_plan(qkv, tab, cs, vs, ws, r.B, r.N, r.H, r.hd, r.hp);
        CHECK(f.err == SFCVIT_OK && b.err == SFCVIT_OK, "rope %d %d %d %d %d refused: %s %s", r.B, r.N, r.H, r.hd, r.hp, f.msg, b.msg);
        const int sgs = (2 * r.H + 7) / 8, tbs = int((int64_t(r.N) + ROPE_WAVES - 1) / ROPE_WAVES);
        const int bcs = int((int64_t(r.B) + ROPE_BATCH_PER_WG - 1) / ROPE_BATCH_PER_WG);
        CHECK(f.vpl == r.hp / 64 && f.slot_groups == sgs && f.token_blocks == tbs && f.batch_chunks == bcs &&
                  int64_t(f.blocks) == int64_t(sgs) * tbs * bcs,
              "rope fwd %d %d %d %d: vpl %d groups %d token blocks %d batch chunks %d blocks %d", r.B, r.N, r.H, r.hp, f.vpl,
              f.slot_groups, f.token_blocks, f.batch_chunks, f.blocks);
        CHECK(b.blocks == f.blocks && b.part_ld == 8 * r.hp && b.ws_bytes == int64_t(b.blocks) * 8 * r.hp * 4 && b.sums,
              "rope bwd %d %d %d %d: blocks %d ws %lld", r.B, r.N, r.H, r.hp, b.blocks, (long long)b.ws_bytes);
        CHECK(int64_t(tbs) * ROPE_WAVES >= r.N && int64_t(tbs - 1) * ROPE_WAVES < r.N, "rope token blocks %d for %d tokens", tbs, r.N);
        CHECK(int64_t(bcs) * ROPE_BATCH_PER_WG >= r.B && int64_t(bcs - 1) * ROPE_BATCH_PER_WG < r.B, "rope batch chunks %d for %d images", bcs, r.B);
        CHECK(rope_geometry(r.B, r.N, r.H, r.hp, "t").ws_bytes == b.ws_bytes, "rope: the workspace query disagrees");
        const int Da = r.H * r.hp;
        CHECK(b.reduce_blocks == 2 * Da / 16 + (Da + 1023) / 1024, "rope bwd reduce blocks %d", b.reduce_blocks);
        const RopePlan c = rope_bwd_plan(qkv, tab, cs, nullptr, ws, r.B, r.N, r.H, r.hd, r.hp);
        CHECK(c.err == SFCVIT_OK && c.sums && c.reduce_blocks == 2 * Da / 16, "rope bwd without vsum: %s, %d reduce blocks", c.msg, c.reduce_blocks);
        const RopePlan n = rope_bwd_plan(qkv, tab, nullptr, nullptr, nullptr, r.B, r.N, r.H, r.hd, r.hp);
        CHECK(n.err == SFCVIT_OK && !n.sums && n.reduce_blocks == 0, "rope bwd without sums: %s, %d reduce blocks", n.msg, n.reduce_blocks);
        const RopePlan w = rope_bwd_plan(qkv, tab, nullptr, nullptr, ws, r.B, r.N, r.H, r.hd, r.hp);     // a workspace nobody needs is no error
        CHECK(w.err == SFCVIT_OK && !w.sums, "rope bwd with a spare workspace: %s", w.msg);
    }
    // ViT-B/16 at batch 256 fills 256 CUs several times over
    CHECK(rope_geometry(256, 196, 12, 64, "t").blocks == 3 * 49 * 16, "rope: ViT-B grid %d", rope_geometry(256, 196, 12, 64, "t").blocks);
    auto fwd = [&](const char *what, const char *frag, void *q_, const void *t_, int B, int N, int H, int hd, int hp) {
        const RopePlan r = rope_fwd_plan(q_, t_, B, N, H, hd, hp);
        CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag), "rope fwd %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
    };
    auto bwd = [&](const char *what, const char *frag, void *q_, const void *t_, void *c_, const float *v_, void *w_, int B, int N, int H,
                   int hd, int hp) {
        const RopePlan r = rope_bwd_plan(q_, t_, c_, v_, w_, B, N, H, hd, hp);
        CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag), "rope bwd %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
    };
    auto off8 = [](const void *p) { return reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(p) + 8); };
    fwd("null qkv", "null", nullptr, tab, 2, 5, 4, 64, 64);
    fwd("null table", "null", qkv, nullptr, 2, 5, 4, 64, 64);
    fwd("qkv + 8", "aligned", off8(qkv), tab, 2, 5, 4, 64, 64);
    fwd("table + 8", "aligned", qkv, off8(tab), 2, 5, 4, 64, 64);
    bwd("null dqkv", "null", nullptr, tab, cs, vs, ws, 2, 5, 4, 64, 64);
    bwd("null table", "null", qkv, nullptr, cs, vs, ws, 2, 5, 4, 64, 64);
    bwd("null ws", "colsum without a workspace", qkv, tab, cs, vs, nullptr, 2, 5, 4, 64, 64);
    bwd("null ws, no vsum", "colsum without a workspace", qkv, tab, cs, nullptr, nullptr, 2, 5, 4, 64, 64);
    bwd("vsum alone", "vsum without colsum", qkv, tab, nullptr, vs, ws, 2, 5, 4, 64, 64);
    bwd("dqkv + 8", "aligned", off8(qkv), tab, cs, vs, ws, 2, 5, 4, 64, 64);
    bwd("table + 8", "aligned", qkv, off8(tab), cs, vs, ws, 2, 5, 4, 64, 64);
    bwd("colsum + 8", "aligned", qkv, tab, off8(cs), vs, ws, 2, 5, 4, 64, 64);
    bwd("vsum + 8", "aligned", qkv, tab, cs, static_cast<const float *>(off8(vs)), ws, 2, 5, 4, 64, 64);
    bwd("ws + 8", "aligned", qkv, tab, cs, vs, off8(ws), 2, 5, 4, 64, 64);
    for (int hp : {0, 32, 96, 65, 512, -64}) {
        fwd("hp", "not a kernel head dim", qkv, tab, 2, 5, 4, 8, hp);
        bwd("hp", "not a kernel head dim", qkv, tab, cs, vs, ws, 2, 5, 4, 8, hp);
    }
    for (int hd : {0, -2, 1, 3, 63, 66, 1000}) {                                            // odd, < 2, > hp
        fwd("hd", "hd=", qkv, tab, 2, 5, 4, hd, 64);
        bwd("hd", "hd=", qkv, tab, cs, vs, ws, 2, 5, 4, hd, 64);
    }
    fwd("hd > hp", "hd=130", qkv, tab, 2, 5, 4, 130, 128);
    for (int z : {0, -5}) {
        fwd("B", "B=", qkv, tab, z, 5, 4, 64, 64);
        fwd("N", "N=", qkv, tab, 2, z, 4, 64, 64);
        fwd("H", "H=", qkv, tab, 2, 5, z, 64, 64);
        bwd("B", "B=", qkv, tab, cs, vs, ws, z, 5, 4, 64, 64);
        bwd("N", "N=", qkv, tab, cs, vs, ws, 2, z, 4, 64, 64);
        bwd("H", "H=", qkv, tab, cs, vs, ws, 2, 5, z, 64, 64);
    }
    fwd("row width", "leaves int", qkv, tab, 2, 5, 11184811, 64, 64);                       // 3 * H * 64 = 2^31 + 64
    bwd("row width", "leaves int", qkv, tab, cs, vs, ws, 2, 5, INT_MAX, 64, 256);
    CHECK(rope_fwd_plan(qkv, tab, 2, 5, 11184810, 64, 64).err == SFCVIT_OK, "rope: the widest row that fits is refused");
    fwd("rows", "leaves int", qkv, tab, 65536, 32768, 1, 64, 64);                           // B * N = 2^31
    fwd("grid", "leaves int", qkv, tab, 1, INT_MAX, 64, 64, 64);                            // 16 slot groups * 2^29 token blocks
}

static void check_model_ema() {
    using namespace sfcvit;
    const RowwiseKnobs k0;
    const struct { int64_t n; int grid; } ok[] = {{1, 1}, {3, 1}, {4, 1}, {7, 1}, {2048, 1}, {2049, 2}, {2451, 2}, {5525002, 2048}, {4194304, 2048},
                                                  {4194296, 2048}, {4194305, 2048}, {12582917, 2048}, {86567656, 2048}};
    for (const auto &q : ok) {
        const size_t n = size_t(q.n);
        std::unique_ptr<char[]> pb(new char[n * 2 + 16]), gb(new char[n * 2 + 16]), wb(new char[n * 4 + 16]), mb(new char[n * 4 + 16]),
            vb(new char[n * 4 + 16]), eb(new char[n * 4 + 16]);
        auto al = [](char *p) { return reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(p) + 15) & ~uintptr_t(15)); };
        sfcvit_adamw_args a{};
        a.param = al(pb.get()); a.grad = al(gb.get());
        a.master = reinterpret_cast<float *>(al(wb.get())); a.m = reinterpret_cast<float *>(al(mb.get())); a.v = reinterpret_cast<float *>(al(vb.get()));
        a.n = q.n; a.lr = 3e-4f; a.beta1 = 0.9f; a.beta2 = 0.999f; a.eps = 1e-8f; a.grad_scale = 1.f; a.step = 1;
        sfcvit_ema_args e{reinterpret_cast<float *>(al(eb.get())), 0.9999f, 1};
        const AdamwEmaPlan p = adamw_ema_plan(&a, &e, k0);
        CHECK(p.err == SFCVIT_OK, "model_ema n %lld refused: %s", (long long)q.n, p.msg);
        CHECK(p.grid == q.grid && p.grid >= 1 && p.grid <= ADAMW_MAX_BLOCKS, "model_ema n %lld: grid %d, want %d", (long long)q.n, p.grid, q.grid);
        // one lane per 8 parameters covers everything below the cap
        CHECK(p.grid == ADAMW_MAX_BLOCKS || int64_t(p.grid) * ADAMW_THREADS * 8 >= q.n, "model_ema n %lld: grid %d is short", (long long)q.n, p.grid);
        e.decay = 0.f;
        CHECK(adamw_ema_plan(&a, &e, k0).err == SFCVIT_OK, "model_ema: decay 0 refused");
        e.decay = 0.9999f;
        { sfcvit_adamw_args b = a; b.step = 0; float st[8] = {}; b.dev_state = st;
          CHECK(adamw_ema_plan(&b, &e, k0).err == SFCVIT_OK, "model_ema: step 0 with dev_state refused"); }
        auto bad = [&](const sfcvit_adamw_args *a_, const sfcvit_ema_args *e_, const char *frag, const char *what) {
            const AdamwEmaPlan r = adamw_ema_plan(a_, e_, k0);
            CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag) && r.grid == 0, "model_ema %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
        };
        bad(nullptr, &e, "null pointer (a)", "null a");
        bad(&a, nullptr, "null pointer (e)", "null e");
        { sfcvit_adamw_args b = a; b.param = nullptr; bad(&b, &e, "null", "null param"); }
        { sfcvit_adamw_args b = a; b.master = nullptr; bad(&b, &e, "null", "null master"); }
        { sfcvit_adamw_args b = a; b.grad = nullptr; bad(&b, &e, "null", "null grad"); }
        { sfcvit_adamw_args b = a; b.m = nullptr; bad(&b, &e, "null", "null m"); }
        { sfcvit_adamw_args b = a; b.v = nullptr; bad(&b, &e, "null", "null v"); }
        { sfcvit_ema_args f = e; f.ema = nullptr; bad(&a, &f, "(ema)", "null ema"); }
        { sfcvit_adamw_args b = a; b.n = 0; bad(&b, &e, "n=0", "n = 0"); }
        { sfcvit_adamw_args b = a; b.n = -5; bad(&b, &e, "n=-5", "n < 0"); }
        { sfcvit_adamw_args b = a; b.n = INT64_MAX; bad(&b, &e, "address space", "n = 2^63 - 1"); }
        { sfcvit_adamw_args b = a; b.step = 0; bad(&b, &e, "step=0", "step 0 without dev_state"); }
        { sfcvit_adamw_args b = a; b.param = static_cast<char *>(a.param) + 2; bad(&b, &e, "aligned", "misaligned param"); }
        { sfcvit_adamw_args b = a; b.master = a.master + 1; bad(&b, &e, "aligned", "misaligned master"); }
        { sfcvit_adamw_args b = a; b.v = a.v + 2; bad(&b, &e, "aligned", "misaligned v"); }
        { sfcvit_ema_args f = e; f.ema = e.ema + 1; bad(&a, &f, "ema must be 16-byte aligned", "misaligned ema"); }
        for (float d : {1.f, -0.1f, 1.5f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
            sfcvit_ema_args f = e; f.decay = d; bad(&a, &f, "decay=", "decay outside [0, 1)");
        }
        { sfcvit_ema_args f = e; f.ema = a.master; bad(&a, &f, "ema overlaps master", "ema = master"); }
        { sfcvit_ema_args f = e; f.ema = a.m; bad(&a, &f, "ema overlaps m", "ema = m"); }
        { sfcvit_ema_args f = e; f.ema = a.v; bad(&a, &f, "ema overlaps v", "ema = v"); }
        { sfcvit_ema_args f = e; f.ema = static_cast<float *>(a.param); bad(&a, &f, "ema overlaps param", "ema = param"); }
        { sfcvit_ema_args f = e; f.ema = reinterpret_cast<float *>(const_cast<void *>(a.grad)); bad(&a, &f, "ema overlaps", "ema = grad"); }       // n fp32 from grad may reach a neighbouring block first
        if (q.n >= 8) {       // starts in master's last vector / ends in master's first
            sfcvit_ema_args f = e;
            f.ema = a.master + (q.n - 1) / 4 * 4; bad(&a, &f, "ema overlaps", "ema starts in master's last vector");
            sfcvit_adamw_args b = a; b.master = e.ema + (q.n - 1) / 4 * 4; bad(&b, &e, "ema overlaps", "master starts in ema's last vector");
        }
    }
}

// grad_accum_plan / grad_accum_finish_plan (grad_accum.cpp): the grids at the sizes of the tests and the workloads -- adamw_plan's,
// and with a sum of squares sumsq_plan's -- and every refusal, with heap buffers of exactly n bf16 (grad) and n fp32 (acc), one
// float (sumsq) and SFCVIT_SUMSQ_WORKSPACE_BYTES (workspace).  The plans read no byte of any buffer.
static void check_grad_accum() {
    using namespace sfcvit;
    const RowwiseKnobs k0;
    const int max_parts = SFCVIT_SUMSQ_WORKSPACE_BYTES / 4;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const struct { int64_t n; int grid; } ok[] = {{1, 1}, {3, 1}, {4, 1}, {7, 1}, {2048, 1}, {2049, 2}, {2451, 2}, {5525002, 2048}, {4194304, 2048},
                                                  {2097152, 1024}, {2097153, 1025}, {12582917, 2048}, {86567656, 2048}};
    for (const auto &q : ok) {
        const size_t n = size_t(q.n);
        std::unique_ptr<char[]> gb(new char[n * 2 + 16]), ab(new char[n * 4 + 16]), sb(new char[4 + 16]), wb(new char[SFCVIT_SUMSQ_WORKSPACE_BYTES + 16]);
        auto al = [](char *p) { return reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(p) + 15) & ~uintptr_t(15)); };
        char *g = al(gb.get()), *w = al(wb.get());
        float *acc = reinterpret_cast<float *>(al(ab.get())), *sq = reinterpret_cast<float *>(al(sb.get()));
        sfcvit_adamw_args aa{};
        aa.param = g; aa.grad = g; aa.master = acc; aa.m = acc; aa.v = acc; aa.n = q.n; aa.step = 1;
        const int adamw_grid = adamw_plan(&aa, k0).grid;
        for (int first = 0; first < 2; first++) {
            const GradAccumPlan p = grad_accum_plan(g, acc, q.n, k0);
            CHECK(p.err == SFCVIT_OK && p.grid == q.grid && p.grid == adamw_grid && p.nt == 3, "grad_accum n %lld: grid %d, want %d (%s)", (long long)q.n, p.grid, q.grid, p.msg);
        }
        const GradAccumPlan f0 = grad_accum_finish_plan(g, acc, q.n, 0.25f, nullptr, nullptr, k0);
        CHECK(f0.err == SFCVIT_OK && f0.grid == q.grid, "grad_accum_finish n %lld: grid %d, want %d (%s)", (long long)q.n, f0.grid, q.grid, f0.msg);
        CHECK(grad_accum_finish_plan(g, acc, q.n, 0.25f, nullptr, w, k0).err == SFCVIT_OK, "grad_accum_finish: workspace without sumsq refused");
        const GradAccumPlan f1 = grad_accum_finish_plan(g, acc, q.n, 0.25f, sq, w, k0);
        const int want = q.grid > max_parts ? max_parts : q.grid;
        CHECK(f1.err == SFCVIT_OK && f1.grid == want && f1.grid == sumsq_plan(g, q.n, sq, w).grid && f1.nt == 3,
              "grad_accum_finish + sumsq n %lld: grid %d, want %d (%s)", (long long)q.n, f1.grid, want, f1.msg);
        CHECK(int64_t(f1.grid) * 4 <= SFCVIT_SUMSQ_WORKSPACE_BYTES, "grad_accum_finish n %lld: %d partials leave the workspace", (long long)q.n, f1.grid);
        { RowwiseKnobs k; k.adamw_nt = 0; CHECK(grad_accum_plan(g, acc, q.n, k).nt == 0 && grad_accum_finish_plan(g, acc, q.n, 1.f, sq, w, k).nt == 0, "grad_accum: adamw_nt 0"); }
        auto bad = [&](const GradAccumPlan &r, const char *frag, const char *what) {
            CHECK(r.err == SFCVIT_EINVAL && std::strstr(r.msg, frag) && r.grid == 0, "grad_accum %s: want '%s', got %d '%s'", what, frag, r.err, r.msg);
        };
        // what both entry points refuse
        bad(grad_accum_plan(nullptr, acc, q.n, k0), "(grad)", "null grad");
        bad(grad_accum_plan(g, nullptr, q.n, k0), "(acc)", "null acc");
        bad(grad_accum_plan(g, acc, 0, k0), "n=0", "n = 0");
        bad(grad_accum_plan(g, acc, -5, k0), "n=-5", "n < 0");
        bad(grad_accum_plan(g, acc, INT64_MAX, k0), "address space", "n = 2^63 - 1");
        bad(grad_accum_plan(g + 2, acc, q.n, k0), "grad must be 16-byte aligned", "misaligned grad");
        bad(grad_accum_plan(g, acc + 1, q.n, k0), "acc must be 16-byte aligned", "misaligned acc");
        bad(grad_accum_plan(g, reinterpret_cast<float *>(g), q.n, k0), "acc overlaps grad", "acc = grad");
        bad(grad_accum_finish_plan(nullptr, acc, q.n, 0.5f, sq, w, k0), "grad_accum_finish: null pointer (grad)", "finish: null grad");
        bad(grad_accum_finish_plan(g, nullptr, q.n, 0.5f, sq, w, k0), "(acc)", "finish: null acc");
        bad(grad_accum_finish_plan(g, acc, 0, 0.5f, sq, w, k0), "n=0", "finish: n = 0");
        bad(grad_accum_finish_plan(g + 8, acc, q.n, 0.5f, sq, w, k0), "grad must be 16-byte aligned", "finish: misaligned grad");
        bad(grad_accum_finish_plan(g, acc + 2, q.n, 0.5f, sq, w, k0), "acc must be 16-byte aligned", "finish: misaligned acc");
        bad(grad_accum_finish_plan(g, reinterpret_cast<float *>(g), q.n, 0.5f, sq, w, k0), "acc overlaps grad", "finish: acc = grad");
        if (q.n >= 16) {      // acc starts in grad's last vector / grad starts in acc's last vector
            bad(grad_accum_plan(g, reinterpret_cast<float *>(g + (q.n * 2 - 1) / 16 * 16), q.n, k0), "acc overlaps grad", "acc starts in grad's last vector");
            bad(grad_accum_plan(reinterpret_cast<char *>(acc) + (q.n * 4 - 1) / 16 * 16, acc, q.n, k0), "acc overlaps grad", "grad starts in acc's last vector");
        }
        // what the finish adds
        for (float sc : {0.f, -0.5f, nan, inf, -inf}) bad(grad_accum_finish_plan(g, acc, q.n, sc, nullptr, nullptr, k0), "scale=", "scale not finite or <= 0");
        bad(grad_accum_finish_plan(g, acc, q.n, 0.5f, sq, nullptr, k0), "sumsq without workspace", "sumsq without workspace");
        bad(grad_accum_finish_plan(g, acc, q.n, 0.5f, reinterpret_cast<float *>(reinterpret_cast<char *>(sq) + 2), w, k0), "sumsq must be 4-byte aligned", "misaligned sumsq");
        bad(grad_accum_finish_plan(g, acc, q.n, 0.5f, sq, w + 1, k0), "workspace must be 4-byte aligned", "misaligned workspace");
        bad(grad_accum_finish_plan(g, acc, q.n, 0.5f, acc, w, k0), "sumsq overlaps acc", "sumsq = acc");
        bad(grad_accum_finish_plan(g, acc, q.n, 0.5f, reinterpret_cast<float *>(g), w, k0), "sumsq overlaps grad", "sumsq = grad");
        bad(grad_accum_finish_plan(g, acc, q.n, 0.5f, acc + (q.n - 1), w, k0), "sumsq overlaps acc", "sumsq = acc's last element");
        bad(grad_accum_finish_plan(g, acc, q.n, 0.5f, sq, acc, k0), "workspace overlaps", "workspace = acc");     // 4 KiB from a small acc may reach a neighbouring block first
        bad(grad_accum_finish_plan(g, acc, q.n, 0.5f, sq, g, k0), "workspace overlaps grad", "workspace = grad");
        bad(grad_accum_finish_plan(g, acc, q.n, 0.5f, sq, g - (SFCVIT_SUMSQ_WORKSPACE_BYTES - 4), k0), "workspace overlaps grad", "workspace ends in grad's first word");
    }
}

// The plans of rowwise.cpp: which kernel, grid, LDS and workspace the LayerNorm, AdamW and column-sum shapes of the workloads
// and the edge shapes get, what the four switches change, and one refusal of each kind per entry point.  The plans read no
// pointer, so fake aligned ones serve.
static void check_rowwise() {
    using namespace sfcvit;
    const RowwiseKnobs k0;
    CHECK(k0.ln_cols == 1 && k0.ln_blocks == 0 && k0.ln_fwd_two_rows == 1 && k0.adamw_nt == 3, "rowwise: knob defaults");
    void *a = ptr(0), *b = ptr(1), *c = ptr(2), *d = ptr(3), *odd = static_cast<char *>(ptr(4)) + 8;
    float *f = static_cast<float *>(ptr(5)), *g = static_cast<float *>(ptr(6));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    auto refused = [](const PlanStatus &p, const char *frag, const char *what) {
        CHECK(p.err == SFCVIT_EINVAL && std::strstr(p.msg, frag), "rowwise %s: want '%s', got %d '%s'", what, frag, p.err, p.msg);
    };

    // LayerNorm backward, and its stochastic-depth twin: the same geometry, the ..._path_kernel names
    struct LB { int M, D; bool add; int ln_cols, ln_blocks; const char *name, *path_name; int blocks; };
    const LB lbs[] = {
        {50176, 768, true, 1, 0, "ln_bwd_cols_kernel<3, true>", "ln_bwd_cols_path_kernel<3, true>", 768},
        {36864, 1024, false, 1, 0, "ln_bwd_cols_kernel<4, false>", "ln_bwd_cols_path_kernel<4, false>", 512},
        {50176, 768, false, 0, 0, "ln_bwd_kernel<2, false>", "ln_bwd_path_kernel<2, false>", 512},
        {50176, 512, true, 1, 0, "ln_bwd_kernel<1, true>", "ln_bwd_path_kernel<1, true>", 512},
        {50176, 2048, false, 1, 0, "ln_bwd_kernel<4, false>", "ln_bwd_path_kernel<4, false>", 512},
        {10, 16, false, 1, 0, "ln_bwd_kernel<1, false>", "ln_bwd_path_kernel<1, false>", 3},
        {50176, 768, false, 1, 100, "ln_bwd_cols_kernel<3, false>", "ln_bwd_cols_path_kernel<3, false>", 100},
        {50176, 1032, false, 1, 0, "ln_bwd_kernel<4, false>", "ln_bwd_path_kernel<4, false>", 512},
    };
    for (const LB &q : lbs) {
        RowwiseKnobs k;
        k.ln_cols = q.ln_cols;
        k.ln_blocks = q.ln_blocks;
        const LnBwdPlan p = ln_bwd_plan(a, b, f, g, c, q.add ? d : nullptr, ptr(7), ptr(8), 0.1f, ptr(9), ptr(10), q.M, q.D, ptr(11), k);
        const LnBwdPlan pp = ln_bwd_path_plan(a, b, f, g, c, q.add ? d : nullptr, ptr(7), ptr(8), 0.1f, ptr(9), ptr(10), q.M / 2, 2, q.D,
                                              ptr(11), 0.5f, k);
        char name[96], path_name[96];
        kernel_name(p, false, name, sizeof(name));
        kernel_name(pp, true, path_name, sizeof(path_name));
        CHECK(p.err == SFCVIT_OK && pp.err == SFCVIT_OK, "ln_bwd %d %d refused: %s %s", q.M, q.D, p.msg, pp.msg);
        CHECK(!std::strcmp(name, q.name) && !std::strcmp(path_name, q.path_name), "ln_bwd %d %d: %s / %s", q.M, q.D, name, path_name);
        CHECK(p.blocks == q.blocks && p.M == q.M && p.D == q.D, "ln_bwd %d %d: %d workgroups, want %d", q.M, q.D, p.blocks, q.blocks);
        CHECK(p.lds == size_t(4) * 3 * q.D * 4 && p.ws_bytes == int64_t(q.blocks) * 3 * q.D * 4, "ln_bwd %d %d: lds %zu ws %lld", q.M, q.D,
              p.lds, (long long)p.ws_bytes);
        CHECK(pp.blocks == p.blocks && pp.lds == p.lds && pp.ws_bytes == p.ws_bytes && pp.M == p.M && pp.cols == p.cols && pp.inst == p.inst,
              "ln_bwd_path %d %d: geometry differs from ln_bwd's", q.M, q.D);
        CHECK(ln_bwd_geometry(q.M, q.D, false, k).ws_bytes == p.ws_bytes, "ln_bwd %d %d: the workspace query disagrees", q.M, q.D);
    }
    CHECK(ln_bwd_plan(a, b, f, g, c, d, ptr(7), ptr(8), 0.1f, ptr(9), ptr(10), 50176, 768, ptr(11), k0).lds == 36864, "ln_bwd: LDS at D 768");
    CHECK(ln_bwd_plan(a, b, f, g, c, nullptr, ptr(7), nullptr, nan, ptr(9), ptr(10), 8, 8, ptr(11), k0).err == SFCVIT_OK, "ln_bwd: p unused without dx_drop");
    refused(ln_bwd_plan(nullptr, b, f, g, c, d, ptr(7), ptr(8), 0.1f, ptr(9), ptr(10), 8, 8, ptr(11), k0), "null", "ln_bwd null dy");
    refused(ln_bwd_plan(a, b, f, g, c, d, ptr(7), ptr(8), 0.1f, ptr(9), ptr(10), 8, 8, nullptr, k0), "null", "ln_bwd null ws");
    refused(ln_bwd_plan(a, b, f, g, c, d, ptr(7), ptr(8), 0.1f, ptr(9), ptr(10), 8, 2056, ptr(11), k0), "D=2056", "ln_bwd D 2056");
    refused(ln_bwd_plan(a, b, f, g, c, d, ptr(7), ptr(8), 0.1f, ptr(9), ptr(10), 0, 8, ptr(11), k0), "M=0", "ln_bwd M 0");
    refused(ln_bwd_plan(a, b, f, g, c, d, ptr(7), ptr(8), 0.1f, ptr(9), ptr(10), 8, 12, ptr(11), k0), "D=12", "ln_bwd D 12");
    refused(ln_bwd_plan(a, b, f, g, c, odd, ptr(7), ptr(8), 0.1f, ptr(9), ptr(10), 8, 8, ptr(11), k0), "alignment", "ln_bwd dx_add");
    refused(ln_bwd_plan(a, b, f, g, c, d, ptr(7), ptr(8), 1.f, ptr(9), ptr(10), 8, 8, ptr(11), k0), "dropout p=1", "ln_bwd p 1");
    refused(ln_bwd_plan(a, b, f, g, c, d, ptr(7), ptr(8), nan, ptr(9), ptr(10), 8, 8, ptr(11), k0), "dropout p=", "ln_bwd p NaN");

    // LayerNorm forward
    struct LF { int M, D, two_rows_knob; bool two; int vpl, blocks; };
    const LF lfs[] = {{4096, 768, 1, true, 3, 512}, {4095, 768, 1, false, 2, 1024}, {4096, 768, 0, false, 2, 1024}, {50176, 1024, 1, true, 4, 6272},
                      {8192, 4096, 1, false, 8, 2048}, {8192, 512, 1, false, 1, 2048}, {5, 2048, 1, false, 4, 2}, {4097, 1024, 1, true, 4, 513}};
    for (const LF &q : lfs) {
        RowwiseKnobs k;
        k.ln_fwd_two_rows = q.two_rows_knob;
        const LnFwdPlan p = ln_fwd_plan(a, b, c, d, f, g, q.M, q.D, k);
        CHECK(p.err == SFCVIT_OK && p.two_rows == q.two && p.vpl == q.vpl && p.blocks == q.blocks, "ln_fwd %d %d: %s two %d vpl %d blocks %d",
              q.M, q.D, p.msg, int(p.two_rows), p.vpl, p.blocks);
    }
    refused(ln_fwd_plan(a, b, c, d, f, g, 8, 4104, k0), "D=4104", "ln_fwd D 4104");
    refused(ln_fwd_plan(a, b, c, d, f, g, -1, 8, k0), "M=-1", "ln_fwd M -1");
    refused(ln_fwd_plan(a, b, c, d, nullptr, g, 8, 8, k0), "null", "ln_fwd null mean");
    refused(ln_fwd_plan(a, odd, c, d, f, g, 8, 8, k0), "alignment", "ln_fwd gamma");
    {   // add_ln_path_plan takes the one-row form from the same helper
        int vpl = 0, blocks = 0;
        ln_fwd_rows(130, 768, vpl, blocks);
        const AddLnPathPlan p = add_ln_path_plan(a, b, c, d, ptr(7), ptr(8), f, g, 2, 65, 768, 0.1f);
        CHECK(p.err == SFCVIT_OK && p.vpl == vpl && p.blocks == blocks && vpl == 2 && blocks == 33, "add_ln_path: vpl %d blocks %d (%s)", p.vpl, p.blocks, p.msg);
    }

    // AdamW, and the same step with the EMA
    sfcvit_adamw_args aa{};
    auto far = [](int i) { return reinterpret_cast<float *>(uintptr_t(i + 1) << 36); };       // 64 GiB apart: no buffer reaches the next
    aa.param = far(0); aa.grad = far(1); aa.master = far(2); aa.m = far(3); aa.v = far(4);
    aa.lr = 3e-4f; aa.beta1 = 0.9f; aa.beta2 = 0.999f; aa.eps = 1e-8f; aa.grad_scale = 1.f; aa.step = 1;
    const sfcvit_ema_args ee{far(5), 0.9999f, 1};
    const int64_t per = 8 * ADAMW_THREADS;
    const struct { int64_t n; int grid; } grids[] = {{1, 1}, {per - 1, 1}, {per, 1}, {per + 1, 2}, {5 * per - 1, 5}, {5 * per, 5}, {5 * per + 1, 6},
                                                     {2047 * per, 2047}, {2047 * per + 1, 2048}, {2048 * per, 2048}, {2048 * per + 1, 2048},
                                                     {int64_t(2049) * 2048, 2048}};
    for (const auto &q : grids) {
        aa.n = q.n;
        const AdamwPlan p = adamw_plan(&aa, k0);
        CHECK(p.err == SFCVIT_OK && p.grid == q.grid && p.nt == 3, "adamw n %lld: grid %d, want %d (%s)", (long long)q.n, p.grid, q.grid, p.msg);
        const AdamwEmaPlan pe = adamw_ema_plan(&aa, &ee, k0);
        CHECK(pe.err == SFCVIT_OK && pe.grid == p.grid && pe.nt == p.nt, "adamw_ema n %lld: grid %d, adamw's %d (%s)", (long long)q.n, pe.grid, p.grid, pe.msg);
    }
    aa.n = 4096;
    const struct { int knob, nt; } nts[] = {{0, 0}, {1, 1}, {2, 2}, {3, 3}, {4, 0}, {7, 3}, {-1, 3}};
    for (const auto &q : nts) {
        RowwiseKnobs k;
        k.adamw_nt = q.knob;
        CHECK(adamw_plan(&aa, k).nt == q.nt && adamw_ema_plan(&aa, &ee, k).nt == q.nt, "adamw_nt %d: want %d", q.knob, q.nt);
    }
    refused(adamw_plan(nullptr, k0), "null", "adamw null a");
    { sfcvit_adamw_args x = aa; x.m = nullptr; refused(adamw_plan(&x, k0), "null", "adamw null m"); }
    { sfcvit_adamw_args x = aa; x.n = 0; refused(adamw_plan(&x, k0), "n=0", "adamw n 0"); }
    { sfcvit_adamw_args x = aa; x.step = 0; refused(adamw_plan(&x, k0), "step=0", "adamw step 0"); float st[8] = {}; x.dev_state = st;
      CHECK(adamw_plan(&x, k0).err == SFCVIT_OK, "adamw: step 0 with dev_state refused"); }
    { sfcvit_adamw_args x = aa; x.grad = odd; refused(adamw_plan(&x, k0), "aligned", "adamw grad"); }

    // column sums
    const struct { int M, N, cb, rb, rpb; } cs[] = {{50176, 768, 3, 251, 200}, {50176, 2304, 9, 112, 448}, {8, 8, 1, 1, 8}};
    for (const auto &q : cs) {
        const int64_t ws = int64_t(q.rb) * q.N * 4;
        const ColsumPlan p = colsum_plan(a, q.M, q.N, q.N, b, c, ws);
        CHECK(p.err == SFCVIT_OK && p.col_blocks == q.cb && p.row_blocks == q.rb && p.rpb == q.rpb && p.ws_bytes == ws,
              "colsum %d %d: (%d, %d, %d) ws %lld %s", q.M, q.N, p.col_blocks, p.row_blocks, p.rpb, (long long)p.ws_bytes, p.msg);
        CHECK(int64_t(p.rpb) * p.row_blocks >= q.M && p.rpb % 8 == 0 && colsum_geometry(q.M, q.N).ws_bytes == ws, "colsum %d %d: cover", q.M, q.N);
        refused(colsum_plan(a, q.M, q.N, q.N, b, c, ws - 1), "workspace", "colsum workspace one byte short");
    }
    refused(colsum_plan(a, 8, 8, 8, b, nullptr, 1 << 20), "workspace", "colsum null workspace");
    refused(colsum_plan(nullptr, 8, 8, 8, b, c, 1 << 20), "null", "colsum null x");
    refused(colsum_plan(a, 8, 12, 16, b, c, 1 << 20), "N=12", "colsum N 12");
    refused(colsum_plan(a, 8, 16, 8, b, c, 1 << 20), "ld=8", "colsum ld < N");
    refused(colsum_plan(odd, 8, 8, 8, b, c, 1 << 20), "alignment", "colsum x");

    // the entry points whose plan is refusals + a grid
    { const RowGridPlan p = transpose_plan(a, 768, 2304, 2304, b, 768); CHECK(p.err == SFCVIT_OK && p.grid == 36 && p.grid_y == 12, "transpose grid"); }
    { const RowGridPlan p = transpose_plan(a, 8, 72, 72, b, 8); CHECK(p.err == SFCVIT_OK && p.grid == 2 && p.grid_y == 1, "transpose 8 x 72 grid"); }
    refused(transpose_plan(a, 8, 8, 8, nullptr, 8), "null", "transpose null dst");
    refused(transpose_plan(a, 8, 12, 16, b, 8), "C=12", "transpose C 12");
    refused(transpose_plan(a, 16, 8, 8, b, 8), "ldd=8", "transpose ldd < R");
    refused(transpose_plan(odd, 8, 8, 8, b, 8), "alignment", "transpose src");
    CHECK(transpose_batched_plan(a, b, c, 77).grid == 77, "transpose_batched grid");
    refused(transpose_batched_plan(a, b, nullptr, 4), "null", "transpose_batched null tiles");
    refused(transpose_batched_plan(a, b, c, 0), "no tiles", "transpose_batched no tiles");
    refused(transpose_batched_plan(a, odd, c, 4), "alignment", "transpose_batched dst");
    CHECK(gelu_plan(false, nullptr, a, b, 8).err == SFCVIT_OK && gelu_plan(true, a, b, c, int64_t(50176) * 3072).err == SFCVIT_OK, "gelu refused");
    refused(gelu_plan(false, nullptr, a, b, 12), "gelu_fwd: n=12", "gelu_fwd n 12");
    refused(gelu_plan(false, nullptr, nullptr, b, 8), "gelu_fwd", "gelu_fwd null x");
    refused(gelu_plan(true, nullptr, a, b, 8), "gelu_bwd", "gelu_bwd null dy");
    refused(gelu_plan(true, a, b, c, 0), "gelu_bwd: n=0", "gelu_bwd n 0");
    CHECK(gelu_drop_plan(false, nullptr, a, b, 37, 264, 0.1f).err == SFCVIT_OK && gelu_drop_plan(true, a, b, c, 50176, 3072, 0.f).err == SFCVIT_OK, "gelu_drop refused");
    refused(gelu_drop_plan(true, nullptr, a, b, 8, 8, 0.1f), "gelu_drop_bwd: null", "gelu_drop_bwd null dy");
    refused(gelu_drop_plan(false, nullptr, a, nullptr, 8, 8, 0.1f), "gelu_drop_fwd: rows=8", "gelu_drop_fwd null y");
    refused(gelu_drop_plan(false, nullptr, a, b, 8, 12, 0.1f), "cols=12", "gelu_drop_fwd cols 12");
    refused(gelu_drop_plan(true, a, b, c, 8, 8, 1.f), "gelu_drop_bwd: dropout p=1", "gelu_drop_bwd p 1");
    refused(gelu_drop_plan(false, nullptr, a, b, 8, 8, nan), "dropout p=", "gelu_drop_fwd p NaN");
    CHECK(dropout_mask_plan(a, 5, 7, 0.5f).err == SFCVIT_OK && dropout_mask_plan(a, 300, 5, 0.f).err == SFCVIT_OK, "dropout_mask refused");
    refused(dropout_mask_plan(nullptr, 5, 7, 0.5f), "bad argument", "dropout_mask null out");
    refused(dropout_mask_plan(a, 0, 7, 0.5f), "bad argument", "dropout_mask rows 0");
    refused(dropout_mask_plan(a, 5, 7, 1.f), "bad argument", "dropout_mask p 1");
    CHECK(soft_ce_plan(a, f, g, 256, 1000, 1024).grid == 64 && soft_ce_plan(a, f, g, 5, 10, 10).grid == 2, "soft_ce grid");
    refused(soft_ce_plan(a, nullptr, g, 8, 8, 8), "null", "soft_ce null targets");
    refused(soft_ce_plan(a, f, g, 8, 16, 8), "ld=8", "soft_ce ld < C");
    static_assert(SFCVIT_SUMSQ_WORKSPACE_BYTES / 4 < ADAMW_MAX_BLOCKS, "the workspace, not the grid cap, bounds the sumsq grid");
    const struct { int64_t n; int grid; } sq[] = {{1, 1}, {per, 1}, {per + 1, 2}, {1023 * per, 1023}, {1023 * per + 1, 1024}, {1024 * per + 1, 1024},
                                                  {int64_t(86567656), SFCVIT_SUMSQ_WORKSPACE_BYTES / 4}};
    for (const auto &q : sq) {
        const RowGridPlan p = sumsq_plan(a, q.n, f, b);
        CHECK(p.err == SFCVIT_OK && p.grid == q.grid, "sumsq n %lld: grid %d, want %d (%s)", (long long)q.n, p.grid, q.grid, p.msg);
    }
    refused(sumsq_plan(a, 0, f, b), "bad argument", "sumsq n 0");
    refused(sumsq_plan(a, 8, f, nullptr), "bad argument", "sumsq null workspace");
    refused(sumsq_plan(odd, 8, f, b), "alignment", "sumsq g");
    CHECK(step_advance_plan(a).err == SFCVIT_OK && step_advance_plan(a).grid == 1, "step_advance");
    refused(step_advance_plan(nullptr), "16-byte aligned", "step_advance null state");
    refused(step_advance_plan(odd), "16-byte aligned", "step_advance state");
}

// The plans of tokenizer.cpp: form, grid, LDS and workspace of the token gathers, the fused patch embedding (generic and
// tiled), the hierarchical tokenizer, the resampling concatenation and the two mix entry points at the benchmark shapes and at
// every form boundary; every refusal with its text; the proof that the tiled forms never need more workspace than
// sfcvit_patch_embed_workspace reports; and extents no tensor can have, so that UBSan sees the arithmetic.  Expected values are
// the parent commit's (its library's answers to the queries, its formulas evaluated by hand for the grids).
static std::vector<int32_t> tile_class_counts(int curve, int img) {
    const int N = img * img / 256, cap = 16 + 2 * N + 2 * 8 * 256;
    std::unique_ptr<int32_t[]> flat(new int32_t[img * img]), pix(new int32_t[img * img]), desc(new int32_t[cap]);
    CHECK(sfcvit_curve_table(curve, img, flat.get()) == SFCVIT_OK && sfcvit_pixel_table(flat.get(), img, 1, 256, pix.get()) == SFCVIT_OK,
          "tokenizer: tables of %d px", img);
    CHECK(sfcvit_tile_descriptors(pix.get(), N, 256, img, desc.get(), cap) > 0, "tokenizer: %d px is not tiles", img);
    std::vector<int32_t> cnt;
    for (int c = 0; c < desc[1]; c++) cnt.push_back(desc[6 + c + 1] - desc[6 + c]);
    return cnt;
}

static void check_tokenizer() {
    using namespace sfcvit;
    const TokenizerKnobs k0;
    CHECK(k0.gather_u == 1 && k0.gather_nt == 3, "tokenizer: knob defaults");
    void *a = ptr(0), *b = ptr(1), *odd = static_cast<char *>(ptr(4)) + 8, *odd4 = static_cast<char *>(ptr(4)) + 4;
    const int32_t *ia = static_cast<const int32_t *>(ptr(2)), *ib = static_cast<const int32_t *>(ptr(3)), *ic = static_cast<const int32_t *>(ptr(5));
    const uint32_t *rec = static_cast<const uint32_t *>(ptr(6));
    const int big = INT32_MAX;
    auto refused = [](const PlanStatus &p, const char *frag, const char *what) {
        CHECK(p.err == SFCVIT_EINVAL && std::strstr(p.msg, frag), "tokenizer %s: want '%s', got %d '%s'", what, frag, p.err, p.msg);
    };
    auto named = [](const auto &p, const char *want, const char *what) {
        char name[96];
        kernel_name(p, name, sizeof(name));
        CHECK(p.err == SFCVIT_OK && !std::strcmp(name, want), "tokenizer %s: '%s', want '%s' (%s)", what, name, want, p.msg);
    };

    // ---- token gathers ----
    auto tiles = [&](int B, int C, int H, int W, int N, int ld, const int32_t *perm, const TokenizerKnobs &k) {
        return gather_tiles_plan("tokens_gather_tiles", a, ia, ib, perm, B, C, H, W, N, b, ld, k);
    };
    {   // the benchmark shapes: ViT-B/16 at 224 with 256 images, ViT-L at 384 with 64
        const GatherPlan p = tiles(256, 3, 224, 224, 196, 768, nullptr, k0);
        named(p, "tokens_gather_tiles_kernel<3, fp32>", "tiles ViT-B");
        CHECK(p.form == GatherForm::TILES && p.grid_x == 98 && p.grid_y == 64 && p.threads == 256 && p.lds == 13312 && p.upw == 1 && p.nt == 3 &&
              p.HW == 50176 && p.wmagic == uint32_t((uint64_t(1) << 32) / 224) + 1, "tiles ViT-B: grid (%d, %d) lds %zu", p.grid_x, p.grid_y, p.lds);
        const GatherPlan l = tiles(64, 3, 384, 384, 576, 768, nullptr, k0);
        CHECK(l.err == SFCVIT_OK && l.grid_x == 288 && l.grid_y == 16 && l.lds == 13312, "tiles ViT-L: grid (%d, %d)", l.grid_x, l.grid_y);
        TokenizerKnobs k2;
        k2.gather_u = 2;
        const GatherPlan u = tiles(256, 3, 224, 224, 196, 768, nullptr, k2);
        CHECK(u.err == SFCVIT_OK && u.upw == 2 && u.grid_y == 32 && u.lds == 1024 + 8 * 3 * 1024, "tiles U = 2: grid y %d lds %zu", u.grid_y, u.lds);
        const GatherPlan m = gather_mix_plan(a, ia, ib, ic, rec, 256, 3, 224, 224, 196, 256, b, 768, k2);
        named(m, "tokens_gather_tiles_kernel<3, mix>", "tiles ViT-B mix");
        CHECK(m.mix && m.upw == 1 && m.grid_x == 98 && m.grid_y == 64 && m.lds == 13312, "tiles mix: upw %d grid y %d", m.upw, m.grid_y);
        const struct { int knob, u; } us[] = {{1, 1}, {2, 2}, {0, 1}, {3, 1}, {-2, 1}};
        for (const auto &q : us) { TokenizerKnobs k; k.gather_u = q.knob; CHECK(tiles(8, 1, 16, 16, 1, 256, nullptr, k).upw == q.u, "gather_u %d", q.knob); }
        const struct { int knob, nt; } nts[] = {{0, 0}, {1, 1}, {2, 2}, {3, 3}, {4, 0}, {-1, 0}, {7, 0}};
        for (const auto &q : nts) { TokenizerKnobs k; k.gather_nt = q.knob; CHECK(tiles(8, 1, 16, 16, 1, 256, nullptr, k).nt == q.nt, "gather_nt %d", q.knob); }
        for (int C = 1; C <= 4; C++) {
            const GatherPlan ok = tiles(5, C, 32, 24, 3, 256 * C, nullptr, k0);
            CHECK(ok.err == SFCVIT_OK && ok.C == C && ok.grid_x == 2 && ok.grid_y == 2 && ok.lds == size_t(1024 + 4 * C * 1024), "tiles C %d", C);
        }
    }
    refused(gather_tiles_plan("tokens_gather_tiles", nullptr, ia, ib, nullptr, 1, 3, 32, 32, 4, b, 768, k0), "tokens_gather_tiles: null pointer", "tiles null x");
    refused(gather_tiles_plan("tokens_gather_tiles", a, ia, nullptr, nullptr, 1, 3, 32, 32, 4, b, 768, k0), "tokens_gather_tiles: null pointer", "tiles null origin");
    refused(gather_tiles_plan("tokens_gather_tiles", a, nullptr, ib, nullptr, 1, 3, 32, 32, 4, b, 768, k0), "null pointer", "tiles null pix");
    refused(gather_tiles_plan("tokens_gather_tiles", a, ia, ib, nullptr, 1, 3, 32, 32, 4, nullptr, 768, k0), "null pointer", "tiles null tokens");
    refused(tiles(0, 3, 32, 32, 4, 768, nullptr, k0), "B=0 C=3 H=32 W=32 N=4 (1 <= C <= 4", "tiles B 0");
    refused(tiles(1, 5, 32, 32, 4, 1280, nullptr, k0), "C=5", "tiles C 5");
    refused(tiles(1, 0, 32, 32, 4, 0, nullptr, k0), "C=0", "tiles C 0");
    refused(tiles(1, 3, 32, 36, 4, 768, nullptr, k0), "W=36", "tiles W % 8");
    refused(tiles(1, 3, 24, 32, 3, 768, nullptr, k0), "H=24", "tiles H % 16");
    refused(tiles(1, 3, 32, 32, 5, 768, nullptr, k0), "N=5", "tiles N");
    refused(tiles(1, 3, 32, 32, 4, 512, nullptr, k0), "ld=512 (must be 256 * C = 768)", "tiles ld");
    refused(gather_tiles_plan("tokens_gather_tiles", odd, ia, ib, nullptr, 1, 3, 32, 32, 4, b, 768, k0), "x and tokens must be 16-byte aligned", "tiles x");
    refused(gather_tiles_plan("tokens_gather_tiles", a, ia, ib, nullptr, 1, 3, 32, 32, 4, odd, 768, k0), "x and tokens must be 16-byte aligned", "tiles tokens");
    refused(tiles(1, 1, 16, 16384, 1024, 256, nullptr, k0), "W=16384 too wide", "tiles W 16384");          // 16 W W = 2^32
    CHECK(tiles(1, 1, 32, 16376, 2047, 256, nullptr, k0).err == SFCVIT_OK, "tiles W 16376 refused");       // the widest W % 8 == 0 below it
    refused(tiles(65535 * 4 + 1, 1, 16, 16, 1, 256, nullptr, k0), "batch 262141 too large", "tiles grid y");
    CHECK(tiles(65535 * 4, 1, 16, 16, 1, 256, nullptr, k0).grid_y == 65535, "tiles grid y 65535");
    refused(tiles(65535 * 8, 1, 16, 16, 1, 256, nullptr, k0), "too large", "tiles B 65535 * 8");
    refused(tiles(1, 1, 1 << 20, 8192, 1 << 25, 256, nullptr, k0), "H * W must fit 31 bits", "tiles H * W = 2^33");     // was an int product
    refused(tiles(big, 1, 16, 16, 1, 256, nullptr, k0), "too large", "tiles B max");
    refused(tiles(1, 1, big, big, big, 256, nullptr, k0), "tokens_gather_tiles: B=1", "tiles H W N max");
    refused(tiles(1, big, 16, 16, 1, 256, nullptr, k0), "C=2147483647", "tiles C max");

    auto rows = [&](int x_bf16, int B, int C, int HW, int N, int P, int ld, const int32_t *perm = nullptr) {
        return gather_plan(perm ? "tokens_gather_mix" : "tokens_gather", a, x_bf16, ia, perm, B, C, HW, N, P, b, ld);
    };
    {   // form boundaries
        const GatherPlan p = rows(0, 9, 4, 1024, 4, 256, 1024);                // 2 * 8 * 1024 * 2 = 32 KiB
        named(p, "tokens_gather_p256_kernel<fp32>", "P 256 C 4");
        CHECK(p.form == GatherForm::P256 && p.lds == 32768 && p.grid_x == 2 && p.grid_y == 2 && p.threads == 512, "P 256 C 4: lds %zu", p.lds);
        const GatherPlan e = rows(1, 9, 4, 1024, 4, 256, 2048);                // 64 KiB: the last ld of this form
        named(e, "tokens_gather_p256_kernel<bf16>", "ld 2048");
        CHECK(e.lds == 65536, "ld 2048: lds %zu", e.lds);
        const GatherPlan r = rows(0, 9, 4, 1024, 4, 256, 2056);                // the first ld above 2048 halfwords
        named(r, "tokens_gather_kernel<fp32>", "ld 2056");
        CHECK(r.form == GatherForm::ROWS && r.lds == 4112 && r.grid_x == 4 && r.grid_y == 2 && r.threads == 256, "ld 2056: lds %zu", r.lds);
        named(rows(0, 1, 3, 1028, 4, 257, 776), "tokens_gather_kernel<fp32>", "P 257");
        named(rows(1, 1, 5, 1024, 4, 256, 1280), "tokens_gather_kernel<bf16>", "C 5");
        named(rows(0, 1, 5, 1024, 4, 256, 1280, ic), "tokens_gather_kernel<mix>", "C 5 mix");
        named(rows(0, 1, 3, 1024, 64, 16, 48, ic), "tokens_gather_p256_kernel<mix>", "P 16 mix");
        // a bf16 image with a tile table goes to sfcvit_tokens_gather (Python decides): ViT-B
        const GatherPlan v = rows(1, 256, 3, 50176, 196, 256, 768);
        named(v, "tokens_gather_p256_kernel<bf16>", "ViT-B bf16");
        CHECK(v.grid_x == 98 && v.grid_y == 32 && v.lds == 24576, "ViT-B bf16: grid (%d, %d) lds %zu", v.grid_x, v.grid_y, v.lds);
        const GatherPlan m = gather_mix_plan(a, ia, nullptr, ic, rec, 9, 3, 32, 32, 64, 16, b, 48, k0);
        named(m, "tokens_gather_p256_kernel<mix>", "mix without origin");
        CHECK(m.HW == 1024 && m.grid_x == 32 && m.grid_y == 2, "mix without origin: HW %d", m.HW);
    }
    refused(gather_plan("tokens_gather", nullptr, 0, ia, nullptr, 1, 3, 1024, 64, 16, b, 48), "tokens_gather: null pointer", "gather null x");
    refused(gather_plan("tokens_gather", a, 0, nullptr, nullptr, 1, 3, 1024, 64, 16, b, 48), "tokens_gather: null pointer", "gather null pix");
    refused(gather_plan("tokens_gather", a, 0, ia, nullptr, 1, 3, 1024, 64, 16, nullptr, 48), "tokens_gather: null pointer", "gather null tokens");
    refused(rows(0, 0, 3, 1024, 64, 16, 48), "B=0 C=3 HW=1024 N=64 P=16 (N * P must equal H * W)", "gather B 0");
    refused(rows(0, 1, 3, 1024, 64, 15, 48), "P=15", "gather N * P");
    refused(rows(0, 1, 0, 1024, 64, 16, 48), "C=0", "gather C 0");
    refused(rows(0, 1, 3, 1024, 64, 16, 40), "ld=40 (>= P * C = 48, multiple of 8, <= 32768)", "gather ld < K");
    refused(rows(0, 1, 3, 1024, 64, 16, 52), "ld=52", "gather ld % 8");
    refused(rows(0, 1, 1, 32776, 1, 32776, 32776), "ld=32776", "gather ld > 32768");
    refused(gather_plan("tokens_gather", a, 0, ia, nullptr, 1, 3, 1024, 64, 16, odd, 48), "tokens must be 16-byte aligned", "gather tokens");
    CHECK(gather_plan("tokens_gather", odd4, 0, ia, nullptr, 1, 3, 1024, 64, 16, b, 48).err == SFCVIT_OK, "gather: x needs no alignment");
    refused(rows(0, 65535 * 8 + 1, 3, 1024, 64, 16, 48), "batch 524281 too large", "gather grid y");
    CHECK(rows(0, 65535 * 8, 3, 1024, 64, 16, 48).grid_y == 65535, "gather B 65535 * 8");
    refused(rows(0, big, 3, 1024, 64, 16, 48), "too large", "gather B max");
    refused(rows(0, 1, big, big, 1, big, 32768), "P * C = 4611686014132420609", "gather P C max");        // was an int product
    {
        const GatherPlan p = gather_plan("tokens_gather", a, 0, ia, nullptr, 8, 1, big, big, 1, b, 8);    // N = HW = INT32_MAX, one pixel per token
        CHECK(p.err == SFCVIT_OK && p.form == GatherForm::P256 && p.grid_x == (1 << 30) && p.grid_y == 1, "gather N max: grid x %d", p.grid_x);
    }
    refused(gather_mix_plan(a, ia, nullptr, nullptr, rec, 1, 3, 32, 32, 64, 16, b, 48, k0), "tokens_gather_mix: null perm / rec", "mix null perm");
    refused(gather_mix_plan(a, ia, nullptr, ic, nullptr, 1, 3, 32, 32, 64, 16, b, 48, k0), "tokens_gather_mix: null perm / rec", "mix null rec");
    refused(gather_mix_plan(a, ia, nullptr, ic, rec, 1, 3, 0, 32, 64, 16, b, 48, k0), "tokens_gather_mix: H=0 W=32", "mix H 0");
    refused(gather_mix_plan(a, ia, nullptr, ic, rec, 1, 3, 65536, 32768, 64, 16, b, 48, k0), "tokens_gather_mix: H=65536 W=32768", "mix H W = 2^31");
    refused(gather_mix_plan(a, ia, nullptr, ic, rec, 1, 3, big, big, 64, 16, b, 48, k0), "tokens_gather_mix: H=2147483647", "mix H W max");
    refused(gather_mix_plan(odd, ia, nullptr, ic, rec, 1, 3, 32, 32, 64, 16, b, 48, k0), "tokens_gather_mix: x must be 16-byte aligned", "mix x");
    refused(gather_mix_plan(a, ia, ib, ic, rec, 1, 3, 32, 32, 64, 16, b, 48, k0), "P=16 with a tile origin table", "mix P with origin");
    refused(gather_mix_plan(a, ia, ib, ic, rec, 1, 3, 32, 32, 4, 256, b, 512, k0), "tokens_gather_mix: ld=512", "mix tiles ld");
    refused(gather_mix_plan(a, ia, ib, ic, rec, 1, 5, 32, 32, 4, 256, b, 1280, k0), "tokens_gather_mix: B=1 C=5", "mix tiles C 5");
    refused(gather_mix_plan(a, ia, nullptr, ic, rec, 1, 3, 32, 32, 64, 15, b, 48, k0), "tokens_gather_mix: B=1 C=3 HW=1024 N=64 P=15", "mix N * P");
    refused(gather_mix_plan(nullptr, ia, nullptr, ic, rec, 1, 3, 32, 32, 64, 16, b, 48, k0), "tokens_gather_mix: null pointer", "mix null x");

    // ---- patch embedding ----
    auto pe_args = [&](int B, int C, int N, int P, int D, const std::vector<int32_t> &cnt) {
        sfcvit_patch_embed_args q{};
        q.x = a; q.pix = ia; q.w = ptr(7); q.bias = ptr(8); q.y = b; q.dw = ptr(9); q.dbias = ptr(10); q.workspace = ptr(11);
        q.workspace_bytes = INT64_MAX;
        q.B = B; q.C = C; q.N = N; q.P = P; q.D = D; q.HW = int(int64_t(N) * P);
        if (!cnt.empty()) { q.desc = ib; q.desc_ncls = int(cnt.size()); for (size_t c = 0; c < cnt.size() && c < 8; c++) q.desc_cnt[c] = cnt[c]; }
        return q;
    };
    {   // the benchmark shapes with the class counts of the real Hilbert tables
        const std::vector<int32_t> cb = tile_class_counts(SFCVIT_CURVE_HILBERT, 224), cl = tile_class_counts(SFCVIT_CURVE_HILBERT, 384);
        CHECK(cb == std::vector<int32_t>({49, 52, 49, 46}) && cl == std::vector<int32_t>({148, 144, 140, 144}), "hilbert class counts");
        struct S { int B, N, D; const std::vector<int32_t> &cnt; int n_row_tiles, grid_f, KR, nz, grid_b; int64_t ws_f, ws_b, tiled_b; };
        const S shapes[] = {{256, 196, 768, cb, 392, 1176, 2240, 24, 216, 9437184, 68419584, 56623104},
                            {64, 576, 1024, cl, 288, 1152, 2368, 16, 192, 12582912, 69206016, 50331648}};
        for (const S &q : shapes) {
            sfcvit_patch_embed_args x = pe_args(q.B, 3, q.N, 256, q.D, q.cnt);
            CHECK(patch_embed_geometry(q.B, 3, q.N, 256, q.D, false).ws_bytes == q.ws_f && patch_embed_geometry(q.B, 3, q.N, 256, q.D, true).ws_bytes == q.ws_b &&
                  pe2_bwd_workspace(3, q.D) == q.tiled_b, "patch embed D %d: workspaces", q.D);
            x.workspace_bytes = q.ws_f;
            const PatchEmbedPlan f = patch_embed_plan(&x, false);
            named(f, "pe2_fwd_kernel<fp32>", "tiled forward");
            CHECK(f.form == PeForm::TILED && f.n_row_tiles == q.n_row_tiles && f.groups == q.n_row_tiles / 8 && f.grid == q.grid_f && f.lds == 100352 &&
                  f.permute_grid == 1024 && f.wp_bytes == int64_t(4) * q.D * 768 * 2 && f.ws_bytes == q.ws_f && f.M == q.B * q.N && f.Kp == 768,
                  "tiled forward D %d: row tiles %d grid %d lds %zu", q.D, f.n_row_tiles, f.grid, f.lds);
            x.workspace_bytes = q.ws_f - 1;
            refused(patch_embed_plan(&x, false), "patch_embed_fwd: workspace of", "forward workspace one byte short");
            x.workspace_bytes = q.ws_b;
            x.x_is_bf16 = 1;
            const PatchEmbedPlan g = patch_embed_plan(&x, true);
            named(g, "pe2_bwd_kernel<bf16>", "tiled backward");
            CHECK(g.form == PeForm::TILED && g.KR == q.KR && g.nz == q.nz && g.grid == q.grid_b && g.lds == 131072 && g.dbias &&
                  g.slab_bytes == int64_t(q.nz) * q.D * 768 * 4 && g.slab_bytes <= q.tiled_b && g.reduce_grid == q.D * 3 && g.ws_bytes == q.ws_b,
                  "tiled backward D %d: KR %d nz %d grid %d", q.D, g.KR, g.nz, g.grid);
            x.workspace_bytes = q.ws_b - 1;
            refused(patch_embed_plan(&x, true), "patch_embed_bwd: workspace of", "backward workspace one byte short");
            // without the descriptor: the generic kernels at the same shape
            sfcvit_patch_embed_args y = pe_args(q.B, 3, q.N, 256, q.D, {});
            const PatchEmbedPlan gf = patch_embed_plan(&y, false), gb = patch_embed_plan(&y, true);
            named(gf, "pe_fwd_kernel<fp32>", "generic forward");
            named(gb, "pe_bwd_kernel<fp32>", "generic backward");
            const int tiles_d = q.D / 128, M = q.B * q.N, splits = (1024 + tiles_d * 6 - 1) / (tiles_d * 6), mps = ((M / 64 + splits - 1) / splits) * 64;
            CHECK(gf.form == PeForm::GENERIC && gf.grid == tiles_d * (M / 128) && gf.lds == 65536 && gf.permute_grid == q.D * 3 && gf.wp_bytes == int64_t(q.D) * 768 * 2,
                  "generic forward D %d: grid %d", q.D, gf.grid);
            CHECK(gb.splits == splits && gb.m_per_split == mps && gb.zs == (M + mps - 1) / mps && gb.grid == 6 * tiles_d * gb.zs && gb.lds == 65536 &&
                  gb.reduce_grid == q.D * 48 && gb.slab_bytes == int64_t(splits) * q.D * 768 * 4, "generic backward D %d: splits %d zs %d", q.D, gb.splits, gb.zs);
        }
        // form boundaries, forward and backward alike
        struct F { int C, N, P, D, HW; int ncls; bool tiled; };
        const F forms[] = {{3, 196, 256, 512, 50176, 4, true}, {3, 196, 256, 384, 50176, 4, false}, {3, 784, 64, 768, 50176, 4, false},
                           {3, 196, 256, 768, 50176, 0, false}, {3, 196, 256, 768, 50176, 9, false}, {3, 196, 256, 768, 50176, 8, true},
                           {1, 1, 256, 256, 256, 1, true}};
        for (const F &q : forms)
            for (int bwd = 0; bwd < 2; bwd++) {
                sfcvit_patch_embed_args x = pe_args(4, q.C, q.N, q.P, q.D, std::vector<int32_t>(q.ncls > 0 ? q.ncls : 1, q.N / (q.ncls > 0 ? q.ncls : 1)));
                x.desc_ncls = q.ncls;
                const PatchEmbedPlan p = patch_embed_plan(&x, bwd);
                CHECK(p.err == SFCVIT_OK && (p.form == PeForm::TILED) == q.tiled, "patch embed P %d D %d ncls %d: form (%s)", q.P, q.D, q.ncls, p.msg);
            }
        {   // H * W % 8 != 0 with P = 256 never reaches the choice of form: N * P == H * W is refused first
            sfcvit_patch_embed_args x = pe_args(4, 3, 196, 256, 768, cb);
            x.HW = 50180;
            refused(patch_embed_plan(&x, false), "N*P=50176 must equal H*W=50180", "HW % 8");
        }
    }
    {   // the query: the parent's values, and 0 where there is no such shape
        const struct { int B, C, N, P, D; int64_t f, b; } ws[] = {{256, 3, 196, 256, 512, 6291456, 67633152}, {256, 3, 196, 256, 384, 4718592, 67239936},
            {128, 3, 64, 16, 256, 196608, 6291456}, {8, 3, 16, 64, 192, 589824, 294912}, {2, 1, 27, 27, 104, 53248, 13312}, {4, 3, 4, 256, 256, 3145728, 62914560},
            {1, 1, 1, 1, 8, 1024, 256}, {256, 3, 784, 64, 768, 2359296, 50724864}, {3, 4, 9, 256, 1280, 20971520, 41943040}, {512, 3, 4, 256, 2048, 25165824, 69206016}};
        for (const auto &q : ws)
            CHECK(patch_embed_geometry(q.B, q.C, q.N, q.P, q.D, false).ws_bytes == q.f && patch_embed_geometry(q.B, q.C, q.N, q.P, q.D, true).ws_bytes == q.b,
                  "workspace %d %d %d %d %d: %lld / %lld", q.B, q.C, q.N, q.P, q.D, (long long)patch_embed_geometry(q.B, q.C, q.N, q.P, q.D, false).ws_bytes,
                  (long long)patch_embed_geometry(q.B, q.C, q.N, q.P, q.D, true).ws_bytes);
        for (int bwd = 0; bwd < 2; bwd++) {
            CHECK(!patch_embed_geometry(0, 3, 4, 256, 256, bwd).ws_bytes && !patch_embed_geometry(1, -3, 4, 256, 256, bwd).ws_bytes &&
                  !patch_embed_geometry(1, 3, 0, 256, 256, bwd).ws_bytes && !patch_embed_geometry(1, 3, 4, 0, 256, bwd).ws_bytes &&
                  !patch_embed_geometry(1, 3, 4, 256, -8, bwd).ws_bytes, "workspace of a non-positive dimension");
            // extents no tensor can have: singly and in pairs
            const int v[] = {1, 8, big};
            for (int B : v) for (int C : v) for (int N : v) for (int P : v) for (int D : v) {
                const int64_t w = patch_embed_geometry(B, C, N, P, D, bwd).ws_bytes;
                CHECK(w >= 0, "workspace %d %d %d %d %d negative", B, C, N, P, D);
                sfcvit_patch_embed_args x = pe_args(B, C, N, P, D == big ? big - 7 : D, {4});
                x.HW = int64_t(N) * P > big ? big : int(int64_t(N) * P);
                const PatchEmbedPlan p = patch_embed_plan(&x, bwd);
                CHECK(p.err == SFCVIT_OK || p.err == SFCVIT_EINVAL, "patch embed extents");
            }
        }
        sfcvit_patch_embed_args x = pe_args(1, big, 1, 8, 8, {});
        refused(patch_embed_plan(&x, false), "patch_embed_fwd: C*P=17179869176 D=8 too large", "C * P past int");          // was an int product
        x = pe_args(1, 1 << 20, 1, 1 << 10, big - 7, {});
        refused(patch_embed_plan(&x, true), "patch_embed_bwd: C*P=1073741824 D=2147483640 too large", "D * Kp past 2^35");
        x = pe_args(1 << 15, 1, (1 << 15) - 1, 8, 1 << 16, {});               // 2^9 x (2^23 - 2^8) tiles
        refused(patch_embed_plan(&x, false), "too many workgroups", "forward grid past int");                              // was an int product
        CHECK(patch_embed_plan(&x, true).err == SFCVIT_OK, "backward at that shape refused");
    }
    {   // the two dead fall-backs: whatever the class counts, the tiled forms need no more than the query reports
        uint32_t rng = 12345;
        auto next = [&](uint32_t n) { rng = rng * 1664525u + 1013904223u; return (rng >> 8) % n; };
        for (int it = 0; it < 4000; it++) {
            const int C = 1 + int(next(4)), D = 256 * (1 + int(next(it % 8 ? 8 : 40))), ncls = 1 + int(next(8));
            const int N = ncls + int(next(it % 3 ? 64 : 1100)), B = 1 + int(next(it % 5 ? 16 : 600));
            std::vector<int32_t> cnt(ncls, 1);
            for (int left = N - ncls; left > 0;) { const int take = 1 + int(next(left)); cnt[next(ncls)] += take; left -= take; }
            sfcvit_patch_embed_args x = pe_args(B, C, N, 256, D, cnt);
            const PatchEmbedPlan f = patch_embed_plan(&x, false), g = patch_embed_plan(&x, true);
            const int tiles = (D / 256) * C, G = 8 * (32 / tiles > 1 ? 32 / tiles : 1);
            CHECK(f.err == SFCVIT_OK && f.form == PeForm::TILED && f.wp_bytes == int64_t(ncls) * D * C * 256 * 2 && f.wp_bytes <= f.ws_bytes &&
                  f.ws_bytes == patch_embed_geometry(B, C, N, 256, D, false).ws_bytes, "sweep forward B %d C %d N %d D %d ncls %d (%s)", B, C, N, D, ncls, f.msg);
            CHECK(g.err == SFCVIT_OK && g.form == PeForm::TILED && g.nz >= 1 && g.nz <= G && g.KR % 64 == 0 && g.slab_bytes <= pe2_bwd_workspace(C, D) &&
                  pe2_bwd_workspace(C, D) <= g.ws_bytes && g.ws_bytes == patch_embed_geometry(B, C, N, 256, D, true).ws_bytes,
                  "sweep backward B %d C %d N %d D %d ncls %d: nz %d G %d (%s)", B, C, N, D, ncls, g.nz, G, g.msg);
            int64_t rows_covered = 0, nz = 0;
            for (int c = 0; c < ncls; c++) { const int64_t r = int64_t(cnt[c]) * B; nz += (r + g.KR - 1) / g.KR; rows_covered += r; }
            CHECK(nz == g.nz && rows_covered == int64_t(B) * N, "sweep backward: nz %lld, the plan's %d", (long long)nz, g.nz);
            x.desc = nullptr;                                        // the generic forms at the same shape: zs slabs within the query
            const PatchEmbedPlan gb = patch_embed_plan(&x, true);
            CHECK(gb.err == SFCVIT_OK && gb.zs >= 1 && gb.zs <= gb.splits && int64_t(gb.zs) * gb.m_per_split >= gb.M && gb.slab_bytes <= gb.ws_bytes, "sweep generic backward");
        }
    }
    {   // refusals, in check order
        const std::vector<int32_t> none;
        auto bad = [&](bool bwd, const char *frag, const char *what, auto edit) {
            sfcvit_patch_embed_args x = pe_args(1, 3, 8, 8, 8, none);
            edit(x);
            refused(patch_embed_plan(&x, bwd), frag, what);
        };
        refused(patch_embed_plan(nullptr, false), "patch_embed_fwd: null pointer", "pe null a");
        refused(patch_embed_plan(nullptr, true), "patch_embed_bwd: null pointer", "pe null a");
        bad(false, "patch_embed_fwd: null pointer", "pe null x", [](auto &x) { x.x = nullptr; });
        bad(true, "patch_embed_bwd: null pointer", "pe null pix", [](auto &x) { x.pix = nullptr; });
        bad(true, "patch_embed_bwd: null pointer", "pe null y", [](auto &x) { x.y = nullptr; });
        bad(false, "patch_embed_fwd: non-positive dimension", "pe B 0", [](auto &x) { x.B = 0; });
        bad(true, "patch_embed_bwd: non-positive dimension", "pe D -8", [](auto &x) { x.D = -8; });
        bad(false, "patch_embed_fwd: N*P=64 must equal H*W=72", "pe HW", [](auto &x) { x.HW = 72; });
        bad(false, "patch_embed_fwd: D=12 must be a multiple of 8", "pe D 12", [](auto &x) { x.D = 12; });
        bad(true, "patch_embed_bwd: B*N too large", "pe B N", [](auto &x) { x.B = 1 << 28; });
        bad(true, "patch_embed_bwd: B*N too large", "pe B max", [&](auto &x) { x.B = big; });
        bad(false, "patch_embed_fwd: alignment", "pe x", [&](auto &x) { x.x = odd; });
        bad(false, "patch_embed_fwd: alignment", "pe y", [&](auto &x) { x.y = odd; });
        bad(true, "patch_embed_bwd: weight / bias alignment (w 16 bytes, bias 8 bytes)", "pe w", [&](auto &x) { x.w = odd; });
        bad(false, "patch_embed_fwd: weight / bias alignment", "pe bias", [&](auto &x) { x.bias = odd4; });
        bad(false, "patch_embed_fwd: null weight", "pe null w", [](auto &x) { x.w = nullptr; });
        bad(true, "patch_embed_bwd: null dw", "pe null dw", [](auto &x) { x.dw = nullptr; });
        bad(false, "patch_embed_fwd: workspace of 3072 bytes needed", "pe null workspace", [](auto &x) { x.workspace = nullptr; });
        bad(false, "patch_embed_fwd: workspace of 3072 bytes needed", "pe short workspace", [](auto &x) { x.workspace_bytes = 3071; });
        bad(true, "patch_embed_bwd: workspace of 768 bytes needed", "pe workspace alignment", [&](auto &x) { x.workspace = odd; });
        sfcvit_patch_embed_args x = pe_args(1, 3, 8, 8, 8, none);
        x.bias = static_cast<char *>(ptr(8)) + 8; x.dbias = nullptr; x.w = nullptr;
        const PatchEmbedPlan p = patch_embed_plan(&x, true);
        CHECK(p.err == SFCVIT_OK && !p.dbias && p.K == 24 && p.Kp == 24 && p.M == 8 && p.splits == 1 && p.zs == 1 && p.m_per_split == 64 && p.grid == 1,
              "pe backward without w / dbias: %s", p.msg);
    }

    // ---- hierarchical tokenizer ----
    auto hier_args = [&](int L, int D, int C, const std::vector<int32_t> &P, int N, int B, bool fuse) {
        sfcvit_hier_args q{};
        q.x = a; q.h = b; q.y = fuse ? ptr(7) : nullptr; q.wf = fuse ? ptr(8) : nullptr; q.bf = fuse ? ptr(9) : nullptr;
        for (int l = 0; l < L && l < 4; l++) { q.pix[l] = ia; q.w[l] = ptr(10); q.b[l] = ptr(11); q.P[l] = P[l]; }
        q.B = B; q.C = C; q.N = N; q.L = L; q.D = D; q.HW = int(int64_t(N) * P[0]);
        return q;
    };
    {
        struct H { int L, D, C; std::vector<int32_t> P; int N, B; int kp_sum, lds_fuse, lds_levels; };
        const H hs[] = {{1, 256, 1, {8}, 5, 13, 32, 38912, 5120}, {2, 128, 3, {8, 8}, 8, 2, 64, 43008, 9216}, {4, 64, 3, {64, 64, 64, 64}, 16, 3, 768, 133120, 99328},
                        {3, 256, 3, {16, 16, 16}, 64, 2, 192, 124928, 25600}, {4, 192, 3, {32, 32, 32, 32}, 4, 5, 384, 149504, 50176},
                        {4, 192, 1, {96, 96, 96, 96}, 4, 5, 384, 149504, 50176}};
        for (const H &q : hs) {
            sfcvit_hier_args x = hier_args(q.L, q.D, q.C, q.P, q.N, q.B, true);
            const HierPlan f = hier_plan(&x);
            named(f, "hier_fwd_kernel<fp32, fuse>", "hier fuse");
            CHECK(f.fuse && f.kp_sum == q.kp_sum && f.E == q.L * q.D && f.h_stride == 2 * f.E + 16 && f.a_stride == 2 * q.kp_sum + 16 && f.lds == q.lds_fuse &&
                  f.M == q.B * q.N && f.grid == (q.B * q.N + 63) / 64, "hier L %d D %d: kp %d lds %d grid %d", q.L, q.D, f.kp_sum, f.lds, f.grid);
            x = hier_args(q.L, q.D, q.C, q.P, q.N, q.B, false);
            x.x_is_bf16 = 1;
            const HierPlan l = hier_plan(&x);
            named(l, "hier_fwd_kernel<bf16, levels>", "hier levels");
            CHECK(!l.fuse && l.lds == q.lds_levels && l.lds == HT_ROWS * l.a_stride && l.grid == f.grid, "hier L %d D %d levels: lds %d", q.L, q.D, l.lds);
        }
        int E = 0, kp = 0;
        auto sfcvit_hier_tokenizer_supported = [](int L, int D, int C, const int32_t *P) { int e = 0, k = 0; return hier_envelope(L, D, C, P, e, k); };   // the entry point's body
        const int32_t inside[4] = {96, 96, 96, 192}, outside[4] = {96, 96, 128, 192}, k104[4] = {104, 104, 104, 104}, k768[4] = {256, 256, 256, 256};
        CHECK(hier_envelope(4, 192, 1, inside, E, kp) && E == 768 && kp == 480 && 64 * (2 * E + 16) + 64 * (2 * kp + 16) == 161792, "hier: kp 480 is inside 160 KiB");
        CHECK(!hier_envelope(4, 192, 1, outside, E, kp) && !hier_envelope(4, 192, 1, k104, E, kp) && !hier_envelope(4, 192, 3, k768, E, kp), "hier: kp 512 is outside");
        const int32_t p16[5] = {16, 16, 16, 16, 16}, p4[2] = {4, 4}, pneg[2] = {16, -16}, pbig[4] = {big, big, big, big}, p8big[4] = {big - 7, 8, 8, 8};
        CHECK(!sfcvit_hier_tokenizer_supported(3, 64, 3, p16) && !sfcvit_hier_tokenizer_supported(2, 96, 3, p16) && !sfcvit_hier_tokenizer_supported(2, 128, 3, p4) &&
              !sfcvit_hier_tokenizer_supported(5, 256, 3, p16) && !sfcvit_hier_tokenizer_supported(0, 256, 3, p16) && !sfcvit_hier_tokenizer_supported(2, 128, 3, pneg) &&
              !sfcvit_hier_tokenizer_supported(2, 128, 0, p16) && !sfcvit_hier_tokenizer_supported(2, 128, 3, nullptr) && !sfcvit_hier_tokenizer_supported(2, 0, 3, p16),
              "hier envelope: refusals");
        CHECK(!sfcvit_hier_tokenizer_supported(4, big - 63, big, pbig) && !sfcvit_hier_tokenizer_supported(4, 1 << 30, 8, p8big) &&
              !sfcvit_hier_tokenizer_supported(4, 64, big, pbig) && !sfcvit_hier_tokenizer_supported(1, 256, 1, p8big), "hier envelope: extents");
        const std::vector<int32_t> P3 = {16, 16, 16};
        auto bad = [&](const char *frag, const char *what, auto edit) {
            sfcvit_hier_args x = hier_args(3, 256, 3, P3, 64, 2, true);
            edit(x);
            refused(hier_plan(&x), frag, what);
        };
        refused(hier_plan(nullptr), "hier_tokenizer_fwd: null pointer", "hier null a");
        bad("hier_tokenizer_fwd: null pointer", "hier null x", [](auto &x) { x.x = nullptr; });
        bad("hier_tokenizer_fwd: null pointer", "hier null h", [](auto &x) { x.h = nullptr; });
        bad("hier_tokenizer_fwd: null pointer", "hier wf without y", [](auto &x) { x.y = nullptr; });
        bad("hier_tokenizer_fwd: B=0 C=3 HW=1024 N=64", "hier B 0", [](auto &x) { x.B = 0; });
        bad("outside the fused kernel's envelope", "hier D 96", [](auto &x) { x.D = 96; });
        bad("hier_tokenizer_fwd: L=5 D=256 C=3 outside", "hier L 5", [](auto &x) { x.L = 5; });
        bad("hier_tokenizer_fwd: too many token rows", "hier rows", [](auto &x) { x.B = 1 << 25; });
        bad("hier_tokenizer_fwd: too many token rows", "hier B N max", [&](auto &x) { x.B = big; x.N = big; });
        bad("hier_tokenizer_fwd: level 1: null pointer", "hier null pix 1", [](auto &x) { x.pix[1] = nullptr; });
        bad("hier_tokenizer_fwd: level 2: null pointer", "hier null w 2", [](auto &x) { x.w[2] = nullptr; });
        bad("hier_tokenizer_fwd: level 1: N * P = 64 * 8 != H*W = 1024 (levels must share the token count)", "hier P 1", [](auto &x) { x.P[1] = 8; });
        bad("hier_tokenizer_fwd: level 0: weight / bias alignment", "hier w 0", [&](auto &x) { x.w[0] = odd; });
        bad("hier_tokenizer_fwd: level 2: weight / bias alignment", "hier b 2", [&](auto &x) { x.b[2] = odd4; });
        bad("hier_tokenizer_fwd: fusion weight / output alignment", "hier wf", [&](auto &x) { x.wf = odd; });
        bad("hier_tokenizer_fwd: fusion weight / output alignment", "hier h", [&](auto &x) { x.h = odd; });
        bad("hier_tokenizer_fwd: fusion weight / output alignment", "hier bf", [&](auto &x) { x.bf = odd4; });
        sfcvit_hier_args x = hier_args(1, 256, 8, {1}, big - 64, 1, false);            // the most rows it takes: 2^31 - 65
        CHECK(hier_plan(&x).err == SFCVIT_OK && hier_plan(&x).grid == 33554431, "hier: B * N = %d refused (%s)", x.N, hier_plan(&x).msg);
    }
    {   // resampling: host arrays of exactly L entries
        for (int bwd = 0; bwd < 2; bwd++) {
            const char *name = bwd ? "hier_resample_concat_bwd_kernel" : "hier_resample_concat_kernel", *pre = bwd ? "hier_resample_concat_bwd: " : "hier_resample_concat: ";
            std::unique_ptr<int32_t[]> n(new int32_t[3]{64, 16, 64});
            std::unique_ptr<const void *[]> lev(new const void *[3]{ptr(7), ptr(8), ptr(9)});
            const ResamplePlan p = resample_plan(bwd, lev.get(), n.get(), 3, 3, 64, 40, a);
            named(p, name, "resample");
            if (!bwd) CHECK(p.blocks[0] == (3 * 64 * 3 * 5 + 255) / 256 && p.blocks[1] == 0, "resample forward: %d workgroups", p.blocks[0]);
            else CHECK(p.blocks[0] == 4 && p.blocks[1] == 1 && p.blocks[2] == 4, "resample backward: %d %d %d workgroups", p.blocks[0], p.blocks[1], p.blocks[2]);
            const ResamplePlan v = resample_plan(bwd, lev.get(), n.get(), 1, 256, 64, 768, a);       // 256 x 64 rows of 96 vectors: 6144 workgroups
            CHECK(v.err == SFCVIT_OK && v.blocks[0] == 6144, "resample 256 x 64 x 768: %d", v.blocks[0]);
            n[0] = 1 << 20;
            const ResamplePlan c = resample_plan(bwd, lev.get(), n.get(), 3, 64, 1 << 20, 1024, a);
            CHECK(c.err == SFCVIT_OK && c.blocks[0] == 65536 && (!bwd || (c.blocks[1] == 512 && c.blocks[2] == 2048)), "resample cap: %d", c.blocks[0]);
            n[0] = big; n[1] = big; n[2] = big - 1;
            const ResamplePlan e = resample_plan(bwd, lev.get(), n.get(), 3, big, big, big - 7, a);
            CHECK(e.err == SFCVIT_OK && e.blocks[0] == 65536 && (!bwd || (e.blocks[1] == 65536 && e.blocks[2] == 65536)), "resample extents: %s", e.msg);
            n[0] = 64; n[1] = 16; n[2] = 64;
            auto msg = [&](const char *rest) { static char buf[160]; std::snprintf(buf, sizeof(buf), "%s%s", pre, rest); return buf; };
            refused(resample_plan(bwd, nullptr, n.get(), 3, 3, 64, 40, a), msg("null pointer"), "resample null levels");
            refused(resample_plan(bwd, lev.get(), nullptr, 3, 3, 64, 40, a), msg("null pointer"), "resample null counts");
            refused(resample_plan(bwd, lev.get(), n.get(), 3, 3, 64, 40, nullptr), msg("null pointer"), "resample null cat");
            refused(resample_plan(bwd, lev.get(), n.get(), 0, 3, 64, 40, a), msg("L=0 B=3 N0=64 D=40 (1 <= L <= 8, D % 8 == 0)"), "resample L 0");
            refused(resample_plan(bwd, lev.get(), n.get(), 9, 3, 64, 40, a), msg("L=9"), "resample L 9");
            refused(resample_plan(bwd, lev.get(), n.get(), 3, 0, 64, 40, a), msg("L=3 B=0"), "resample B 0");
            refused(resample_plan(bwd, lev.get(), n.get(), 3, 3, 64, 44, a), msg("L=3 B=3 N0=64 D=44"), "resample D 44");
            refused(resample_plan(bwd, lev.get(), n.get(), 3, 3, 48, 40, a), msg("the first level has 64 tokens, not N0 = 48"), "resample N0");
            refused(resample_plan(bwd, lev.get(), n.get(), 3, 3, 64, 40, odd), msg("alignment"), "resample cat");
            n[1] = 0;
            refused(resample_plan(bwd, lev.get(), n.get(), 3, 3, 64, 40, a), msg("level 1 (pointer / token count / alignment)"), "resample n 1");
            n[1] = 16; lev[2] = nullptr;
            refused(resample_plan(bwd, lev.get(), n.get(), 3, 3, 64, 40, a), msg("level 2 (pointer / token count / alignment)"), "resample null level 2");
            lev[2] = ptr(9); lev[0] = odd;
            refused(resample_plan(bwd, lev.get(), n.get(), 3, 3, 64, 40, a), msg("level 0 (pointer / token count / alignment)"), "resample level 0");
        }
    }

    // ---- MixUp / CutMix ----
    {
        auto far = [](int i) { return reinterpret_cast<void *>(uintptr_t(i + 1) << 44); };         // 16 TiB apart
        const MixPlan p = mix_images_plan(far(0), ia, rec, far(1), 256, 3, 224, 224);
        CHECK(p.err == SFCVIT_OK && p.vec == 4 && p.HW == 50176 && p.grid == 49 && p.grid_y == 768, "mix_images ViT-B: vec %d grid (%d, %d)", p.vec, p.grid, p.grid_y);
        const MixPlan q = mix_images_plan(far(0), ia, rec, far(1), 2048, 3, 27, 27);
        CHECK(q.err == SFCVIT_OK && q.vec == 1 && q.HW == 729 && q.grid == 3 && q.grid_y == 4096, "mix_images 27 px: vec %d grid (%d, %d)", q.vec, q.grid, q.grid_y);
        const MixPlan e = mix_images_plan(far(0), ia, rec, reinterpret_cast<void *>(uintptr_t(1) << 63), 1, 1, big, 1);
        CHECK(e.err == SFCVIT_OK && e.vec == 1 && e.grid == (1 << 23), "mix_images H max: %s grid %d", e.msg, e.grid);
        refused(mix_images_plan(nullptr, ia, rec, b, 1, 1, 4, 4), "mix_images: null pointer", "mix_images null x");
        refused(mix_images_plan(a, nullptr, rec, b, 1, 1, 4, 4), "mix_images: null pointer", "mix_images null perm");
        refused(mix_images_plan(a, ia, nullptr, b, 1, 1, 4, 4), "mix_images: null pointer", "mix_images null rec");
        refused(mix_images_plan(a, ia, rec, nullptr, 1, 1, 4, 4), "mix_images: null pointer", "mix_images null out");
        refused(mix_images_plan(a, ia, rec, b, 0, 1, 4, 4), "mix_images: B=0 C=1 H=4 W=4", "mix_images B 0");
        refused(mix_images_plan(a, ia, rec, b, 1, 1, 65536, 32768), "mix_images: B=1 C=1 H=65536 W=32768", "mix_images H W = 2^31");
        refused(mix_images_plan(a, ia, rec, b, 65536, 32768, 4, 4), "mix_images: B=65536 C=32768", "mix_images B C = 2^31");
        refused(mix_images_plan(a, ia, rec, b, big, big, big, big), "mix_images: B=2147483647", "mix_images extents");
        refused(mix_images_plan(a, ia, rec, a, 1, 1, 4, 4), "mix_images: out must not alias x", "mix_images out = x");
        refused(mix_images_plan(a, ia, rec, static_cast<char *>(a) + 32, 1, 1, 4, 4), "must not alias", "mix_images overlap");
        refused(mix_images_plan(a, ia, rec, b, big, 1, big, 1), "must not alias", "mix_images 2^64 bytes");
        CHECK(mix_images_plan(a, ia, rec, static_cast<char *>(a) + 64, 1, 1, 4, 4).err == SFCVIT_OK, "mix_images: adjacent buffers refused");
        refused(mix_images_plan(a, ia, rec, odd, 1, 1, 4, 4), "mix_images: x and out must be 16-byte aligned", "mix_images out");
        const float *f = static_cast<const float *>(ptr(7));
        const int64_t *ya = static_cast<const int64_t *>(ptr(8)), *yb = static_cast<const int64_t *>(ptr(9));
        CHECK(soft_ce_pair_plan(a, ya, yb, rec, f, 256, 1000, 1024).grid == 64 && soft_ce_pair_plan(a, ya, yb, rec, f, 5, 10, 10).grid == 2 &&
              soft_ce_pair_plan(a, ya, yb, rec, f, big, big, big).grid == (1 << 29), "soft_ce_pair grid");
        refused(soft_ce_pair_plan(nullptr, ya, yb, rec, f, 1, 10, 16), "soft_ce_pair: null pointer", "soft_ce_pair null logits");
        refused(soft_ce_pair_plan(a, nullptr, yb, rec, f, 1, 10, 16), "soft_ce_pair: null pointer", "soft_ce_pair null y_a");
        refused(soft_ce_pair_plan(a, ya, nullptr, rec, f, 1, 10, 16), "soft_ce_pair: null pointer", "soft_ce_pair null y_b");
        refused(soft_ce_pair_plan(a, ya, yb, nullptr, f, 1, 10, 16), "soft_ce_pair: null pointer", "soft_ce_pair null rec");
        refused(soft_ce_pair_plan(a, ya, yb, rec, nullptr, 1, 10, 16), "soft_ce_pair: null pointer", "soft_ce_pair null loss");
        refused(soft_ce_pair_plan(a, ya, yb, rec, f, 0, 10, 16), "soft_ce_pair: B=0 C=10 ld=16", "soft_ce_pair B 0");
        refused(soft_ce_pair_plan(a, ya, yb, rec, f, 1, 0, 16), "soft_ce_pair: B=1 C=0", "soft_ce_pair C 0");
        refused(soft_ce_pair_plan(a, ya, yb, rec, f, 1, 10, 8), "soft_ce_pair: B=1 C=10 ld=8", "soft_ce_pair ld");
    }
    char name[96];
    CHECK(sfcvit_last_tokenizer_kernel(name, sizeof(name)) == SFCVIT_OK && !std::strcmp(name, "none"), "tokenizer: last kernel '%s'", name);
    CHECK(sfcvit_last_tokenizer_kernel(nullptr, 4) == SFCVIT_EINVAL, "tokenizer: null name buffer accepted");
}

int main() {
    const int curves[] = {SFCVIT_CURVE_HILBERT, SFCVIT_CURVE_Z, SFCVIT_CURVE_MOORE, SFCVIT_CURVE_PEANO, SFCVIT_CURVE_RASTER,
                          SFCVIT_CURVE_SPIRAL, SFCVIT_CURVE_HILBERT_T};
    const int sizes[] = {1, 2, 3, 5, 7, 8, 9, 14, 16, 24, 27, 28, 32, 33, 81, 100, 224};
    for (int c : curves)
        for (int n : sizes) {
            const int n2 = n * n;
            std::unique_ptr<int32_t[]> flat(new int32_t[n2]);
            std::unique_ptr<int64_t[]> rc(new int64_t[2 * size_t(n2)]);
            const int r1 = sfcvit_curve_table(c, n, flat.get());
            if (c == SFCVIT_CURVE_HILBERT_T && (n & (n - 1))) {      // the _2D tokenizer's private generator: powers of two only
                CHECK(r1 != SFCVIT_OK || is_permutation(flat.get(), n2), "curve %d n %d: accepted but not a permutation", c, n);
                continue;
            }
            CHECK(r1 == SFCVIT_OK, "curve %d n %d: %s", c, n, sfcvit_last_error());
            if (r1 != SFCVIT_OK) continue;
            CHECK(is_permutation(flat.get(), n2), "curve %d n %d: not a permutation of the grid", c, n);
            CHECK(sfcvit_curve_table_rc(c, n, rc.get()) == SFCVIT_OK, "curve %d n %d (rc): %s", c, n, sfcvit_last_error());
            for (int t = 0; t < n2; t++)
                if (rc[2 * size_t(t)] * n + rc[2 * size_t(t) + 1] != flat[t]) { CHECK(false, "curve %d n %d: rc / flat disagree at %d", c, n, t); break; }
        }
    // argument errors come back as codes with a message, never as a crash
    CHECK(sfcvit_curve_table(99, 4, nullptr) == SFCVIT_EINVAL, "null output accepted");
    {
        int32_t one[16];
        CHECK(sfcvit_curve_table(99, 4, one) == SFCVIT_EINVAL && std::strlen(sfcvit_last_error()) > 0, "unknown curve accepted");
        CHECK(sfcvit_curve_table(SFCVIT_CURVE_HILBERT, 0, one) != SFCVIT_OK, "n = 0 accepted");
        CHECK(sfcvit_curve_table(SFCVIT_CURVE_HILBERT, -3, one) != SFCVIT_OK, "n < 0 accepted");
    }
    // pixel tables: (img, p, g) of the _1D tokenizers (p = 1, g = pixels per token), ViT/16 patches (p = 16, g = 1), the
    // hierarchical levels of the reference's main.py (32 px: p = 1 g = 16, p = 2 g = 4 ... ) and a grouped case
    struct PT { int img, p, g, curve; };
    const PT pts[] = {{32, 1, 256, SFCVIT_CURVE_HILBERT}, {32, 16, 1, SFCVIT_CURVE_Z}, {32, 2, 16, SFCVIT_CURVE_Z}, {32, 4, 4, SFCVIT_CURVE_MOORE},
                      {224, 1, 256, SFCVIT_CURVE_HILBERT}, {224, 16, 1, SFCVIT_CURVE_HILBERT}, {224, 1, 256, SFCVIT_CURVE_RASTER},
                      {27, 3, 9, SFCVIT_CURVE_PEANO}, {48, 1, 256, SFCVIT_CURVE_SPIRAL}};
    for (const PT &q : pts) {
        const int grid = q.img / q.p, cells = grid * grid, P = q.g * q.p * q.p, N = cells / q.g;
        std::unique_ptr<int32_t[]> flat(new int32_t[cells]);
        CHECK(sfcvit_curve_table(q.curve, grid, flat.get()) == SFCVIT_OK, "pixel table: curve table failed");
        std::unique_ptr<int32_t[]> pix(new int32_t[size_t(N) * P]);
        const int rc = sfcvit_pixel_table(flat.get(), q.img, q.p, q.g, pix.get());
        CHECK(rc == SFCVIT_OK, "pixel table img %d p %d g %d: %s", q.img, q.p, q.g, sfcvit_last_error());
        if (rc != SFCVIT_OK) continue;
        CHECK(is_permutation(pix.get(), q.img * q.img), "pixel table img %d p %d g %d: not a permutation of the pixels", q.img, q.p, q.g);
        if (P == 256 && q.img % 8 == 0) {                          // what the tokenizers hand to sfcvit_tile_descriptors
            const int cap_needed = 16 + 2 * N + 2 * 8 * 256;       // DESC_HDR + 2 N + 2 MAXCLS 256
            std::unique_ptr<int32_t[]> probe(new int32_t[cap_needed]);
            const int total = sfcvit_tile_descriptors(pix.get(), N, P, q.img, probe.get(), cap_needed);
            CHECK(total >= 0, "tile descriptors img %d: %s", q.img, sfcvit_last_error());
            if (total > 0) {
                std::unique_ptr<int32_t[]> exact(new int32_t[total]);   // exactly what it said it writes
                CHECK(sfcvit_tile_descriptors(pix.get(), N, P, q.img, exact.get(), total) == total, "tile descriptors: exact capacity refused");
                CHECK(sfcvit_tile_descriptors(pix.get(), N, P, q.img, exact.get(), total - 1) < 0, "tile descriptors: short capacity accepted");
                CHECK(exact[4] == N && exact[5] == 256 && exact[1] >= 1 && exact[1] <= 8, "tile descriptors: header");
            }
        }
    }
    {
        int32_t flat[4] = {0, 1, 2, 7}, out[4 * 4 * 4];
        CHECK(sfcvit_pixel_table(flat, 4, 2, 1, out) == SFCVIT_EINVAL, "pixel table: out-of-range index accepted");
        CHECK(sfcvit_pixel_table(flat, 5, 2, 1, out) == SFCVIT_EINVAL, "pixel table: img not a multiple of p accepted");
        CHECK(sfcvit_pixel_table(flat, 4, 2, 3, out) == SFCVIT_EINVAL, "pixel table: group that does not divide accepted");
        CHECK(sfcvit_pixel_table(nullptr, 4, 2, 1, out) == SFCVIT_EINVAL, "pixel table: null accepted");
        CHECK(sfcvit_tile_descriptors(nullptr, 4, 256, 32, out, 64) < 0, "tile descriptors: null accepted");
    }
    CHECK(sfcvit_abi_version() == SFCVIT_ABI_VERSION, "abi version");
    check_dispatch();
    check_mask_blocks();
    check_attention_bias();
    check_pos_embed();
    check_token_pool();
    check_dwconv();
    check_tokmix();
    check_rowwise();
    check_tokenizer();
    check_drop_path();
    check_layer_scale();
    check_qk_norm();
    check_rope();
    check_model_ema();
    check_grad_accum();
    if (g_fail) { std::fprintf(stderr, "host_check: %d check(s) failed\n", g_fail); return 1; }
    std::printf("host_check ok\n");
    return 0;
}
