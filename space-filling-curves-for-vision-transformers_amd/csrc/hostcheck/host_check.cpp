// Sanitizer driver for the HOST-ONLY code of libsfcvit_hip.so ("Race detection / sanitizers": GPU ASan is not
// available on this pool, so the native host code gets a CPU-side -fsanitize=address,undefined build of its own):
//   sfcvit_curve_table / _rc (curves.cpp), sfcvit_pixel_table (curves.cpp), sfcvit_tile_descriptors (patch_embed_tiled.hip,
//   host part), the error path of common.cpp, and the mask validation and block map of attention_masked.cpp (check_mask_blocks), the plan and refusals of pos_embed.cpp (check_pos_embed) and of token_pool.cpp (check_token_pool), and the kernel selection of dispatch.cpp (check_dispatch: which kernel, grid,
//   splits and post passes each GEMM / attention shape of the benchmarked models gets).  Every output buffer is a heap block of EXACTLY the documented size, so that
// an off-by-one in a generator or in the descriptor writer is a heap-buffer-overflow report instead of silent corruption.
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
#include "../dispatch.h"
#include "../pos_embed.h"
#include "../token_pool.h"

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
    check_pos_embed();
    check_token_pool();
    if (g_fail) { std::fprintf(stderr, "host_check: %d check(s) failed\n", g_fail); return 1; }
    std::printf("host_check ok\n");
    return 0;
}
