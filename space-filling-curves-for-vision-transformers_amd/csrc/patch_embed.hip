// Fused SFC gather + patchify + linear projection for gfx950 (see
// sfcvit_patch_embed_fwd / _bwd in include/sfcvit.h).
//
// The reference does this in three passes over the image (advanced-index gather,
// reshape copy, GEMM; hilbert_embedding1D.py:36-43) and keeps the gathered
// [B, N, P*C] tensor for backward.  Here the gather is the A-operand loader of the
// MFMA GEMM: token rows are assembled in registers from the image through the
// per-token pixel table and written straight into the LDS tile, so the token
// matrix never exists in HBM; backward re-gathers it the same way.
//
// The contraction index is reordered channel-major (f' = c*P + kk instead of the
// reference's kk*C + c) so that 8 consecutive features are 8 consecutive curve
// positions of one channel: one 32-byte read of the pixel table + 8 image reads
// per LDS vector.  W is permuted to that order once per call into the workspace
// (D*K bf16, L2-resident); dW is permuted back by the split-K reduction.
#include "common_host.h"
#include "gemm_core.h"
#include "mix.h"
#include "tokenizer.h"

namespace sfcvit {
namespace {

using namespace gemm_core;
static_assert(BM == PATCH_BM && BN == PATCH_BN && BK == PATCH_BK && THREADS == PATCH_THREADS && TILE_BYTES == PATCH_TILE_BYTES,
              "patch_embed_plan sizes the grids and the LDS of pe_fwd_kernel / pe_bwd_kernel from these");

struct Geo {
    const void *x;
    const int32_t *pix;
    int B, C, HW, N, P, M, K, Kp;   // M = B*N token rows, K = C*P features, Kp = K rounded up to 8 (zero padded)
};

// 8 consecutive channel-major features f..f+7 of token row m, as bf16x8 bits.
template <bool XBF16>
__device__ __forceinline__ u32x4 gather8(const Geo &g, int m, int f) {
    const int b = m / g.N, t = m - b * g.N;
    float v[8];
    if ((g.P & 7) == 0) {
        const int c = f / g.P, kk = f - c * g.P;
        const int32_t *pp = g.pix + size_t(t) * g.P + kk;
        const u32x4 i0 = *reinterpret_cast<const u32x4 *>(pp), i1 = *reinterpret_cast<const u32x4 *>(pp + 4);
        const uint32_t idx[8] = {i0[0], i0[1], i0[2], i0[3], i1[0], i1[1], i1[2], i1[3]};
        const size_t plane = (size_t(b) * g.C + c) * g.HW;
#pragma unroll
        for (int j = 0; j < 8; j++)
            v[j] = XBF16 ? bf2f(static_cast<const uint16_t *>(g.x)[plane + idx[j]])
                         : static_cast<const float *>(g.x)[plane + idx[j]];
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int ff = f + j;
            float val = 0.f;
            if (ff < g.K) {
                const int c = ff / g.P, kk = ff - c * g.P;
                const size_t off = (size_t(b) * g.C + c) * g.HW + g.pix[size_t(t) * g.P + kk];
                val = XBF16 ? bf2f(static_cast<const uint16_t *>(g.x)[off]) : static_cast<const float *>(g.x)[off];
            }
            v[j] = val;
        }
    }
    return u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
}

// Token tile for the forward GEMM: 128 token rows x 64 features ("kc" image).
template <bool XBF16>
__device__ __forceinline__ void load_tokens_kc(Stage &s, const Geo &g, int m0, int k0, int tid) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int v = tid + THREADS * i;
        const int m = m0 + (v >> 3), f = k0 + ((v & 7) << 3);
        s.v[i] = (m < g.M && f < g.Kp) ? gather8<XBF16>(g, m, f) : u32x4{0u, 0u, 0u, 0u};
    }
}

// Token tile for the weight-gradient GEMM: 64 token rows (contraction) x 128 features ("st" image).
template <bool XBF16>
__device__ __forceinline__ void load_tokens_st(Stage &s, const Geo &g, int f0, int m0, int mend, int tid) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int v = tid + THREADS * i;
        const int m = m0 + (v >> 4), f = f0 + ((v & 15) << 3);
        s.v[i] = (m < mend && f < g.Kp) ? gather8<XBF16>(g, m, f) : u32x4{0u, 0u, 0u, 0u};
    }
}

// W'[d][c*P + kk] = W[d][kk*C + c]; rows padded with zeros to Kp features
__global__ __launch_bounds__(256) void permute_w_kernel(const uint16_t *__restrict__ w, uint16_t *__restrict__ wp, int D,
                                                        int C, int P, int Kp) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const int K = C * P;
    if (i >= int64_t(D) * Kp) return;
    const int d = int(i / Kp), f = int(i % Kp);
    const int c = f / P, kk = f % P;
    wp[i] = f < K ? w[size_t(d) * K + kk * C + c] : uint16_t(0);
}

// y[m, d] = sum_f' tokens'[m, f'] W'[d, f'] + bias[d]
template <bool XBF16>
__global__ __launch_bounds__(THREADS, 2) void pe_fwd_kernel(const Geo g, const uint16_t *__restrict__ wp,
                                                            const uint16_t *__restrict__ bias, uint16_t *__restrict__ y,
                                                            int D) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_n = (D + BN - 1) / BN;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
    const int nk = (g.Kp + BK - 1) / BK;
    f32x4 acc[4][4];
    zero_acc(acc);
    Stage sa, sb;
    load_tokens_kc<XBF16>(sa, g, m0, 0, tid);
    load_tile<false>(sb, wp, g.Kp, n0, D, 0, g.Kp, tid);
    store_tile<false>(sa, smem, tid);
    store_tile<false>(sb, smem + TILE_BYTES, tid);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const char *ia = smem + (kt & 1) * 2 * TILE_BYTES;
        const bool more = kt + 1 < nk;
        if (more) {
            load_tokens_kc<XBF16>(sa, g, m0, (kt + 1) * BK, tid);
            load_tile<false>(sb, wp, g.Kp, n0, D, (kt + 1) * BK, g.Kp, tid);
        }
        mma_tile<false, false>(acc, ia, ia + TILE_BYTES, wm, wn, lane);
        if (more) {
            char *oa = smem + ((kt + 1) & 1) * 2 * TILE_BYTES;
            store_tile<false>(sa, oa, tid);
            store_tile<false>(sb, oa + TILE_BYTES, tid);
        }
        __syncthreads();
    }
    mfma_fence();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
        if (n >= D) continue;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (bias) {
            const u32x2 b2 = *reinterpret_cast<const u32x2 *>(bias + n);
            bv[0] = bf2f(uint16_t(b2[0])); bv[1] = bf2f(uint16_t(b2[0] >> 16));
            bv[2] = bf2f(uint16_t(b2[1])); bv[3] = bf2f(uint16_t(b2[1] >> 16));
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int m = m0 + wm * 64 + i * 16 + (lane & 15);
            if (m >= g.M) continue;
            u32x2 o = {pack2bf(acc[i][j][0] + bv[0], acc[i][j][1] + bv[1]), pack2bf(acc[i][j][2] + bv[2], acc[i][j][3] + bv[3])};
            *reinterpret_cast<u32x2 *>(y + size_t(m) * D + n) = o;
        }
    }
}

// slab[z][d, f'] = sum_{m in split z} dY[m, d] tokens'[m, f']
template <bool XBF16>
__global__ __launch_bounds__(THREADS, 2) void pe_bwd_kernel(const Geo g, const uint16_t *__restrict__ dy,
                                                            float *__restrict__ slabs, int D, int m_per_split) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // 1-D grid, XCD-aware: logical index = (split z, feature tile, d tile) with the d tile fastest, and consecutive
    // logical indices on one XCD -- the D / 128 workgroups that re-gather the same token tile then share it in that
    // XCD's L2 (with a plain 3-D grid they were dealt round-robin over the XCDs: 1.79 GB of HBM-side traffic per launch
    // for 0.23 GB of operands, rocprofv3 FETCH_SIZE).
    const int tiles_d = (D + BM - 1) / BM, tiles_f = (g.Kp + BN - 1) / BN;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int dz = lid % tiles_d, fz = (lid / tiles_d) % tiles_f, zz = lid / (tiles_d * tiles_f);
    const int d0 = dz * BM, f0 = fz * BN;
    const int mbeg = zz * m_per_split, mend = min(g.M, mbeg + m_per_split);
    const int nk = (mend - mbeg + BK - 1) / BK;
    f32x4 acc[4][4];
    zero_acc(acc);
    Stage sa, sb;
    load_tile<true>(sa, dy, D, d0, D, mbeg, mend, tid);
    load_tokens_st<XBF16>(sb, g, f0, mbeg, mend, tid);
    store_tile<true>(sa, smem, tid);
    store_tile<true>(sb, smem + TILE_BYTES, tid);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const char *ia = smem + (kt & 1) * 2 * TILE_BYTES;
        const bool more = kt + 1 < nk;
        if (more) {
            load_tile<true>(sa, dy, D, d0, D, mbeg + (kt + 1) * BK, mend, tid);
            load_tokens_st<XBF16>(sb, g, f0, mbeg + (kt + 1) * BK, mend, tid);
        }
        mma_tile<true, true>(acc, ia, ia + TILE_BYTES, wm, wn, lane);
        if (more) {
            char *oa = smem + ((kt + 1) & 1) * 2 * TILE_BYTES;
            store_tile<true>(sa, oa, tid);
            store_tile<true>(sb, oa + TILE_BYTES, tid);
        }
        __syncthreads();
    }
    mfma_fence();
    store_partial(acc, slabs + size_t(zz) * D * g.Kp, D, g.Kp, d0, f0, wm, wn, lane);
}

// dW[d][kk*C + c] = sum_z slab[z][d][c*P + kk].  A 1024-thread block owns 16 consecutive slab elements; its 64 thread
// rows each add every 64th slab (a narrow tokenizer level -- K = 48, D = 256 -- has 2 output tiles and therefore 512
// slabs: one thread per element summed them serially in 119 us), then 4 thread rows add 16 sub-sums each and one adds
// those 4.  Fixed order: bit-reproducible.
__global__ __launch_bounds__(1024) void pe_bwd_reduce(const float *__restrict__ slabs, int splits, float *__restrict__ dw,
                                                      int D, int C, int P, int Kp) {
    __shared__ float red[64][17];
    __shared__ float red2[4][16];
    const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int64_t i = int64_t(blockIdx.x) * 16 + cl, total = int64_t(D) * Kp;
    float s = 0.f;
    if (i < total)
        for (int z = grp; z < splits; z += 64) s += slabs[size_t(z) * total + i];
    red[grp][cl] = s;
    __syncthreads();
    if (grp < 4) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; k++) t += red[grp * 16 + k][cl];
        red2[grp][cl] = t;
    }
    __syncthreads();
    if (grp == 0 && i < total) {
        const int K = C * P, d = int(i / Kp), f = int(i % Kp);
        if (f < K) {
            const int c = f / P, kk = f % P;
            dw[size_t(d) * K + kk * C + c] = (red2[0][cl] + red2[1][cl]) + (red2[2][cl] + red2[3][cl]);
        }
    }
}

}  // namespace

// patch_embed_tiled.hip: raise the LDS limit and launch what the plan says
int launch_pe2_fwd(const PatchEmbedPlan &p, const sfcvit_patch_embed_args &a, hipStream_t s);
int launch_pe2_bwd(const PatchEmbedPlan &p, const sfcvit_patch_embed_args &a, hipStream_t s);
}  // namespace sfcvit

using namespace sfcvit;

// ---------------------------------------------------------------------------------------------------------------------
// The gather alone (sfcvit_tokens_gather): one workgroup per (token n, group of IMG images).  The token's P pixel offsets
// are read once; per image every thread loads its pixels' C channel values (4-byte / 2-byte loads that between them
// use every byte of the token's image lines), rounds to bf16 into an LDS row in the reference's feature order
// kk * C + c, and the row leaves as 16-byte stores.
// ---------------------------------------------------------------------------------------------------------------------
namespace sfcvit {
namespace {
constexpr int GT = GATHER_THREADS, GIMG = GATHER_IMG;

// MIX: image b is mixed with image perm[b] as the record says (mix.h) on the way to bf16; fp32 images only.
template <bool XBF16, bool MIX>
__global__ __launch_bounds__(GT) void tokens_gather_kernel(const void *__restrict__ x, const int32_t *__restrict__ pix,
                                                           uint16_t *__restrict__ tokens, int B, int C, int HW, int N, int P, int ld,
                                                           int W, const int32_t *__restrict__ perm, const uint32_t *__restrict__ rec) {
    static_assert(!(XBF16 && MIX), "a mix needs fp32 images");
    extern __shared__ __attribute__((aligned(16))) char smem_g[];
    uint16_t *row = reinterpret_cast<uint16_t *>(smem_g);                 // [ld]
    const int n = blockIdx.x, b0 = blockIdx.y * GIMG, tid = threadIdx.x, K = P * C;
    MixRec mr{};
    if constexpr (MIX) mr = load_mix_rec(rec);
    for (int i = K + tid; i < ld; i += GT) row[i] = 0;                     // padding columns
    for (int b = b0; b < min(B, b0 + GIMG); b++) {
        const size_t img = size_t(b) * C * HW;
        size_t imq = img;
        if constexpr (MIX) imq = size_t(mix_partner(perm, b, B)) * C * HW;
        for (int kk = tid; kk < P; kk += GT) {
            const int off = pix[size_t(n) * P + kk];
            const int pr = MIX ? off / W : 0, pc = MIX ? off - pr * W : 0;
            const bool partner = MIX && mix_needs_partner(mr, pr, pc), inside = MIX && in_box(mr, pr, pc);
            for (int c = 0; c < C; c++) {
                const size_t src = img + size_t(c) * HW + off;
                if constexpr (MIX) {
                    const float a = static_cast<const float *>(x)[src];
                    const float bq = partner ? static_cast<const float *>(x)[imq + size_t(c) * HW + off] : 0.f;
                    row[kk * C + c] = f2bf(mix_px(mr, a, bq, inside));
                } else {
                    row[kk * C + c] = XBF16 ? static_cast<const uint16_t *>(x)[src] : f2bf(static_cast<const float *>(x)[src]);
                }
            }
        }
        __syncthreads();
        uint16_t *dst = tokens + (size_t(b) * N + n) * ld;
        for (int v = tid; v < ld / 8; v += GT) *reinterpret_cast<u32x4 *>(dst + v * 8) = *reinterpret_cast<const u32x4 *>(row + v * 8);
        __syncthreads();
    }
}

// P <= 256 (every reference tokenizer: 16, 64 or 256 pixels per token), C <= 4: one pixel per thread, the loads of all GIMG
// images in flight at once, one barrier per workgroup -- and TWO tokens per workgroup, taken from `order`: a 16 x 16 tile's
// rows are 64 bytes of fp32, half a 128-byte line whose other half belongs to the tile next to it; with one token per
// workgroup every line of the image was fetched twice (62 us at ViT-B / 256 images: 154 MB of image read as 308).  The
// caller orders the tokens by their lowest pixel offset, which puts horizontal neighbours side by side.
template <bool XBF16, int CMAX, bool MIX>
__global__ __launch_bounds__(2 * GT) void tokens_gather_p256_kernel(const void *__restrict__ x, const int32_t *__restrict__ pix,
                                                                    const int32_t *__restrict__ order, uint16_t *__restrict__ tokens,
                                                                    int B, int C, int HW, int N, int P, int ld,
                                                                    int W, const int32_t *__restrict__ perm, const uint32_t *__restrict__ rec) {
    static_assert(!(XBF16 && MIX), "a mix needs fp32 images");
    extern __shared__ __attribute__((aligned(16))) char smem_g[];
    const int half = threadIdx.x >> 8, tid = threadIdx.x & (GT - 1);
    const int slot = 2 * blockIdx.x + half;
    uint16_t *rows = reinterpret_cast<uint16_t *>(smem_g) + size_t(half) * GIMG * ld;   // [2][GIMG][ld]
    const int b0 = blockIdx.y * GIMG, K = P * C;
    const int nb = min(GIMG, B - b0);
    const bool live = slot < N;
    const int n = live ? (order ? order[slot] : slot) : 0;
    uint16_t v[GIMG][CMAX];
    if (live && tid < P) {
        const int off = pix[size_t(n) * P + tid];
        if constexpr (MIX) {
            // the partner's pixel rides along with the image's own: all loads of the GIMG images in flight, then combined
            const MixRec mr = load_mix_rec(rec);
            const int pr = off / W, pc = off - pr * W;
            const bool partner = mix_needs_partner(mr, pr, pc), inside = in_box(mr, pr, pc);   // per pixel: a CutMix box cuts through tokens
            float a[GIMG][CMAX], bq[GIMG][CMAX];
#pragma unroll
            for (int i = 0; i < GIMG; i++) {
                if (i < nb) {
                    const size_t img = size_t(b0 + i) * C * HW + off;
                    const size_t imq = size_t(mix_partner(perm, b0 + i, B)) * C * HW + off;
#pragma unroll
                    for (int c = 0; c < CMAX; c++)
                        if (c < C) {
                            a[i][c] = static_cast<const float *>(x)[img + size_t(c) * HW];
                            bq[i][c] = partner ? static_cast<const float *>(x)[imq + size_t(c) * HW] : 0.f;
                        }
                }
            }
#pragma unroll
            for (int i = 0; i < GIMG; i++)
                if (i < nb)
#pragma unroll
                    for (int c = 0; c < CMAX; c++)
                        if (c < C) v[i][c] = f2bf(mix_px(mr, a[i][c], bq[i][c], inside));
        } else {
#pragma unroll
            for (int i = 0; i < GIMG; i++) {
                if (i < nb) {
                    const size_t img = size_t(b0 + i) * C * HW + off;
#pragma unroll
                    for (int c = 0; c < CMAX; c++)
                        if (c < C) v[i][c] = XBF16 ? static_cast<const uint16_t *>(x)[img + size_t(c) * HW] : f2bf(static_cast<const float *>(x)[img + size_t(c) * HW]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < GIMG; i++)
            if (i < nb)
#pragma unroll
                for (int c = 0; c < CMAX; c++)
                    if (c < C) rows[i * ld + tid * C + c] = v[i][c];
    }
    if (live)
        for (int i = K + tid; i < ld; i += GT)
            for (int r = 0; r < nb; r++) rows[r * ld + i] = 0;
    __syncthreads();
    if (!live) return;
    const int vpr = ld / 8;
    for (int j = tid; j < nb * vpr; j += GT) {
        const int r = j / vpr, vv = j - r * vpr;
        *reinterpret_cast<u32x4 *>(tokens + (size_t(b0 + r) * N + n) * ld + vv * 8) = *reinterpret_cast<const u32x4 *>(rows + r * ld + vv * 8);
    }
}


// Tokens that are 16 x 16 pixel tiles of an fp32 image (every Hilbert / Z tokenizer at 256 pixels per token): the image is
// read in WHOLE 128-byte lines -- a line is one tile row of two horizontally adjacent tiles -- with 16-byte loads, eight
// lines per wave instruction, and the curve order is applied on the way OUT of LDS.  One wave owns a unit = (tile pair,
// image): 2 C wave loads, the bf16 pair image [C][16 rows][32 pixels] in a wave-private LDS region, then every lane
// collects the 8 features of each of its C output vectors with 2-byte LDS reads at addresses worked out once per
// workgroup (feature j of token t: channel j % C of curve pixel j / C), and the two token rows leave as contiguous
// 16-byte stores.  Against the per-pixel kernel above: a quarter of the load instructions, half the lines touched per
// byte (a 4-byte-per-lane load of 64 curve-consecutive pixels touches 8 lines for 256 bytes), no workgroup barrier
// between a unit's loads and its stores.  Workgroup = 4 waves x U images (U = 1: 78 registers, six workgroups per CU, 6 272
// short workgroups at ViT-B / 256 images -- the tail of the launch is what U = 2 lost: 45.7 vs 44.0 us in the step); the
// image is read and the tokens are written with nontemporal accesses (see the launch code).  A third form -- one workgroup
// per 16-row strip of the image, read front to back -- was built and dropped: 56 us warm against 38 (two barriers per image,
// 132 registers).
constexpr int TG_THREADS = GATHER_THREADS;

// MIX: the wave loads the same lines of image perm[b] next to those of b and combines them in registers before pack2bf
// (mix.h): MixUp everywhere, CutMix per pixel -- row and column follow from `line`, `chunk` and the tile origin -- and a
// tile pair that the box does not touch (or mode 0) issues no partner loads at all: the test is wave-uniform.
template <int C, int NT, int U, bool MIX>
__global__ __launch_bounds__(TG_THREADS) void tokens_gather_tiles_kernel(const float *__restrict__ x, const int32_t *__restrict__ pix,
                                                                         const int32_t *__restrict__ order, const int32_t *__restrict__ origin,
                                                                         uint16_t *__restrict__ tokens, int B, int HW, int W,
                                                                         uint32_t wmagic, int N,
                                                                         const int32_t *__restrict__ perm, const uint32_t *__restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) char smem_g[];
    uint16_t *pos = reinterpret_cast<uint16_t *>(smem_g);                  // [2 tokens][256 curve pixels] -> pixel of the pair image
    constexpr int UNIT = C * 16 * 64;                                      // bytes of one bf16 pair image
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int slot = 2 * blockIdx.x;
    const bool two = slot + 1 < N;
    const int n0 = order ? order[slot] : slot;
    const int n1 = two ? (order ? order[slot + 1] : slot + 1) : n0;
    const int o0 = origin[n0], o1 = origin[n1];
    for (int i = tid; i < 512; i += TG_THREADS) {
        const int t = i >> 8, kk = i & 255;
        const uint32_t d = uint32_t(pix[size_t(t ? n1 : n0) * 256 + kk] - (t ? o1 : o0));     // < 16 W
        const uint32_t r = __umulhi(d, wmagic);                           // d / W: exact for d W < 2^32
        pos[i] = uint16_t(r * 32 + 16 * t + (d - r * W));
    }
    // this wave's two images: every line of the pair's rows, all loads in flight
    const int b0 = blockIdx.y * (4 * U) + U * wave;
    const int chunk = lane & 7, lt = chunk >> 2;
    const size_t src0 = size_t(lt ? o1 : o0) + 4 * (chunk & 3);
    f32x4 v[U][2 * C];
    // MIX: pixel (row, col) of this lane's vector i is (trow + (line & 15), tcol + e), e = 0..3; `partner` is the same
    // for every lane of the workgroup (record and tile origins are)
    MixRec mr{};
    int trow = 0, tcol = 0;
    bool partner = false;
    if constexpr (MIX) {
        mr = load_mix_rec(rec);
        const int oo = lt ? o1 : o0;
        trow = oo / W;
        tcol = oo - trow * W + 4 * (chunk & 3);
        const int ra = o0 / W, ca = o0 - ra * W, rb = o1 / W, cb = o1 - rb * W;
        partner = mr.mode == 1u ||
                  (mr.mode == 2u && ((ra < mr.r1 && ra + 16 > mr.r0 && ca < mr.c1 && ca + 16 > mr.c0) ||
                                     (rb < mr.r1 && rb + 16 > mr.r0 && cb < mr.c1 && cb + 16 > mr.c0)));
    }
    f32x4 vq[MIX ? U : 1][MIX ? 2 * C : 1];
#pragma unroll
    for (int u = 0; u < U; u++) {
        if (b0 + u < B) {
            const float *im = x + size_t(b0 + u) * C * HW + src0;
#pragma unroll
            for (int i = 0; i < 2 * C; i++) {
                const int line = 8 * i + (lane >> 3);
                const f32x4 *src = reinterpret_cast<const f32x4 *>(im + size_t(line >> 4) * HW + size_t(line & 15) * W);
                v[u][i] = (NT & 1) ? __builtin_nontemporal_load(src) : *src;
            }
            if constexpr (MIX) {
                if (partner) {
                    const float *iq = x + size_t(mix_partner(perm, b0 + u, B)) * C * HW + src0;
#pragma unroll
                    for (int i = 0; i < 2 * C; i++) {
                        const int line = 8 * i + (lane >> 3);
                        const f32x4 *src = reinterpret_cast<const f32x4 *>(iq + size_t(line >> 4) * HW + size_t(line & 15) * W);
                        vq[u][i] = (NT & 1) ? __builtin_nontemporal_load(src) : *src;
                    }
                }
            }
        }
    }
    if constexpr (MIX) {
        if (partner) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (b0 + u < B) {
#pragma unroll
                    for (int i = 0; i < 2 * C; i++) {
                        const int row = trow + ((8 * i + (lane >> 3)) & 15);
#pragma unroll
                        for (int e = 0; e < 4; e++) v[u][i][e] = mix_px(mr, v[u][i][e], vq[u][i][e], in_box(mr, row, tcol + e));
                    }
                }
            }
        }
    }
    __syncthreads();
    // byte addresses of the features of this lane's output vectors (vector vv of the pair = lane + 64 i: token vv / (32 C),
    // features 8 (vv % (32 C)) ... + 8)
    uint32_t addr[C][8];
#pragma unroll
    for (int i = 0; i < C; i++) {
        const int vv = lane + 64 * i, t = vv / (32 * C), j0 = (vv - t * 32 * C) * 8;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int j = j0 + e, kk = j / C, c = j - kk * C;
            addr[i][e] = uint32_t(c) * 1024 + 2 * uint32_t(pos[t * 256 + kk]);
        }
    }
    char *mine = smem_g + 1024 + size_t(U * wave) * UNIT;
#pragma unroll
    for (int u = 0; u < U; u++) {
        if (b0 + u >= B) break;                                            // wave-uniform
        char *im = mine + u * UNIT;
#pragma unroll
        for (int i = 0; i < 2 * C; i++) {
            const int line = 8 * i + (lane >> 3);
            u32x2 pk;
            pk[0] = pack2bf(v[u][i][0], v[u][i][1]);
            pk[1] = pack2bf(v[u][i][2], v[u][i][3]);
            *reinterpret_cast<u32x2 *>(im + line * 64 + chunk * 8) = pk;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int i = 0; i < C; i++) {
            const int vv = lane + 64 * i, t = vv / (32 * C), j0 = (vv - t * 32 * C) * 8;
            u32x4 o;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t lo = *reinterpret_cast<const uint16_t *>(im + addr[i][2 * q]);
                const uint32_t hi = *reinterpret_cast<const uint16_t *>(im + addr[i][2 * q + 1]);
                o[q] = lo | (hi << 16);
            }
            if (t == 0 || two) {
                u32x4 *dst = reinterpret_cast<u32x4 *>(tokens + (size_t(b0 + u) * N + (t ? n1 : n0)) * (256 * C) + j0);
                if (NT & 2) __builtin_nontemporal_store(o, dst);
                else *dst = o;
            }
        }
    }
}

}  // namespace
}  // namespace sfcvit

namespace sfcvit {
namespace {

// perm / rec: the batch mix (both or neither, as p.mix says).
int launch_gather_tiles(const GatherPlan &p, const char *what, const void *x, const int32_t *pix, const int32_t *order,
                        const int32_t *origin, const int32_t *perm, const uint32_t *rec, int B, int W, int N, void *tokens, void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto *xp = static_cast<const float *>(x);
    auto *tp = static_cast<uint16_t *>(tokens);
    const dim3 grid(p.grid_x, p.grid_y);
    note_tokenizer_kernel(p);
#define TILES_K(CC, NTV, UU, MX) hipLaunchKernelGGL((tokens_gather_tiles_kernel<CC, NTV, UU, MX>), grid, dim3(p.threads), p.lds, s, xp, pix, order, origin, tp, B, p.HW, W, p.wmagic, N, perm, rec)
#define TILES(CC, NTV) do { if (p.mix) TILES_K(CC, NTV, 1, true); else if (p.upw == 2) TILES_K(CC, NTV, 2, false); else TILES_K(CC, NTV, 1, false); } while (0)
#define TILES_C(CC) do { if (p.nt == 1) TILES(CC, 1); else if (p.nt == 2) TILES(CC, 2); else if (p.nt == 3) TILES(CC, 3); else TILES(CC, 0); } while (0)
    switch (p.C) {
    case 1: TILES_C(1); break;
    case 2: TILES_C(2); break;
    case 3: TILES_C(3); break;
    default: TILES_C(4); break;
    }
#undef TILES_C
#undef TILES
#undef TILES_K
    return check_launch(what);
}

// W is only read by the mixing kernels (pixel offset -> row, column).
int launch_gather(const GatherPlan &p, const char *what, const void *x, const int32_t *pix, const int32_t *order, const int32_t *perm,
                  const uint32_t *rec, int B, int W, int N, int P, void *tokens, int ld, void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto *tp = static_cast<uint16_t *>(tokens);
    const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
    note_tokenizer_kernel(p);
    if (p.form == GatherForm::P256) {
        if (p.mix)
            hipLaunchKernelGGL((tokens_gather_p256_kernel<false, 4, true>), grid, block, p.lds, s, x, pix, order, tp, B, p.C, p.HW, N, P, ld, W, perm, rec);
        else if (p.x_bf16)
            hipLaunchKernelGGL((tokens_gather_p256_kernel<true, 4, false>), grid, block, p.lds, s, x, pix, order, tp, B, p.C, p.HW, N, P, ld, W, perm, rec);
        else
            hipLaunchKernelGGL((tokens_gather_p256_kernel<false, 4, false>), grid, block, p.lds, s, x, pix, order, tp, B, p.C, p.HW, N, P, ld, W, perm, rec);
    } else if (p.mix) {
        hipLaunchKernelGGL((tokens_gather_kernel<false, true>), grid, block, p.lds, s, x, pix, tp, B, p.C, p.HW, N, P, ld, W, perm, rec);
    } else if (p.x_bf16) {
        hipLaunchKernelGGL((tokens_gather_kernel<true, false>), grid, block, p.lds, s, x, pix, tp, B, p.C, p.HW, N, P, ld, W, perm, rec);
    } else {
        hipLaunchKernelGGL((tokens_gather_kernel<false, false>), grid, block, p.lds, s, x, pix, tp, B, p.C, p.HW, N, P, ld, W, perm, rec);
    }
    return check_launch(what);
}

}  // namespace
}  // namespace sfcvit

extern "C" int sfcvit_tokens_gather_tiles(const void *x, const int32_t *pix, const int32_t *order, const int32_t *origin, int B, int C,
                                          int H, int W, int N, void *tokens, int ld, void *stream) {
    const GatherPlan p = gather_tiles_plan("tokens_gather_tiles", x, pix, origin, nullptr, B, C, H, W, N, tokens, ld, read_tokenizer_knobs());
    if (p.err) return fail(p.err, "%s", p.msg);
    return launch_gather_tiles(p, "tokens_gather_tiles", x, pix, order, origin, nullptr, nullptr, B, W, N, tokens, stream);
}

extern "C" int sfcvit_tokens_gather(const void *x, int x_is_bf16, const int32_t *pix, const int32_t *order, int B, int C, int HW, int N,
                                    int P, void *tokens, int ld, void *stream) {
    const GatherPlan p = gather_plan("tokens_gather", x, x_is_bf16, pix, nullptr, B, C, HW, N, P, tokens, ld);
    if (p.err) return fail(p.err, "%s", p.msg);
    return launch_gather(p, "tokens_gather", x, pix, order, nullptr, nullptr, B, 0, N, P, tokens, ld, stream);
}

extern "C" int sfcvit_tokens_gather_mix(const void *x, const int32_t *pix, const int32_t *order, const int32_t *origin,
                                        const int32_t *perm, const uint32_t *rec, int B, int C, int H, int W, int N, int P,
                                        void *tokens, int ld, void *stream) {
    const GatherPlan p = gather_mix_plan(x, pix, origin, perm, rec, B, C, H, W, N, P, tokens, ld, read_tokenizer_knobs());
    if (p.err) return fail(p.err, "%s", p.msg);
    if (p.form == GatherForm::TILES) return launch_gather_tiles(p, "tokens_gather_mix", x, pix, order, origin, perm, rec, B, W, N, tokens, stream);
    return launch_gather(p, "tokens_gather_mix", x, pix, order, perm, rec, B, W, N, P, tokens, ld, stream);
}

extern "C" int64_t sfcvit_patch_embed_workspace(int B, int C, int N, int P, int D, int bwd) {
    return patch_embed_geometry(B, C, N, P, D, bwd != 0).ws_bytes;
}

extern "C" int sfcvit_patch_embed_fwd(const sfcvit_patch_embed_args *a, void *stream) {
    const PatchEmbedPlan p = patch_embed_plan(a, false);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.form == PeForm::TILED) return launch_pe2_fwd(p, *a, s);      // tiles / strips: the coalesced kernel
    const Geo g{a->x, a->pix, a->B, a->C, a->HW, a->N, a->P, p.M, p.K, p.Kp};
    uint16_t *wp = static_cast<uint16_t *>(a->workspace);
    hipLaunchKernelGGL(permute_w_kernel, dim3(p.permute_grid), dim3(256), 0, s, static_cast<const uint16_t *>(a->w), wp, a->D, a->C, a->P, g.Kp);
    if (int rc = check_launch("patch_embed_fwd permute")) return rc;
    note_tokenizer_kernel(p);
    if (p.x_bf16)
        hipLaunchKernelGGL(pe_fwd_kernel<true>, dim3(p.grid), dim3(THREADS), p.lds, s, g, wp, static_cast<const uint16_t *>(a->bias),
                           static_cast<uint16_t *>(a->y), a->D);
    else
        hipLaunchKernelGGL(pe_fwd_kernel<false>, dim3(p.grid), dim3(THREADS), p.lds, s, g, wp, static_cast<const uint16_t *>(a->bias),
                           static_cast<uint16_t *>(a->y), a->D);
    return check_launch("patch_embed_fwd");
}

extern "C" int sfcvit_patch_embed_bwd(const sfcvit_patch_embed_args *a, void *stream) {
    const PatchEmbedPlan p = patch_embed_plan(a, true);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.form == PeForm::TILED) {                                     // tiles / strips: the coalesced kernel
        if (int rc = launch_pe2_bwd(p, *a, s)) return rc;
    } else {
        const Geo g{a->x, a->pix, a->B, a->C, a->HW, a->N, a->P, p.M, p.K, p.Kp};
        float *slabs = static_cast<float *>(a->workspace);
        note_tokenizer_kernel(p);
        if (p.x_bf16)
            hipLaunchKernelGGL(pe_bwd_kernel<true>, dim3(p.grid), dim3(THREADS), p.lds, s, g, static_cast<const uint16_t *>(a->y), slabs, a->D, p.m_per_split);
        else
            hipLaunchKernelGGL(pe_bwd_kernel<false>, dim3(p.grid), dim3(THREADS), p.lds, s, g, static_cast<const uint16_t *>(a->y), slabs, a->D, p.m_per_split);
        if (int rc = check_launch("patch_embed_bwd")) return rc;
        hipLaunchKernelGGL(pe_bwd_reduce, dim3(p.reduce_grid), dim3(1024), 0, s, slabs, p.zs, static_cast<float *>(a->dw), a->D, a->C, a->P, g.Kp);
        if (int rc = check_launch("patch_embed_bwd reduce")) return rc;
    }
    if (p.dbias) return sfcvit_colsum(a->y, p.M, a->D, a->D, a->dbias, 0, a->workspace, a->workspace_bytes, stream);
    return SFCVIT_OK;
}
