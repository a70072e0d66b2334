// GEMMs along the token axis of [B, N, D] (see "Token mixing" in include/sfcvit.h): the token-mix branch of MixerBlock
// (src/models/vit.py:269-271) without its transposes.
//
//   tokmix_left_kernel    C_b[M, D] = epi( op(W) X_b[K, D] ): one 128 x 128 tile of ONE image per workgroup.  X_b is the
//                         k-major B operand of gemm_core ("st" LDS image, ds_read_b64_tr_b16 fragments); W is the A operand,
//                         k-contiguous ("kc" image) as stored or k-major when transposed.  The weight's row pitch is the token
//                         count for W1 (2 N bytes: 8-byte aligned at N = 196, 2-byte aligned at odd N), so its loader takes
//                         the widest load pitch and pointer allow (16 / 8 / 4 / 2 bytes, chosen on the host); W is a few MB
//                         and stays in L2.  The row bias is added to the accumulators, the rest of the epilogue is
//                         gemm_core's (aux_out, erf-GELU, residual, gelu'(aux_in), bf16 store through LDS).
//   tokmix_wgrad_kernel   dW[M, K] = sum_b G_b[M, D] X_b[K, D]^T: both operands k-contiguous (k = d).  The contraction over
//                         (b, d) is cut into ranges of whole images; a workgroup owns one dW tile of one range and writes its
//                         fp32 tile (and, in the first tile column, the row sums of G for db) into the range's row of the
//                         workspace.  reduce_cols adds the rows in a fixed order: no atomics, two runs give the same bits.
#include "common_host.h"
#include "gemm_core.h"
#include "token_mix.h"

namespace sfcvit {
namespace {

using namespace gemm_core;

// 8 consecutive bf16 of one weight row starting at column `col` (a multiple of 8), in loads of U elements; columns
// >= ncols read as zero.  ncols % U == 0 and (p + row_off) is 2 U-byte aligned (host: TokmixPlan::wunit).
template <int U>
__device__ __forceinline__ u32x4 load8(const uint16_t *__restrict__ p, size_t row_off, int col, int ncols) {
    u32x4 w = {0u, 0u, 0u, 0u};
    const uint16_t *q = p + row_off + col;
    if constexpr (U == 8) {
        if (col < ncols) w = *reinterpret_cast<const u32x4 *>(q);
    } else if constexpr (U == 4) {
#pragma unroll
        for (int h = 0; h < 2; h++)
            if (col + 4 * h < ncols) {
                const u32x2 t = *reinterpret_cast<const u32x2 *>(q + 4 * h);
                w[2 * h] = t[0];
                w[2 * h + 1] = t[1];
            }
    } else if constexpr (U == 2) {
#pragma unroll
        for (int h = 0; h < 4; h++)
            if (col + 2 * h < ncols) w[h] = *reinterpret_cast<const uint32_t *>(q + 2 * h);
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++)
            if (col + e < ncols) w[e >> 1] |= uint32_t(q[e]) << (16 * (e & 1));
    }
    return w;
}

// load_tile of gemm_core for the dense weight: KMAJOR = false: W is [M][K]; true: W is [K][M].  Out-of-range elements are zero.
template <bool KMAJOR, int U>
__device__ __forceinline__ void load_w_tile(Stage &s, const uint16_t *__restrict__ w, int m0, int M, int k0, int K, int tid) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int v = tid + THREADS * i;
        u32x4 val = {0u, 0u, 0u, 0u};
        if (!KMAJOR) {
            const int r = m0 + (v >> 3), k = k0 + ((v & 7) << 3);
            if (r < M) val = load8<U>(w, size_t(r) * K, k, K);
        } else {
            const int k = k0 + (v >> 4), r = m0 + ((v & 15) << 3);
            if (k < K) val = load8<U>(w, size_t(k) * M, r, M);
        }
        s.v[i] = val;
    }
}

template <bool KMAJOR>
__device__ __forceinline__ void load_w(Stage &s, const uint16_t *__restrict__ w, int unit, int m0, int M, int k0, int K, int tid) {
    switch (unit) {          // wave-uniform
    case 8: load_w_tile<KMAJOR, 8>(s, w, m0, M, k0, K, tid); break;
    case 4: load_w_tile<KMAJOR, 4>(s, w, m0, M, k0, K, tid); break;
    case 2: load_w_tile<KMAJOR, 2>(s, w, m0, M, k0, K, tid); break;
    default: load_w_tile<KMAJOR, 1>(s, w, m0, M, k0, K, tid); break;
    }
}

template <bool W_KM, bool HEAVY>
__global__ __launch_bounds__(THREADS, 2) void tokmix_left_kernel(const sfcvit_tokmix_args a, int wunit, int tiles_n, int tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][W tile | X tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
    const int M = a.M, K = a.K, D = a.D;
    const uint16_t *W = static_cast<const uint16_t *>(a.w);
    const uint16_t *X = static_cast<const uint16_t *>(a.x) + size_t(img) * K * D;
    const size_t out_off = size_t(img) * M * D;
    const int nk = (K + BK - 1) / BK;

    f32x4 acc[4][4];
    zero_acc(acc);

    Stage sa, sb;
    load_w<W_KM>(sa, W, wunit, m0, M, 0, K, tid);
    load_tile<true>(sb, X, D, n0, D, 0, K, tid);
    store_tile<W_KM>(sa, smem, tid);
    store_tile<true>(sb, smem + TILE_BYTES, tid);
    __syncthreads();

    for (int kt = 0; kt < nk; kt++) {
        const char *ia = smem + (kt & 1) * 2 * TILE_BYTES;
        const bool more = kt + 1 < nk;
        if (more) {
            load_w<W_KM>(sa, W, wunit, m0, M, (kt + 1) * BK, K, tid);
            load_tile<true>(sb, X, D, n0, D, (kt + 1) * BK, K, tid);
        }
        mma_tile<W_KM, true>(acc, ia, ia + TILE_BYTES, wm, wn, lane);
        if (more) {
            char *oa = smem + ((kt + 1) & 1) * 2 * TILE_BYTES;
            store_tile<W_KM>(sa, oa, tid);
            store_tile<true>(sb, oa + TILE_BYTES, tid);
        }
        __syncthreads();
    }
    mfma_fence();

    if (a.bias) {                                   // the ROW bias: a lane's accumulator fragment i holds one m
        const uint16_t *bp = static_cast<const uint16_t *>(a.bias);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int m = m0 + wm * 64 + i * 16 + (lane & 15);
            const float bv = m < M ? bf2f(bp[m]) : 0.f;
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] += f32x4{bv, bv, bv, bv};
        }
    }

    // gemm_core's epilogue on this image's [M, D] matrices (operand tiles are dead after the loop's final barrier)
    sfcvit_gemm_args g = {};
    g.c = static_cast<uint16_t *>(a.c) + out_off;
    g.residual = a.residual ? static_cast<const uint16_t *>(a.residual) + out_off : nullptr;
    g.aux_in = a.aux_in ? static_cast<const uint16_t *>(a.aux_in) + out_off : nullptr;
    g.aux_out = a.aux_out ? static_cast<uint16_t *>(a.aux_out) + out_off : nullptr;
    g.M = M;
    g.N = D;
    g.ldc = g.ldr = g.ldaux = D;
    g.act = a.act;
    g.dact = a.aux_in ? SFCVIT_ACT_GELU : SFCVIT_ACT_NONE;
    epilogue_tile<4, 4, HEAVY>(g, acc, reinterpret_cast<float *>(smem) + wave * (32 * 68), m0 + wm * 64, n0 + wn * 64, lane);
}

// part: [ranges][ld] fp32, ld = M * K + M.  want_dw / want_db: which half of a row is produced.
__global__ __launch_bounds__(THREADS, 2) void tokmix_wgrad_kernel(const uint16_t *__restrict__ G, const uint16_t *__restrict__ X,
                                                                  float *__restrict__ part, int B, int M, int K, int D, int tiles_n,
                                                                  int tiles, int per_range, int ld, int want_dw, int want_db) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][G tile | X tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int range = blockIdx.x / tiles, tile = blockIdx.x - range * tiles;
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
    const int img0 = range * per_range, nimg = min(B, img0 + per_range) - img0;
    const int dt = (D + BK - 1) / BK;               // k-tiles per image
    const int nk = nimg * dt;
    const bool sums = want_db && n0 == 0;           // wave-uniform: the first tile column also sums the rows of G
    const bool mma = want_dw != 0;
    float *row = part + size_t(range) * ld;

    f32x4 acc[4][4];
    zero_acc(acc);
    float rs[4] = {0.f, 0.f, 0.f, 0.f};             // row sums of G rows m0 + (tid >> 3) + 32 i, this thread's 8 columns of every k-tile

    Stage sa, sb;
    auto load = [&](int t) {
        const int img = img0 + t / dt, d0 = (t % dt) * BK;
        load_tile<false>(sa, G + size_t(img) * M * D, D, m0, M, d0, D, tid);
        if (mma) load_tile<false>(sb, X + size_t(img) * K * D, D, n0, K, d0, D, tid);
        if (sums) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float f[8];
                unpack8f(sa.v[i], f);
                rs[i] += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
            }
        }
    };
    load(0);
    if (mma) {
        store_tile<false>(sa, smem, tid);
        store_tile<false>(sb, smem + TILE_BYTES, tid);
    }
    __syncthreads();

    for (int kt = 0; kt < nk; kt++) {
        const char *ia = smem + (kt & 1) * 2 * TILE_BYTES;
        const bool more = kt + 1 < nk;
        if (more) load(kt + 1);
        if (mma) mma_tile<false, false>(acc, ia, ia + TILE_BYTES, wm, wn, lane);
        if (more && mma) {
            char *oa = smem + ((kt + 1) & 1) * 2 * TILE_BYTES;
            store_tile<false>(sa, oa, tid);
            store_tile<false>(sb, oa + TILE_BYTES, tid);
        }
        __syncthreads();
    }
    mfma_fence();

    if (mma) {
        // acc[i][j][r] = dW[m][n], m = m0 + wm 64 + 16 i + (lane & 15), n = n0 + wn 64 + 16 j + 4 (lane >> 4) + r; K may be
        // odd, so the partial is stored element by element (dW is small: the operand traffic is B D / 128 times larger)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int m = m0 + wm * 64 + i * 16 + (lane & 15);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (m < M && n + r < K) row[size_t(m) * K + n + r] = acc[i][j][r];
            }
        }
    }
    if (sums) {
        // the 8 threads tid & 7 of a row are neighbouring lanes of one wave
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float v = rs[i];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            const int m = m0 + (tid >> 3) + 32 * i;
            if ((tid & 7) == 0 && m < M) row[size_t(M) * K + m] = v;
        }
    }
}

template <bool W_KM>
void launch_left(const sfcvit_tokmix_args &a, const TokmixPlan &p, bool heavy, hipStream_t s) {
    const int tiles = p.tiles_m * p.tiles_n;
    if (heavy) hipLaunchKernelGGL((tokmix_left_kernel<W_KM, true>), dim3(p.grid), dim3(THREADS), 4 * TILE_BYTES, s, a, p.wunit, p.tiles_n, tiles);
    else hipLaunchKernelGGL((tokmix_left_kernel<W_KM, false>), dim3(p.grid), dim3(THREADS), 4 * TILE_BYTES, s, a, p.wunit, p.tiles_n, tiles);
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_tokmix_left(const sfcvit_tokmix_args *a, void *stream) {
    const TokmixPlan p = tokmix_left_plan(a);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool heavy = a->act == SFCVIT_ACT_GELU || a->aux_in != nullptr;
    if (a->w_transposed) launch_left<true>(*a, p, heavy, s);
    else launch_left<false>(*a, p, heavy, s);
    g_tokmix.set("tokmix_left_kernel<%s, %s>", a->w_transposed ? "true" : "false", heavy ? "true" : "false");
    return check_launch("tokmix_left");
}

extern "C" int sfcvit_tokmix_wgrad(const void *g, const void *x, void *dw, void *db, int grads_bf16, int B, int M, int K, int D,
                                   void *workspace, int64_t workspace_bytes, void *stream) {
    const TokmixPlan p = tokmix_wgrad_plan("tokmix_wgrad", B, M, K, D);
    if (int rc = tokmix_check_wgrad(p, g, x, dw, db, workspace, workspace_bytes)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(workspace);
    // without dW only the first tile column has work (the row sums)
    const int tiles_n = dw ? p.tiles_n : 1;
    const int tiles = p.tiles_m * tiles_n;
    hipLaunchKernelGGL(tokmix_wgrad_kernel, dim3(tiles * p.ranges), dim3(gemm_core::THREADS), 4 * gemm_core::TILE_BYTES, s,
                       static_cast<const uint16_t *>(g), static_cast<const uint16_t *>(x), part, B, M, K, D, tiles_n, tiles,
                       p.per_range, p.ld, dw ? 1 : 0, db ? 1 : 0);
    g_tokmix.set("tokmix_wgrad_kernel");
    if (int rc = check_launch("tokmix_wgrad")) return rc;
    if (dw)
        if (int rc = reduce_cols(part, p.ranges, p.ld, M * K, dw, grads_bf16, stream)) return rc;
    if (db)
        if (int rc = reduce_cols(part + size_t(M) * K, p.ranges, p.ld, M, db, grads_bf16, stream)) return rc;
    return SFCVIT_OK;
}
