// Depth-wise conv1d along the token sequence of a [B, N, D] bf16 activation, D contiguous (include/sfcvit.h,
// "TokenAggregator"): the first stage of TokenAggregator (src/models/vit.py:20-42), forward and backward.
//
// Every kernel is memory-bound (k multiply-adds per 2-byte element).  A lane owns 8 adjacent channels -- one 16-byte
// load or store per row -- and walks a run of consecutive rows of ONE image; a workgroup is 32 such lanes across a
// 256-channel slab times 8 consecutive runs.  Runs never cross an image: a tap outside 0 .. N - 1 is a zero row.
//   k = 3, s = 1 (the reference's default): the last three rows of x (and of du in backward) stay in registers, so a lane
//     fetches each row once; only the two halo rows of a run are fetched by its neighbour as well (same workgroup: L1 / L2).
//   any other (k, s), k compile-time, s run-time: a loop over the taps that re-reads neighbouring rows through the cache.
// Backward is ONE kernel: dx, and per-lane fp32 sums of dw / db that the workgroup adds over its 8 runs through LDS in a
// fixed order and writes as one partial row [D * k | D] per workgroup into the caller's workspace; the library's fixed-order
// column reduction (reduce_cols: fp32 or bf16 output, deferrable) finishes them.  No atomics: two runs give the same bits.
#include "common_host.h"
#include "device_common.h"
#include "token_agg.h"

namespace sfcvit {
namespace {

struct Row8 { float v[8]; };

__device__ __forceinline__ Row8 zero_row() {
    Row8 r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.v[j] = 0.f;
    return r;
}
__device__ __forceinline__ Row8 load_row(const uint16_t *p) {
    const u32x4 q = *reinterpret_cast<const u32x4 *>(p);
    Row8 r;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        r.v[2 * i] = bf2f(uint16_t(q[i]));
        r.v[2 * i + 1] = bf2f(uint16_t(q[i] >> 16));
    }
    return r;
}
__device__ __forceinline__ void store_row(uint16_t *p, const Row8 &r) {
    u32x4 q;
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = pack2bf(r.v[2 * i], r.v[2 * i + 1]);
    *reinterpret_cast<u32x4 *>(p) = q;
}
// acc += w * x per channel (fp32)
__device__ __forceinline__ void fma_row(Row8 &acc, const float *w, const Row8 &x) {
#pragma unroll
    for (int j = 0; j < 8; j++) acc.v[j] = fmaf(w[j], x.v[j], acc.v[j]);
}
__device__ __forceinline__ void mac_row(float *acc, const Row8 &a, const Row8 &b) {
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = fmaf(a.v[j], b.v[j], acc[j]);
}

// wt[t][j] = w[c + j][t]: the lane's 8 channels x K taps, from the [D, K] weight
template <int K>
__device__ __forceinline__ void load_weights(const uint16_t *__restrict__ w, int c, float (&wt)[K][8]) {
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int t = 0; t < K; t++) wt[t][j] = bf2f(w[size_t(c + j) * K + t]);
}
__device__ __forceinline__ Row8 load_bias(const uint16_t *__restrict__ bias, int c) {
    Row8 b = zero_row();
    if (bias) {
#pragma unroll
        for (int j = 0; j < 8; j++) b.v[j] = bf2f(bias[c + j]);
    }
    return b;
}

// The workgroup's sum of one per-lane quantity over its 8 runs, in run order, into its partial row.
// col(ch) = where channel ch of this quantity sits in the row.  Every thread of the workgroup calls it.
template <class Col>
__device__ __forceinline__ void block_sum_store(float (&red)[DWC_RL][DWC_CV * 8], const float *acc, float *__restrict__ row, int D, Col col) {
    const int cv = threadIdx.x & (DWC_CV - 1), rl = threadIdx.x / DWC_CV;
#pragma unroll
    for (int j = 0; j < 8; j++) red[rl][cv * 8 + j] = acc[j];
    __syncthreads();
    const int ch = blockIdx.x * (DWC_CV * 8) + threadIdx.x;
    if (ch < D) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < DWC_RL; r++) t += red[r][threadIdx.x];
        row[col(ch)] = t;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------
// k = 3, s = 1
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DWC_THREADS) void dwconv3_fwd_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ w,
                                                                  const uint16_t *__restrict__ bias, uint16_t *__restrict__ u,
                                                                  int N, int D, int run) {
    const int cv = threadIdx.x & (DWC_CV - 1), rl = threadIdx.x / DWC_CV;
    const int c = (blockIdx.x * DWC_CV + cv) * 8;
    const int n0 = (blockIdx.y * DWC_RL + rl) * run, n1 = min(N, n0 + run);
    if (c >= D || n0 >= n1) return;
    const size_t img = size_t(blockIdx.z) * size_t(N) * size_t(D) + c;
    const uint16_t *xp = x + img;
    uint16_t *up = u + img;
    float wt[3][8];
    load_weights<3>(w, c, wt);
    const Row8 b = load_bias(bias, c);
    Row8 prev = n0 > 0 ? load_row(xp + size_t(n0 - 1) * D) : zero_row();
    Row8 cur = load_row(xp + size_t(n0) * D);
    auto emit = [&](int n, const Row8 &next) {
        Row8 acc = b;
        fma_row(acc, wt[0], prev);
        fma_row(acc, wt[1], cur);
        fma_row(acc, wt[2], next);
        store_row(up + size_t(n) * D, acc);
        prev = cur;
        cur = next;
    };
    const int n1e = min(n1, N - 1);          // rows whose right neighbour exists
#pragma unroll 4
    for (int n = n0; n < n1e; n++) emit(n, load_row(xp + size_t(n + 1) * D));
    if (n1 == N) emit(N - 1, zero_row());
}

// DX: write dx.  DW: accumulate dw / db partials (x is read only then).
template <bool DX, bool DW>
__global__ __launch_bounds__(DWC_THREADS) void dwconv3_bwd_kernel(const uint16_t *__restrict__ du, const uint16_t *__restrict__ x,
                                                                  const uint16_t *__restrict__ w, uint16_t *__restrict__ dx,
                                                                  float *__restrict__ part, int N, int D, int run, int ld) {
    __shared__ float red[DWC_RL][DWC_CV * 8];
    const int cv = threadIdx.x & (DWC_CV - 1), rl = threadIdx.x / DWC_CV;
    const int c = (blockIdx.x * DWC_CV + cv) * 8;
    const int n0 = (blockIdx.y * DWC_RL + rl) * run, n1 = min(N, n0 + run);
    float aw[3][8], ab[8];
#pragma unroll
    for (int j = 0; j < 8; j++) aw[0][j] = aw[1][j] = aw[2][j] = ab[j] = 0.f;
    if (c < D && n0 < n1) {
        const size_t img = size_t(blockIdx.z) * size_t(N) * size_t(D) + c;
        const uint16_t *dp = du + img, *xp = DW ? x + img : nullptr;
        uint16_t *op = DX ? dx + img : nullptr;
        float wt[3][8];
        if constexpr (DX) load_weights<3>(w, c, wt);
        Row8 dprev = zero_row(), xprev = zero_row(), xcur = zero_row();
        Row8 dcur = load_row(dp + size_t(n0) * D);
        if (DX && n0 > 0) dprev = load_row(dp + size_t(n0 - 1) * D);
        if constexpr (DW) {
            if (n0 > 0) xprev = load_row(xp + size_t(n0 - 1) * D);
            xcur = load_row(xp + size_t(n0) * D);
        }
        auto step = [&](int m, const Row8 &dnext, const Row8 &xnext) {
            if constexpr (DX) {          // dx[m] = w0 du[m + 1] + w1 du[m] + w2 du[m - 1], in tap order
                Row8 acc = zero_row();
                fma_row(acc, wt[0], dnext);
                fma_row(acc, wt[1], dcur);
                fma_row(acc, wt[2], dprev);
                store_row(op + size_t(m) * D, acc);
                dprev = dcur;
            }
            if constexpr (DW) {          // dw[t] += du[m] x[m + t - 1];  db += du[m]
                mac_row(aw[0], dcur, xprev);
                mac_row(aw[1], dcur, xcur);
                mac_row(aw[2], dcur, xnext);
#pragma unroll
                for (int j = 0; j < 8; j++) ab[j] += dcur.v[j];
                xprev = xcur;
                xcur = xnext;
            }
            dcur = dnext;
        };
        const int n1e = min(n1, N - 1);
#pragma unroll 2
        for (int m = n0; m < n1e; m++) {
            const Row8 dnext = load_row(dp + size_t(m + 1) * D);
            const Row8 xnext = DW ? load_row(xp + size_t(m + 1) * D) : zero_row();
            step(m, dnext, xnext);
        }
        if (n1 == N) step(N - 1, zero_row(), zero_row());
    }
    if constexpr (DW) {
        float *row = part + (size_t(blockIdx.z) * gridDim.y + blockIdx.y) * size_t(ld);
#pragma unroll
        for (int t = 0; t < 3; t++) block_sum_store(red, aw[t], row, D, [&](int ch) { return ch * 3 + t; });
        block_sum_store(red, ab, row, D, [&](int ch) { return D * 3 + ch; });
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// any k (compile-time), any s (run-time): neighbouring rows re-read through the cache
// ---------------------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(DWC_THREADS) void dwconv_fwd_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ w,
                                                                 const uint16_t *__restrict__ bias, uint16_t *__restrict__ u,
                                                                 int N, int Nout, int D, int s, int run) {
    constexpr int PAD = K / 2;
    const int cv = threadIdx.x & (DWC_CV - 1), rl = threadIdx.x / DWC_CV;
    const int c = (blockIdx.x * DWC_CV + cv) * 8;
    const int n0 = (blockIdx.y * DWC_RL + rl) * run, n1 = min(Nout, n0 + run);
    if (c >= D || n0 >= n1) return;
    const uint16_t *xp = x + size_t(blockIdx.z) * size_t(N) * size_t(D) + c;
    uint16_t *up = u + size_t(blockIdx.z) * size_t(Nout) * size_t(D) + c;
    float wt[K][8];
    load_weights<K>(w, c, wt);
    const Row8 b = load_bias(bias, c);
    for (int n = n0; n < n1; n++) {
        Row8 acc = b;
#pragma unroll
        for (int t = 0; t < K; t++) {
            const int r = n * s + t - PAD;
            if (r >= 0 && r < N) fma_row(acc, wt[t], load_row(xp + size_t(r) * D));
        }
        store_row(up + size_t(n) * D, acc);
    }
}

// dx (may be NULL) over the lane's run of INPUT rows, dw / db partials (part may be NULL) over its run of OUTPUT rows.
template <int K>
__global__ __launch_bounds__(DWC_THREADS) void dwconv_bwd_kernel(const uint16_t *__restrict__ du, const uint16_t *__restrict__ x,
                                                                 const uint16_t *__restrict__ w, uint16_t *__restrict__ dx,
                                                                 float *__restrict__ part, int N, int Nout, int D, int s, int run_in,
                                                                 int run_out, int ld) {
    constexpr int PAD = K / 2;
    __shared__ float red[DWC_RL][DWC_CV * 8];
    const int cv = threadIdx.x & (DWC_CV - 1), rl = threadIdx.x / DWC_CV;
    const int c = (blockIdx.x * DWC_CV + cv) * 8;
    const int lane_run = blockIdx.y * DWC_RL + rl;
    float aw[K][8], ab[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        ab[j] = 0.f;
#pragma unroll
        for (int t = 0; t < K; t++) aw[t][j] = 0.f;
    }
    if (c < D) {
        const uint16_t *dp = du + size_t(blockIdx.z) * size_t(Nout) * size_t(D) + c;
        const size_t img_in = size_t(blockIdx.z) * size_t(N) * size_t(D) + c;
        if (dx) {
            float wt[K][8];
            load_weights<K>(w, c, wt);
            const int m0 = lane_run * run_in, m1 = min(N, m0 + run_in);
            for (int m = m0; m < m1; m++) {
                Row8 acc = zero_row();
#pragma unroll
                for (int t = 0; t < K; t++) {
                    const int q = m + PAD - t;             // = n * s for the output row n this tap reached m from
                    if (q >= 0 && q % s == 0 && q / s < Nout) fma_row(acc, wt[t], load_row(dp + size_t(q / s) * D));
                }
                store_row(dx + img_in + size_t(m) * D, acc);
            }
        }
        if (part) {
            const int n0 = lane_run * run_out, n1 = min(Nout, n0 + run_out);
            for (int n = n0; n < n1; n++) {
                const Row8 d = load_row(dp + size_t(n) * D);
#pragma unroll
                for (int j = 0; j < 8; j++) ab[j] += d.v[j];
                if (x) {
#pragma unroll
                    for (int t = 0; t < K; t++) {
                        const int r = n * s + t - PAD;
                        if (r >= 0 && r < N) mac_row(aw[t], d, load_row(x + img_in + size_t(r) * D));
                    }
                }
            }
        }
    }
    if (part) {                                            // uniform over the grid: every thread reaches the barriers
        float *row = part + (size_t(blockIdx.z) * gridDim.y + blockIdx.y) * size_t(ld);
#pragma unroll
        for (int t = 0; t < K; t++) block_sum_store(red, aw[t], row, D, [&](int ch) { return ch * K + t; });
        block_sum_store(red, ab, row, D, [&](int ch) { return D * K + ch; });
    }
}

using u16 = uint16_t;

template <int K>
void launch_fwd(const DwconvPlan &p, dim3 grid, hipStream_t st, const u16 *x, const u16 *w, const u16 *bias, u16 *u, int N, int D, int s) {
    hipLaunchKernelGGL(dwconv_fwd_kernel<K>, grid, dim3(DWC_THREADS), 0, st, x, w, bias, u, N, p.Nout, D, s, p.run_out);
}
template <int K>
void launch_bwd(const DwconvPlan &p, dim3 grid, hipStream_t st, const u16 *du, const u16 *x, const u16 *w, u16 *dx, float *part, int N,
                int D, int s) {
    hipLaunchKernelGGL(dwconv_bwd_kernel<K>, grid, dim3(DWC_THREADS), 0, st, du, x, w, dx, part, N, p.Nout, D, s, p.run_in, p.run_out,
                       p.ld);
}
#define DWC_FOR_K(k, CALL)                                                                                                      \
    switch (k) {                                                                                                                \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; case 5: CALL(5); break;     \
    case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break; default: CALL(9); break;                            \
    }

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_dwconv1d_fwd(const void *x, const void *w, const void *bias, void *u, int B, int N, int D, int k, int s,
                                   void *stream) {
    const DwconvPlan p = dwconv_plan("dwconv1d_fwd", B, N, D, k, s);
    if (int rc = dwconv_check_fwd(p, x, w, u)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(p.slabs, p.groups, B);
    const u16 *xs = static_cast<const u16 *>(x), *ws = static_cast<const u16 *>(w), *bs = static_cast<const u16 *>(bias);
    u16 *us = static_cast<u16 *>(u);
    if (p.spec) {
        hipLaunchKernelGGL(dwconv3_fwd_kernel, grid, dim3(DWC_THREADS), 0, st, xs, ws, bs, us, N, D, p.run_out);
        g_dwconv.set("dwconv3_fwd_kernel");
    } else {
#define CALL(KK) launch_fwd<KK>(p, grid, st, xs, ws, bs, us, N, D, s)
        DWC_FOR_K(k, CALL)
#undef CALL
        g_dwconv.set("dwconv_fwd_kernel<%d>", k);
    }
    return check_launch("dwconv1d_fwd");
}

extern "C" int sfcvit_dwconv1d_bwd(const void *du, const void *x, const void *w, void *dx, void *dw, void *db, int grads_bf16, int B,
                                   int N, int D, int k, int s, void *workspace, int64_t workspace_bytes, void *stream) {
    const DwconvPlan p = dwconv_plan("dwconv1d_bwd", B, N, D, k, s);
    if (int rc = dwconv_check_bwd(p, du, x, w, dx, dw, db, workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(p.slabs, p.groups, B);
    const u16 *ds = static_cast<const u16 *>(du), *xs = static_cast<const u16 *>(x), *ws = static_cast<const u16 *>(w);
    u16 *dxs = static_cast<u16 *>(dx);
    const bool sums = dw || db;
    float *part = sums ? static_cast<float *>(workspace) : nullptr;
    if (p.spec && (!sums || x)) {
        if (dx && sums) hipLaunchKernelGGL((dwconv3_bwd_kernel<true, true>), grid, dim3(DWC_THREADS), 0, st, ds, xs, ws, dxs, part, N, D, p.run_out, p.ld);
        else if (dx) hipLaunchKernelGGL((dwconv3_bwd_kernel<true, false>), grid, dim3(DWC_THREADS), 0, st, ds, xs, ws, dxs, part, N, D, p.run_out, p.ld);
        else hipLaunchKernelGGL((dwconv3_bwd_kernel<false, true>), grid, dim3(DWC_THREADS), 0, st, ds, xs, ws, dxs, part, N, D, p.run_out, p.ld);
        g_dwconv.set("dwconv3_bwd_kernel<%s, %s>", dx ? "true" : "false", sums ? "true" : "false");
    } else {          // (also k = 3, s = 1 asked for db alone, without x)
#define CALL(KK) launch_bwd<KK>(p, grid, st, ds, xs, ws, dxs, part, N, D, s)
        DWC_FOR_K(k, CALL)
#undef CALL
        g_dwconv.set("dwconv_bwd_kernel<%d>", k);
    }
    if (int rc = check_launch("dwconv1d_bwd")) return rc;
    const int nparts = B * p.groups;
    if (dw)
        if (int rc = reduce_cols(part, nparts, p.ld, D * k, dw, grads_bf16, stream)) return rc;
    if (db)
        if (int rc = reduce_cols(part + size_t(D) * k, nparts, p.ld, D, db, grads_bf16, stream)) return rc;
    return SFCVIT_OK;
}
