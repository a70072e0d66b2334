// HBM-bound row-wise kernels for gfx950: column sums (bias gradients) with the deferred reduce queue, transposes, GELU, the
// dropout mask and soft-target cross-entropy.  Every global access is a 16-byte vector (8 bf16 or 4 fp32) and reductions are
// wave butterflies.  LayerNorm lives in layernorm.hip, the optimizer in optim.hip; the launchers run what the plans of
// rowwise.h say.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>
#include "common_host.h"
#include "model_ema.h"
#include "rowwise_device.h"

namespace sfcvit {
namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
static_assert(THREADS == ROW_THREADS, "rowwise.h plans the grids for this file's workgroup size");
// grid_for below and the optimizer's plans (ADAMW_THREADS / ADAMW_MAX_BLOCKS, model_ema.h) size grid-stride launches alike
static_assert(ADAMW_THREADS == THREADS, "model_ema.h plans the grid for this file's workgroup size");

// ---------------------------------------------------------------------------
// Column sums of a bf16 [M, ld] matrix (bias gradients).
// Thread (cv, rl) owns 8 columns and every 8th row of the block's row range.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void colsum_kernel(const uint16_t *__restrict__ x, int M, int N, int ld,
                                                         int rows_per_block, float *__restrict__ out) {
    __shared__ float red[8][256];
    const int cv = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int col = blockIdx.x * 256 + cv * 8;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(M, r0 + rows_per_block);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (col < N) {
        for (int r = r0 + rl; r < r1; r += 8) {
            float v[8];
            unpack8(*reinterpret_cast<const u32x4 *>(x + size_t(r) * ld + col), v);
#pragma unroll
            for (int j = 0; j < 8; j++) s[j] += v[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) red[rl][cv * 8 + j] = s[j];
    __syncthreads();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < N) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 8; r++) t += red[r][threadIdx.x];
        out[size_t(blockIdx.y) * N + c] = t;          // partial[row block][column]
    }
}

// Many such reductions in one launch (sfcvit_reduce_flush): a workgroup finds its item by the first-block table.
constexpr int RED_BATCH = 96;
struct ReduceItem {
    const float *part;
    void *out;
    int nparts, ld, ncols, out_bf16;
};
struct ReduceBatch {                 // by value in the kernel arguments: 96 x 32 + 98 x 4 bytes < 4 KiB
    ReduceItem it[RED_BATCH];
    int first[RED_BATCH + 1];        // first workgroup of item i; first[n] = grid size
    int n;
};
__global__ __launch_bounds__(RED_THREADS) void reduce_batched_kernel(const ReduceBatch b) {
    int lo = 0, hi = b.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (b.first[mid] <= int(blockIdx.x)) lo = mid; else hi = mid;
    }
    const float *part = b.it[lo].part;
    void *out = b.it[lo].out;
    const int nparts = b.it[lo].nparts, ld = b.it[lo].ld, ncols = b.it[lo].ncols, as_bf16 = b.it[lo].out_bf16;
    const int c = (int(blockIdx.x) - b.first[lo]) * 16 + (threadIdx.x & 15);
    const float t = reduce_partials16(part, nparts, ld, c, c < ncols);
    if (threadIdx.x < 16 && c < ncols) store_grad(out, c, t, as_bf16);
}

// ---------------------------------------------------------------------------
// bf16 matrix transpose: dst[c][r] = src[r][c], 64 x 64 tiles through LDS (16-byte global
// accesses on both sides).  Used once per step per weight so that dX = dY W runs with both
// operands k-contiguous (the layout the LDS-DMA GEMM is fastest on).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void transpose_kernel(const uint16_t *__restrict__ src, int R, int C, int lds,
                                                            uint16_t *__restrict__ dst, int ldd) {
    __shared__ uint16_t tile[64][66];                       // 66: odd dword stride, conflict-free column reads
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; i++) {                           // 64 rows x 8 vectors
        const int v = t + THREADS * i, r = v >> 3, cv = (v & 7) * 8;
        u32x4 val = {0u, 0u, 0u, 0u};
        if (r0 + r < R && c0 + cv < C) val = *reinterpret_cast<const u32x4 *>(src + size_t(r0 + r) * lds + c0 + cv);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            tile[r][cv + 2 * j] = uint16_t(val[j]);
            tile[r][cv + 2 * j + 1] = uint16_t(val[j] >> 16);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int v = t + THREADS * i, c = v >> 3, rv = (v & 7) * 8;
        if (c0 + c < C && r0 + rv < R) {
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; j++) o[j] = uint32_t(tile[rv + 2 * j][c]) | (uint32_t(tile[rv + 2 * j + 1][c]) << 16);
            *reinterpret_cast<u32x4 *>(dst + size_t(c0 + c) * ldd + r0 + rv) = o;
        }
    }
}

// One launch for many matrices: a workgroup looks its 64 x 64 tile up in a device table (sfcvit_transpose_batched).
__global__ __launch_bounds__(THREADS) void transpose_batched_kernel(const uint16_t *__restrict__ src_base, uint16_t *__restrict__ dst_base,
                                                                    const sfcvit_transpose_tile *__restrict__ tiles) {
    __shared__ uint16_t tile[64][66];
    const sfcvit_transpose_tile d = tiles[blockIdx.x];
    const uint16_t *src = src_base + d.src_off;
    uint16_t *dst = dst_base + d.dst_off;
    const int R = d.R, C = d.C, r0 = d.r0, c0 = d.c0, t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int v = t + THREADS * i, r = v >> 3, cv = (v & 7) * 8;
        u32x4 val = {0u, 0u, 0u, 0u};
        if (r0 + r < R && c0 + cv < C) val = *reinterpret_cast<const u32x4 *>(src + size_t(r0 + r) * C + c0 + cv);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            tile[r][cv + 2 * j] = uint16_t(val[j]);
            tile[r][cv + 2 * j + 1] = uint16_t(val[j] >> 16);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int v = t + THREADS * i, c = v >> 3, rv = (v & 7) * 8;
        if (c0 + c < C && r0 + rv < R) {
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; j++) o[j] = uint32_t(tile[rv + 2 * j][c]) | (uint32_t(tile[rv + 2 * j + 1][c]) << 16);
            *reinterpret_cast<u32x4 *>(dst + size_t(c0 + c) * R + r0 + rv) = o;
        }
    }
}

// ---------------------------------------------------------------------------
// GELU (erf form)
// ---------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(THREADS) void gelu_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                       uint16_t *__restrict__ out, int64_t nvec) {
    for (int64_t i = blockIdx.x * int64_t(THREADS) + threadIdx.x; i < nvec; i += int64_t(gridDim.x) * THREADS) {
        float xv[8], o[8];
        unpack8(*reinterpret_cast<const u32x4 *>(x + i * 8), xv);
        if (BWD) {
            float dv[8];
            unpack8(*reinterpret_cast<const u32x4 *>(dy + i * 8), dv);
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = dv[j] * gelu_erf_grad(xv[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = gelu_erf(xv[j]);
        }
        *reinterpret_cast<u32x4 *>(out + i * 8) = pack8(o);
    }
}

// GELU followed by dropout on a [rows, cols] tensor (cols % 8 == 0); one 8-vector per thread-iteration.
template <bool BWD>
__global__ __launch_bounds__(THREADS) void gelu_drop_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                            uint16_t *__restrict__ out, int rows, int cols, float p,
                                                            uint32_t seed_arg, const uint32_t *__restrict__ seed_off) {
    const uint32_t seed = eff_seed(seed_arg, seed_off);
    const uint32_t th = drop_thresh(p);
    const float sc = 1.f / (1.f - p);
    const int vpr = cols >> 3;
    const int64_t nvec = int64_t(rows) * vpr;
    for (int64_t i = blockIdx.x * int64_t(THREADS) + threadIdx.x; i < nvec; i += int64_t(gridDim.x) * THREADS) {
        const int64_t row = i / vpr;
        const int cv = int(i - row * vpr);
        float xv[8], o[8];
        unpack8(*reinterpret_cast<const u32x4 *>(x + i * 8), xv);
        if (BWD) {
            float dv[8];
            unpack8(*reinterpret_cast<const u32x4 *>(dy + i * 8), dv);
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = dv[j] * gelu_erf_grad(xv[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = gelu_erf(xv[j]);
        }
        const uint32_t rk = drop_row_key(seed, uint64_t(row));
#pragma unroll
        for (int q = 0; q < 4; q++) {
            bool k0, k1;
            drop_keep2(rk, uint32_t(cv * 4 + q), th, k0, k1);
            o[2 * q] = k0 ? o[2 * q] * sc : 0.f;
            o[2 * q + 1] = k1 ? o[2 * q + 1] * sc : 0.f;
        }
        *reinterpret_cast<u32x4 *>(out + i * 8) = pack8(o);
    }
}

__global__ __launch_bounds__(THREADS) void dropout_mask_kernel(uint16_t *__restrict__ out, int64_t rows, int cols, float p,
                                                               uint32_t seed) {
    const uint32_t th = drop_thresh(p);
    const uint16_t on = f2bf(1.f / (1.f - p));
    const int ppr = (cols + 1) >> 1;
    const int64_t npair = rows * ppr;
    for (int64_t i = blockIdx.x * int64_t(THREADS) + threadIdx.x; i < npair; i += int64_t(gridDim.x) * THREADS) {
        const int64_t row = i / ppr;
        const int c = int(i - row * ppr) * 2;
        bool k0, k1;
        drop_keep2(drop_row_key(seed, uint64_t(row)), uint32_t(c >> 1), th, k0, k1);
        out[row * cols + c] = k0 ? on : uint16_t(0);
        if (c + 1 < cols) out[row * cols + c + 1] = k1 ? on : uint16_t(0);
    }
}

// ---------------------------------------------------------------------------
// Soft-target cross entropy: one wave per row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void soft_ce_kernel(const uint16_t *__restrict__ logits,
                                                          const float *__restrict__ targets,
                                                          float *__restrict__ loss_rows, uint16_t *__restrict__ dlogits,
                                                          int B, int C, int ld, float gscale) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (row >= B) return;
    const uint16_t *l = logits + size_t(row) * ld;
    const float *t = targets + size_t(row) * C;
    float mx = -INFINITY;
    int am = C;                                       // this lane's first column that holds its maximum
    for (int c = lane; c < C; c += 64) {
        const float z = bf2f(l[c]);
        if (z > mx) am = c;
        mx = fmaxf(mx, z);
    }
    const float lane_mx = mx;
    mx = wave_max(mx);
    if (lane_mx != mx) am = C;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 64));   // the row's first maximum
    // se, and beside it the same sum without the term of the maximum (soft_ce_pair_kernel's remedy, mix.hip): at that column
    // 1 - softmax is so / se, where 1 - exp(z - lse) loses every digit once the model is sure of the label
    float se = 0.f, so = 0.f, st = 0.f, stl = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float z = bf2f(l[c]);
        const float e = __expf(z - mx);
        se += e;
        so += c == am ? 0.f : e;
        st += t[c];
        stl += t[c] * z;
    }
    se = wave_sum(se);
    so = wave_sum(so);
    st = wave_sum(st);
    stl = wave_sum(stl);
    const float lse = mx + __logf(se);
    if (lane == 0) loss_rows[row] = lse * st - stl;   // -sum t*(z - lse)
    if (dlogits) {
        uint16_t *d = dlogits + size_t(row) * ld;
        const float omp_max = so / se;
        for (int c = lane; c < ld; c += 64) {
            float gr = 0.f;
            if (c < C) {
                // softmax * sum(t) - t, written as p * (sum(t) - t) - t * (1 - p): no cancellation in either factor
                const float p = __expf(bf2f(l[c]) - lse), tc = t[c];
                gr = (p * (st - tc) - tc * (c == am ? omp_max : 1.f - p)) * gscale;
            }
            d[c] = f2bf(gr);
        }
    }
}

// Workgroups of GELU and the dropout mask: one lane per work item, 1 .. 2048 (the optimizer's cap, ADAMW_MAX_BLOCKS).
int grid_for(int64_t work_items) {
    int64_t b = (work_items + THREADS - 1) / THREADS;
    if (b < 1) b = 1;
    return int(b > 2048 ? 2048 : b);
}
static_assert(ADAMW_MAX_BLOCKS == 2048, "grid_for's cap is the optimizer's");

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

namespace sfcvit {
namespace {
std::atomic<int> g_defer{0};
std::mutex g_reduce_mutex;
std::vector<ReduceItem> g_reduce_queue;
}  // namespace

bool reduce_deferring() { return g_defer.load(std::memory_order_relaxed) != 0; }

int reduce_cols(const float *part, int nparts, int ld, int ncols, void *out, int out_bf16, void *stream) {
    if (reduce_deferring()) {
        std::lock_guard<std::mutex> lock(g_reduce_mutex);
        g_reduce_queue.push_back(ReduceItem{part, out, nparts, ld, ncols, out_bf16});
        return SFCVIT_OK;
    }
    ReduceBatch b;
    b.it[0] = ReduceItem{part, out, nparts, ld, ncols, out_bf16};
    b.first[0] = 0;
    b.first[1] = (ncols + 15) / 16;
    b.n = 1;
    hipLaunchKernelGGL(reduce_batched_kernel, dim3(b.first[1]), dim3(RED_THREADS), 0, static_cast<hipStream_t>(stream), b);
    return check_launch("column reduce");
}

int launch_colsum_reduce(const float *part, int nparts, int N, void *out, int out_bf16, void *stream) {
    return reduce_cols(part, nparts, N, N, out, out_bf16, stream);
}
}  // namespace sfcvit

extern "C" int sfcvit_reduce_defer(int on) { return g_defer.exchange(on ? 1 : 0); }

extern "C" int sfcvit_reduce_pending(void) {
    std::lock_guard<std::mutex> lock(g_reduce_mutex);
    return int(g_reduce_queue.size());
}

extern "C" int sfcvit_reduce_discard(void) {
    std::lock_guard<std::mutex> lock(g_reduce_mutex);
    g_reduce_queue.clear();
    return SFCVIT_OK;
}

extern "C" int sfcvit_reduce_flush(void *stream) {
    std::vector<ReduceItem> items;
    {
        std::lock_guard<std::mutex> lock(g_reduce_mutex);
        items.swap(g_reduce_queue);
    }
    for (size_t i0 = 0; i0 < items.size(); i0 += RED_BATCH) {
        ReduceBatch b;
        b.n = int(std::min(items.size() - i0, size_t(RED_BATCH)));
        int blocks = 0;
        for (int i = 0; i < b.n; i++) {
            b.it[i] = items[i0 + i];
            b.first[i] = blocks;
            blocks += (b.it[i].ncols + 15) / 16;
        }
        b.first[b.n] = blocks;
        hipLaunchKernelGGL(reduce_batched_kernel, dim3(blocks), dim3(RED_THREADS), 0, static_cast<hipStream_t>(stream), b);
        if (int rc = check_launch("batched column reduce")) return rc;
    }
    return SFCVIT_OK;
}

extern "C" int64_t sfcvit_colsum_workspace(int M, int N) {
    if (M <= 0 || N <= 0) return 0;
    return colsum_geometry(M, N).ws_bytes;
}

extern "C" int sfcvit_colsum(const void *x, int M, int N, int ld, void *out, int out_bf16, void *workspace,
                             int64_t workspace_bytes, void *stream) {
    const ColsumPlan p = colsum_plan(x, M, N, ld, out, workspace, workspace_bytes);
    if (p.err) return fail(p.err, "%s", p.msg);
    float *part = static_cast<float *>(workspace);
    hipLaunchKernelGGL(colsum_kernel, dim3(p.col_blocks, p.row_blocks), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x), M, N, ld, p.rpb, part);
    if (int rc = check_launch("colsum")) return rc;
    return reduce_cols(part, p.row_blocks, N, N, out, out_bf16, stream);
}

extern "C" int sfcvit_transpose(const void *src, int R, int C, int lds, void *dst, int ldd, void *stream) {
    const RowGridPlan p = transpose_plan(src, R, C, lds, dst, ldd);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipLaunchKernelGGL(transpose_kernel, dim3(p.grid, p.grid_y), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(src), R, C, lds, static_cast<uint16_t *>(dst), ldd);
    return check_launch("transpose");
}

extern "C" int sfcvit_transpose_batched(const void *src_base, void *dst_base, const sfcvit_transpose_tile *tiles, int n_tiles,
                                        void *stream) {
    const RowGridPlan p = transpose_batched_plan(src_base, dst_base, tiles, n_tiles);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipLaunchKernelGGL(transpose_batched_kernel, dim3(p.grid), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(src_base), static_cast<uint16_t *>(dst_base), tiles);
    return check_launch("transpose_batched");
}

// GELU forward (dy = NULL) and backward share a launcher, without and with dropout.
static int launch_gelu(bool bwd, const void *dy, const void *x, void *out, int64_t n, void *stream) {
    const PlanStatus p = gelu_plan(bwd, dy, x, out, n);
    if (p.err) return fail(p.err, "%s", p.msg);
    const dim3 grid(grid_for(n / 8));
    const auto *dyp = static_cast<const uint16_t *>(dy), *xp = static_cast<const uint16_t *>(x);
    if (bwd) hipLaunchKernelGGL(gelu_kernel<true>, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), dyp, xp, static_cast<uint16_t *>(out), n / 8);
    else hipLaunchKernelGGL(gelu_kernel<false>, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), dyp, xp, static_cast<uint16_t *>(out), n / 8);
    return check_launch(bwd ? "gelu_bwd" : "gelu_fwd");
}

static int launch_gelu_drop(bool bwd, const void *dy, const void *x, void *out, int rows, int cols, float drop_p, uint32_t seed,
                            const uint32_t *seed_off, void *stream) {
    const PlanStatus p = gelu_drop_plan(bwd, dy, x, out, rows, cols, drop_p);
    if (p.err) return fail(p.err, "%s", p.msg);
    const dim3 grid(grid_for(int64_t(rows) * cols / 8));
    const auto *dyp = static_cast<const uint16_t *>(dy), *xp = static_cast<const uint16_t *>(x);
    if (bwd) hipLaunchKernelGGL(gelu_drop_kernel<true>, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), dyp, xp, static_cast<uint16_t *>(out), rows, cols, drop_p, seed, seed_off);
    else hipLaunchKernelGGL(gelu_drop_kernel<false>, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), dyp, xp, static_cast<uint16_t *>(out), rows, cols, drop_p, seed, seed_off);
    return check_launch(bwd ? "gelu_drop_bwd" : "gelu_drop_fwd");
}

extern "C" int sfcvit_gelu_fwd(const void *x, void *y, int64_t n, void *stream) { return launch_gelu(false, nullptr, x, y, n, stream); }

extern "C" int sfcvit_gelu_bwd(const void *dy, const void *x, void *dx, int64_t n, void *stream) {
    return launch_gelu(true, dy, x, dx, n, stream);
}

extern "C" int sfcvit_gelu_drop_fwd(const void *x, void *y, int rows, int cols, float p, uint32_t seed, const uint32_t *seed_off,
                                    void *stream) {
    return launch_gelu_drop(false, nullptr, x, y, rows, cols, p, seed, seed_off, stream);
}

extern "C" int sfcvit_gelu_drop_bwd(const void *dy, const void *x, void *dx, int rows, int cols, float p, uint32_t seed,
                                    const uint32_t *seed_off, void *stream) {
    return launch_gelu_drop(true, dy, x, dx, rows, cols, p, seed, seed_off, stream);
}

extern "C" int sfcvit_dropout_mask(void *out, int64_t rows, int cols, float p, uint32_t seed, void *stream) {
    const PlanStatus pl = dropout_mask_plan(out, rows, cols, p);
    if (pl.err) return fail(pl.err, "%s", pl.msg);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(rows * ((cols + 1) / 2))), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<uint16_t *>(out), rows, cols, p, seed);
    return check_launch("dropout_mask");
}

extern "C" int sfcvit_soft_ce(const void *logits, const float *targets, float *loss_rows, void *dlogits, int B, int C,
                              int ld, float gscale, void *stream) {
    const RowGridPlan p = soft_ce_plan(logits, targets, loss_rows, B, C, ld);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipLaunchKernelGGL(soft_ce_kernel, dim3(p.grid), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(logits), targets, loss_rows, static_cast<uint16_t *>(dlogits), B, C, ld, gscale);
    return check_launch("soft_ce");
}
