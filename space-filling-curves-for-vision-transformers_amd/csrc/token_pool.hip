// CLS token and pooled read-outs of a [B, N, D] bf16 activation, D contiguous (include/sfcvit.h, "CLS token and token
// pooling"): the reference's commented-out `x = torch.cat([cls_token.expand(B, -1, -1), x], dim=1)` (src/models/vit.py:
// 237-238), the read-out of token 0 its docstring promises, and the token mean of altvit.py -- with their backwards.
//
// All four are memory-bound and see the tensors as 16-byte vectors of 8 channels (dv = D / 8 per token row).
//   prepend forward:  a lane owns ONE vector of an image's [N + 1, D] output and moves it for `imgs` consecutive images
//             (1, 2, 4 or 8 independent loads in flight); the lanes of row 0 load the CLS vector once.  A short last group
//             re-reads image B - 1 through a clamped index and skips the store.  Bits move: nothing is converted.
//   prepend backward: ONE launch.  Workgroups [0, slabs) of grid.x form dcls: 8 lanes across a 64-column slab of the CLS
//             row times 32 lanes across images; lane rl adds images rl, rl + 32, ... of the workgroup's range in that
//             order and the 32 sums meet in LDS in lane order.  They come first in the grid because theirs is the longest
//             dependent chain.  The other workgroups copy dy[:, 1:, :] to dx as the forward copies.  Up to 2048 images
//             there is one range and the workgroup writes dcls itself, fp32 or bf16; a larger batch is split into ranges
//             whose fp32 partial rows the library's fixed-order reduction (reduce_cols: deferrable) adds.
//   pool forward:     a workgroup is cv lanes across a slab of cv x 8 columns of ONE image times tl = 256 / cv lanes across
//             the token range; lane tl adds tokens first + tl, first + tl + TL, ... in that order (four independent loads
//             in flight), the tl sums meet in LDS in lane order, one fp32 division, one rounding.  count == 1 is a copy
//             of the row's bits by a kernel of its own (a sum that starts from +0 would lose the sign of -0).
//   pool backward:    the same geometry; a lane forms its vector of dy / count once and stores it, or +0, to every token
//             row it owns: every element of dx is written by exactly one lane.
// No atomics, one writer per element: two runs give the same bits.
#include "common_host.h"
#include "device_common.h"
#include "token_pool.h"

namespace sfcvit {
namespace {

using u16 = uint16_t;

__device__ __forceinline__ u32x4 load16(const u16 *p) { return *reinterpret_cast<const u32x4 *>(p); }
__device__ __forceinline__ void store16(u16 *p, u32x4 v) { *reinterpret_cast<u32x4 *>(p) = v; }

__device__ __forceinline__ void add_vec(float (&s)[8], u32x4 q) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s[2 * i] += bf2f(u16(q[i]));
        s[2 * i + 1] += bf2f(u16(q[i] >> 16));
    }
}

// One vector position r of an image's [N + 1, D] rows, `IMGS` consecutive images.
template <int IMGS>
__device__ __forceinline__ void prepend_copy(const u16 *__restrict__ x, const u16 *__restrict__ cls, u16 *__restrict__ y, int B,
                                             int64_t xv, int dv, int64_t r, int b0) {
    u32x4 in[IMGS];
    if (r < dv) {
        const u32x4 c = load16(cls + r * 8);
#pragma unroll
        for (int i = 0; i < IMGS; i++) in[i] = c;
    } else {
#pragma unroll
        for (int i = 0; i < IMGS; i++) in[i] = load16(x + (int64_t(min(b0 + i, B - 1)) * xv + (r - dv)) * 8);
    }
#pragma unroll
    for (int i = 0; i < IMGS; i++)
        if (b0 + i < B) store16(y + (int64_t(b0 + i) * (xv + dv) + r) * 8, in[i]);
}

template <int IMGS>
__global__ __launch_bounds__(TP_THREADS) void cls_prepend_fwd_kernel(const u16 *__restrict__ x, const u16 *__restrict__ cls,
                                                                    u16 *__restrict__ y, int B, int64_t xv, int dv) {
    const int64_t r = int64_t(blockIdx.x) * TP_THREADS + threadIdx.x;
    if (r >= xv + dv) return;                                  // (no barrier in this kernel)
    prepend_copy<IMGS>(x, cls, y, B, xv, dv, r, blockIdx.y * IMGS);
}

// out_kind: 0 = fp32 partial row of this range (part[range][D]), 1 = dcls fp32, 2 = dcls bf16.  dx may be null: the grid
// then has the `slabs` dcls workgroups only.
template <int IMGS>
__global__ __launch_bounds__(TP_THREADS) void cls_prepend_bwd_kernel(const u16 *__restrict__ dy, u16 *__restrict__ dx,
                                                                    void *__restrict__ out, int out_kind, int B, int rows,
                                                                    int64_t xv, int dv, int slabs, int groups) {
    __shared__ float red[CP_RL][CP_CV * 8];
    if (int(blockIdx.x) >= slabs) {                            // workgroup-uniform: a copy workgroup meets no barrier
        const int64_t r = int64_t(blockIdx.x - slabs) * TP_THREADS + threadIdx.x;
        if (r >= xv || int(blockIdx.y) >= groups) return;
        const int b0 = blockIdx.y * IMGS;
        u32x4 in[IMGS];
#pragma unroll
        for (int i = 0; i < IMGS; i++) in[i] = load16(dy + (int64_t(min(b0 + i, B - 1)) * (xv + dv) + dv + r) * 8);
#pragma unroll
        for (int i = 0; i < IMGS; i++)
            if (b0 + i < B) store16(dx + (int64_t(b0 + i) * xv + r) * 8, in[i]);
        return;
    }
    const int r0 = blockIdx.y * rows, r1 = min(B, r0 + rows);
    if (r0 >= B) return;                                       // workgroup-uniform (grid.y also covers the copy groups)
    const int cv = threadIdx.x & (CP_CV - 1), rl = threadIdx.x / CP_CV;
    const int v = blockIdx.x * CP_CV + cv;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (v < dv) {
        const u16 *p = dy + int64_t(v) * 8;
        const int64_t img = (xv + dv) * 8;
        int r = r0 + rl;
        for (; r + 3 * CP_RL < r1; r += 4 * CP_RL) {          // four independent loads, added in image order
            u32x4 a[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = load16(p + int64_t(r + i * CP_RL) * img);
#pragma unroll
            for (int i = 0; i < 4; i++) add_vec(s, a[i]);
        }
        for (; r < r1; r += CP_RL) add_vec(s, load16(p + int64_t(r) * img));
    }
#pragma unroll
    for (int j = 0; j < 8; j++) red[rl][cv * 8 + j] = s[j];
    __syncthreads();                                           // every thread of a dcls workgroup arrives: no exit above
    const int c = blockIdx.x * (CP_CV * 8) + threadIdx.x;
    if (threadIdx.x < CP_CV * 8 && c < dv * 8) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < CP_RL; q++) t += red[q][threadIdx.x];
        if (out_kind == 0) static_cast<float *>(out)[int64_t(blockIdx.y) * dv * 8 + c] = t;
        else if (out_kind == 1) static_cast<float *>(out)[c] = t;
        else static_cast<u16 *>(out)[c] = f2bf(t);
    }
}

// count == 1: y[b, :] = x[b, first, :], the bits.
__global__ __launch_bounds__(TP_THREADS) void token_pool_row_kernel(const u16 *__restrict__ x, u16 *__restrict__ y, int T, int dv,
                                                                   int first) {
    const int v = blockIdx.y * TP_THREADS + threadIdx.x, b = blockIdx.x;
    if (v >= dv) return;                                       // (no barrier in this kernel)
    store16(y + (int64_t(b) * dv + v) * 8, load16(x + ((int64_t(b) * T + first) * dv + v) * 8));
}

template <int CV>
__global__ __launch_bounds__(TP_THREADS) void token_pool_fwd_kernel(const u16 *__restrict__ x, u16 *__restrict__ y, int T, int dv,
                                                                   int first, int count) {
    constexpr int TL = TP_THREADS / CV;
    __shared__ float red[TL][CV * 8];
    const int cv = threadIdx.x & (CV - 1), tl = threadIdx.x / CV;
    const int b = blockIdx.x, v = blockIdx.y * CV + cv;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (v < dv) {                                              // a guarded tail, not an exit: the barrier below is for all
        const u16 *p = x + ((int64_t(b) * T + first) * dv + v) * 8;
        const int64_t row = int64_t(dv) * 8;
        int t = tl;
        for (; t + 3 * TL < count; t += 4 * TL) {             // four independent loads, added in token order
            u32x4 a[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = load16(p + int64_t(t + i * TL) * row);
#pragma unroll
            for (int i = 0; i < 4; i++) add_vec(s, a[i]);
        }
        for (; t < count; t += TL) add_vec(s, load16(p + int64_t(t) * row));
    }
#pragma unroll
    for (int j = 0; j < 8; j++) red[tl][cv * 8 + j] = s[j];
    __syncthreads();
    const int c = blockIdx.y * (CV * 8) + threadIdx.x;
    if (threadIdx.x < CV * 8 && c < dv * 8) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < TL; q++) t += red[q][threadIdx.x];
        y[int64_t(b) * dv * 8 + c] = f2bf(__fdiv_rn(t, float(count)));
    }
}

template <int CV>
__global__ __launch_bounds__(TP_THREADS) void token_pool_bwd_kernel(const u16 *__restrict__ dy, u16 *__restrict__ dx, int T, int dv,
                                                                   int first, int count) {
    constexpr int TL = TP_THREADS / CV;
    const int cv = threadIdx.x & (CV - 1), tl = threadIdx.x / CV;
    const int b = blockIdx.x, v = blockIdx.y * CV + cv;
    if (v >= dv) return;                                       // (no barrier in this kernel)
    u32x4 g = load16(dy + (int64_t(b) * dv + v) * 8);
    if (count != 1) {                                          // count == 1 scatters the row's bits
        const float c = float(count);
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = pack2bf(__fdiv_rn(bf2f(u16(g[k])), c), __fdiv_rn(bf2f(u16(g[k] >> 16)), c));
    }
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u16 *q = dx + (int64_t(b) * T * dv + v) * 8;
    const int64_t row = int64_t(dv) * 8;
    const int last = first + count;                            // <= T
    for (int t = tl; t < T; t += TL) store16(q + int64_t(t) * row, t >= first && t < last ? g : zero);
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

#define BY_IMGS(CALL) \
    switch (p.imgs) { case 1: CALL(1); break; case 2: CALL(2); break; case 4: CALL(4); break; default: CALL(8); break; }
#define BY_CV(CALL) \
    switch (p.cv) { case 8: CALL(8); break; case 16: CALL(16); break; default: CALL(32); break; }

extern "C" int sfcvit_cls_prepend_fwd(const void *x, const void *cls, void *y, int B, int N, int D, void *stream) {
    const ClsPrependPlan p = cls_prepend_plan("cls_prepend_fwd", B, N, D);
    if (int rc = cls_prepend_check_fwd(p, x, cls, y, B, N, D)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(p.fwd_blocks, p.groups);
    const u16 *xs = static_cast<const u16 *>(x), *cs = static_cast<const u16 *>(cls);
    u16 *ys = static_cast<u16 *>(y);
#define CALL(I) hipLaunchKernelGGL(cls_prepend_fwd_kernel<I>, grid, dim3(TP_THREADS), 0, st, xs, cs, ys, B, p.xv, p.dv)
    BY_IMGS(CALL)
#undef CALL
    g_token_pool.set("cls_prepend_fwd_kernel<%d>", p.imgs);
    return check_launch("cls_prepend_fwd");
}

extern "C" int sfcvit_cls_prepend_bwd(const void *dy, void *dx, void *dcls, int grad_bf16, int B, int N, int D, void *workspace,
                                      int64_t workspace_bytes, void *stream) {
    const ClsPrependPlan p = cls_prepend_plan("cls_prepend_bwd", B, N, D);
    if (int rc = cls_prepend_check_bwd(p, dy, dx, dcls, workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int kind = p.splits > 1 ? 0 : grad_bf16 ? 2 : 1;
    const int groups = dx ? p.groups : 0;
    const dim3 grid(p.slabs + (dx ? p.bwd_blocks : 0), groups > p.splits ? groups : p.splits);
    const u16 *ds = static_cast<const u16 *>(dy);
    u16 *xs = static_cast<u16 *>(dx);
    void *out = kind == 0 ? workspace : dcls;
#define CALL(I) hipLaunchKernelGGL(cls_prepend_bwd_kernel<I>, grid, dim3(TP_THREADS), 0, st, ds, xs, out, kind, B, p.rows, p.xv, \
                                   p.dv, p.slabs, groups)
    BY_IMGS(CALL)
#undef CALL
    g_token_pool.set("cls_prepend_bwd_kernel<%d>", p.imgs);
    if (int rc = check_launch("cls_prepend_bwd")) return rc;
    if (kind == 0) return reduce_cols(static_cast<const float *>(workspace), p.splits, D, D, dcls, grad_bf16, stream);
    return SFCVIT_OK;
}

extern "C" int sfcvit_token_pool_fwd(const void *x, void *y, int B, int T, int D, int first, int count, void *stream) {
    const TokenPoolPlan p = token_pool_plan("token_pool_fwd", B, T, D, first, count);
    if (int rc = token_pool_check(p, "token_pool_fwd", x, y)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const u16 *xs = static_cast<const u16 *>(x);
    u16 *ys = static_cast<u16 *>(y);
    if (p.row_copy) {
        hipLaunchKernelGGL(token_pool_row_kernel, dim3(B, p.row_blocks), dim3(TP_THREADS), 0, st, xs, ys, T, p.dv, first);
        g_token_pool.set("token_pool_row_kernel");
        return check_launch("token_pool_fwd");
    }
    const dim3 grid(B, p.slabs);
#define CALL(C) hipLaunchKernelGGL(token_pool_fwd_kernel<C>, grid, dim3(TP_THREADS), 0, st, xs, ys, T, p.dv, first, count)
    BY_CV(CALL)
#undef CALL
    g_token_pool.set("token_pool_fwd_kernel<%d>", p.cv);
    return check_launch("token_pool_fwd");
}

extern "C" int sfcvit_token_pool_bwd(const void *dy, void *dx, int B, int T, int D, int first, int count, void *stream) {
    const TokenPoolPlan p = token_pool_plan("token_pool_bwd", B, T, D, first, count);
    if (int rc = token_pool_check(p, "token_pool_bwd", dy, dx)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(B, p.slabs);
    const u16 *ds = static_cast<const u16 *>(dy);
    u16 *xs = static_cast<u16 *>(dx);
#define CALL(C) hipLaunchKernelGGL(token_pool_bwd_kernel<C>, grid, dim3(TP_THREADS), 0, st, ds, xs, T, p.dv, first, count)
    BY_CV(CALL)
#undef CALL
    g_token_pool.set("token_pool_bwd_kernel<%d>", p.cv);
    return check_launch("token_pool_bwd");
}
