// Positional embedding on a [B, N, D] bf16 activation, D contiguous (include/sfcvit.h, "Positional embedding"): the add
// of the reference's commented-out `x = x + self.pos_embed` (src/models/vit.py:382) and the table's gradient.
//
// Both kernels are memory-bound (one add per 2-byte element) and see the tensors as 16-byte vectors of 8 channels; the
// table is N D / 8 vectors long and image b starts N D / 8 vectors after image b - 1.
//   forward:  a lane owns ONE table vector, loaded once, and adds it to `imgs` consecutive images (up to 8 independent
//             loads in flight); grid (table vectors / 256, image groups).  A short last group re-reads image B - 1 through
//             a clamped index and skips the store.
//   backward: dpos[n, :] = sum_b dy[b, n, :].  A workgroup is 32 lanes across a 256-column slab of the table times 8
//             lanes across images; lane rl adds images rl, rl + 8, ... of the workgroup's range in that order, the eight
//             sums meet in LDS in lane order.  With one range (every workload shape: the table alone gives 588 / 2 304
//             workgroups) the workgroup writes dpos itself, fp32 or bf16: ONE launch and no partial buffer, where
//             sfcvit_colsum on the [B, N D] view writes an [N D] fp32 partial row and launches the column reduction to
//             copy it.  A table too small for that (N D < 512 x 256) under a large batch splits the batch into ranges
//             whose fp32 partial rows the library's fixed-order reduction (reduce_cols: deferrable) adds.
//             No atomics, one writer per element: two runs give the same bits.
// dx is dy itself: no kernel.
#include "common_host.h"
#include "device_common.h"
#include "pos_embed.h"

namespace sfcvit {
namespace {

struct Vec8 { float v[8]; };

__device__ __forceinline__ Vec8 load_vec(const uint16_t *p) {
    const u32x4 q = *reinterpret_cast<const u32x4 *>(p);
    Vec8 r;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        r.v[2 * i] = bf2f(uint16_t(q[i]));
        r.v[2 * i + 1] = bf2f(uint16_t(q[i] >> 16));
    }
    return r;
}

template <int IMGS>
__global__ __launch_bounds__(PE_THREADS) void pos_embed_fwd_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ pos,
                                                                  uint16_t *__restrict__ y, int B, int64_t vecs) {
    const int64_t v = int64_t(blockIdx.x) * PE_THREADS + threadIdx.x;
    if (v >= vecs) return;                                     // (no barrier in this kernel)
    const int b0 = blockIdx.y * IMGS;
    const Vec8 t = load_vec(pos + v * 8);
    u32x4 in[IMGS];
#pragma unroll
    for (int i = 0; i < IMGS; i++) {
        const int b = min(b0 + i, B - 1);
        in[i] = *reinterpret_cast<const u32x4 *>(x + (int64_t(b) * vecs + v) * 8);
    }
#pragma unroll
    for (int i = 0; i < IMGS; i++) {
        u32x4 out;
#pragma unroll
        for (int k = 0; k < 4; k++)
            out[k] = pack2bf(bf2f(uint16_t(in[i][k])) + t.v[2 * k], bf2f(uint16_t(in[i][k] >> 16)) + t.v[2 * k + 1]);
        if (b0 + i < B) *reinterpret_cast<u32x4 *>(y + (int64_t(b0 + i) * vecs + v) * 8) = out;
    }
}

// OUT: 0 = fp32 partial row of this range (part[range][N D]), 1 = dpos fp32, 2 = dpos bf16
template <int OUT>
__global__ __launch_bounds__(PE_THREADS) void pos_embed_bwd_kernel(const uint16_t *__restrict__ dy, void *__restrict__ out, int B,
                                                                  int rows, int64_t vecs) {
    __shared__ float red[PE_RL][PE_CV * 8];
    const int cv = threadIdx.x & (PE_CV - 1), rl = threadIdx.x / PE_CV;
    const int64_t v = int64_t(blockIdx.x) * PE_CV + cv;
    const int r0 = blockIdx.y * rows, r1 = min(B, r0 + rows);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (v < vecs) {
        const uint16_t *p = dy + v * 8;
        int r = r0 + rl;
        for (; r + 3 * PE_RL < r1; r += 4 * PE_RL) {          // four independent loads, added in image order
            Vec8 a[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = load_vec(p + int64_t(r + i * PE_RL) * vecs * 8);
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 8; j++) s[j] += a[i].v[j];
        }
        for (; r < r1; r += PE_RL) {
            const Vec8 a = load_vec(p + int64_t(r) * vecs * 8);
#pragma unroll
            for (int j = 0; j < 8; j++) s[j] += a.v[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) red[rl][cv * 8 + j] = s[j];
    __syncthreads();                                           // every thread of the workgroup arrives: no exit above
    const int64_t c = int64_t(blockIdx.x) * (PE_CV * 8) + threadIdx.x;
    if (c < vecs * 8) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < PE_RL; q++) t += red[q][threadIdx.x];
        if constexpr (OUT == 0) static_cast<float *>(out)[int64_t(blockIdx.y) * vecs * 8 + c] = t;
        else if constexpr (OUT == 1) static_cast<float *>(out)[c] = t;
        else static_cast<uint16_t *>(out)[c] = f2bf(t);
    }
}

using u16 = uint16_t;

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_pos_embed_fwd(const void *x, const void *pos, void *y, int B, int N, int D, void *stream) {
    const PosEmbedPlan p = pos_embed_plan("pos_embed_fwd", B, N, D);
    if (int rc = pos_embed_check_fwd(p, x, pos, y)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(p.fwd_blocks, p.fwd_groups);
    const u16 *xs = static_cast<const u16 *>(x), *ps = static_cast<const u16 *>(pos);
    u16 *ys = static_cast<u16 *>(y);
#define CALL(I) hipLaunchKernelGGL(pos_embed_fwd_kernel<I>, grid, dim3(PE_THREADS), 0, st, xs, ps, ys, B, p.vecs)
    switch (p.imgs) {
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break;
    }
#undef CALL
    g_pos_embed.set("pos_embed_fwd_kernel<%d>", p.imgs);
    return check_launch("pos_embed_fwd");
}

extern "C" int sfcvit_pos_embed_bwd(const void *dy, void *dpos, int grad_bf16, int B, int N, int D, void *workspace,
                                    int64_t workspace_bytes, void *stream) {
    const PosEmbedPlan p = pos_embed_plan("pos_embed_bwd", B, N, D);
    if (int rc = pos_embed_check_bwd(p, dy, dpos, workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(p.slabs, p.splits);
    const u16 *ds = static_cast<const u16 *>(dy);
    const int out = p.splits > 1 ? 0 : grad_bf16 ? 2 : 1;
    if (out == 0) hipLaunchKernelGGL(pos_embed_bwd_kernel<0>, grid, dim3(PE_THREADS), 0, st, ds, workspace, B, p.rows, p.vecs);
    else if (out == 1) hipLaunchKernelGGL(pos_embed_bwd_kernel<1>, grid, dim3(PE_THREADS), 0, st, ds, dpos, B, p.rows, p.vecs);
    else hipLaunchKernelGGL(pos_embed_bwd_kernel<2>, grid, dim3(PE_THREADS), 0, st, ds, dpos, B, p.rows, p.vecs);
    g_pos_embed.set("pos_embed_bwd_kernel<%d>", out);
    if (int rc = check_launch("pos_embed_bwd")) return rc;
    if (out == 0) {
        const int64_t nd = p.vecs * 8;                         // splits > 1 only where N D < PE_MIN_WGS x 256: fits int
        return reduce_cols(static_cast<const float *>(workspace), p.splits, int(nd), int(nd), dpos, grad_bf16, stream);
    }
    return SFCVIT_OK;
}
