// What the device code of the row-wise family shares (layernorm.hip, optim.hip, rowwise.hip): the bf16 <-> fp32 vector converters and
// the fixed-order sum of per-block partials.  THREADS / WAVES are each file's own, tied to ROW_THREADS (rowwise.h).
#pragma once
#include "device_common.h"
#include "rowwise.h"

namespace sfcvit {
namespace {

__device__ __forceinline__ void unpack8(const u32x4 &v, float *f) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        f[2 * i] = bf2f(uint16_t(v[i]));
        f[2 * i + 1] = bf2f(uint16_t(v[i] >> 16));
    }
}
__device__ __forceinline__ u32x4 pack8(const float *f) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = pack2bf(f[2 * i], f[2 * i + 1]);
    return v;
}

// Sum of per-block partials, shared by ln_bwd_reduce and reduce_batched_kernel: a 1024-thread block owns 16 columns;
// its 64 thread rows each add every 64th partial row (<= 8 independent loads in flight per thread for 512 partials,
// where the 16-row form these kernels had serialised 32), then 4 thread rows add 16 sub-sums each and one adds those
// 4.  Fixed summation order, no float atomics: bit-reproducible.  The value is returned in thread row 0.
__device__ __forceinline__ void store_grad(void *p, int i, float v, int as_bf16) {
    if (as_bf16) static_cast<uint16_t *>(p)[i] = f2bf(v);
    else static_cast<float *>(p)[i] = v;
}

constexpr int RED_THREADS = 1024;

__device__ __forceinline__ float reduce_partials16(const float *__restrict__ part, int nparts, int ld, int c, bool ok) {
    __shared__ float red[64][17];
    __shared__ float red2[4][16];
    const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
    float s = 0.f;
    if (ok) {
        int b = grp;
        for (; b + 192 < nparts; b += 256) {
            const float v0 = part[size_t(b) * ld + c], v1 = part[size_t(b + 64) * ld + c];
            const float v2 = part[size_t(b + 128) * ld + c], v3 = part[size_t(b + 192) * ld + c];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; b < nparts; b += 64) s += part[size_t(b) * ld + c];
    }
    red[grp][cl] = s;
    __syncthreads();
    if (grp < 4) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; k++) t += red[grp * 16 + k][cl];
        red2[grp][cl] = t;
    }
    __syncthreads();
    return grp == 0 ? (red2[0][cl] + red2[1][cl]) + (red2[2][cl] + red2[3][cl]) : 0.f;
}

}  // namespace
}  // namespace sfcvit
