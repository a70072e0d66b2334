// LayerNorm for gfx950: forward (one or two rows per wave, and the stochastic-depth residual form), backward (16-byte-vector
// and column-chunk forms, each with a stochastic-depth twin) and the reduction of its partials.  HBM-bound row-wise kernels: one
// 64-lane wave owns one row, every global access is a 16-byte vector (8 bf16 or 4 fp32), reductions are wave butterflies.
// The launchers run what the plans of rowwise.h / drop_path.h say.
#include "common_host.h"
#include "drop_path.h"
#include "rowwise_device.h"

namespace sfcvit {
namespace {

constexpr int THREADS = ROW_THREADS;        // the plans (rowwise.h) size the grids for this
constexpr int WAVES = ROW_WAVES;

// ---------------------------------------------------------------------------
// LayerNorm forward.  VPL = 16-byte vectors per lane (D <= VPL * 512).
// ---------------------------------------------------------------------------
template <int VPL>
__global__ __launch_bounds__(THREADS) void ln_fwd_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ gamma,
                                                         const uint16_t *__restrict__ beta, uint16_t *__restrict__ y,
                                                         float *__restrict__ mean, float *__restrict__ rstd, int M,
                                                         int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nvec = D >> 3;
    float v[VPL][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) {
            unpack8(*reinterpret_cast<const u32x4 *>(x + size_t(row) * D + c * 8), v[i]);
#pragma unroll
            for (int j = 0; j < 8; j++) s += v[i][j];
        }
    }
    const float mu = wave_sum(s) / float(D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++)
        if (lane + 64 * i < nvec) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float d = v[i][j] - mu;
                q += d * d;
            }
        }
    const float rs = rsqrtf(wave_sum(q) / float(D) + eps);
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) {
            float g[8], b[8], o[8];
            unpack8(*reinterpret_cast<const u32x4 *>(gamma + c * 8), g);
            unpack8(*reinterpret_cast<const u32x4 *>(beta + c * 8), b);
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = (v[i][j] - mu) * rs * g[j] + b[j];
            *reinterpret_cast<u32x4 *>(y + size_t(row) * D + c * 8) = pack8(o);
        }
    }
}

// Two rows per wave (D = 768: 2 x 96 vectors = 3 per lane exactly, where one row leaves a third of the lanes idle on the second
// load; D = 1 024: 4 per lane): twice the bytes in flight per wave -- at one 1.5-KB row per wave a CU holds 48 KB of loads, about
// what 6 TB/s needs at this latency, and the kernel ran at 4.6 -- and the two rows' reductions overlap.  In the step (rocprofv3,
// same box, alternating): 33.4 -> 30.8-31.2 us per launch; alone both forms take 26.9 us (inputs warm in the memory-side cache).
// Nontemporal loads of x on top: 31.4-31.5 us, not kept.
template <int VPL>
__global__ __launch_bounds__(THREADS) void ln_fwd2_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ gamma,
                                                          const uint16_t *__restrict__ beta, uint16_t *__restrict__ y,
                                                          float *__restrict__ mean, float *__restrict__ rstd, int M,
                                                          int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row0 = 2 * (blockIdx.x * WAVES + (threadIdx.x >> 6));
    if (row0 >= M) return;
    const int nvec = D >> 3;                                   // 2 * nvec <= 64 * VPL (host)
    const bool two = row0 + 1 < M;
    float v[VPL][8];
    int col[VPL];                                              // vector column, or -1; bit 30: second row
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i, r = c >= nvec ? 1 : 0, cc = c - r * nvec;
        col[i] = (c < 2 * nvec && (r == 0 || two)) ? (cc | (r << 30)) : -1;
        if (col[i] >= 0) {
            unpack8(*reinterpret_cast<const u32x4 *>(x + size_t(row0 + r) * D + cc * 8), v[i]);
            float t = 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++) t += v[i][j];
            if (r) s1 += t; else s0 += t;
        }
    }
    const float mu0 = wave_sum(s0) / float(D), mu1 = wave_sum(s1) / float(D);
    float q0 = 0.f, q1 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++)
        if (col[i] >= 0) {
            const bool r = col[i] >> 30;
            const float mu = r ? mu1 : mu0;
            float t = 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float d = v[i][j] - mu;
                t += d * d;
            }
            if (r) q1 += t; else q0 += t;
        }
    const float rs0 = rsqrtf(wave_sum(q0) / float(D) + eps), rs1 = rsqrtf(wave_sum(q1) / float(D) + eps);
    if (lane == 0) {
        mean[row0] = mu0;
        rstd[row0] = rs0;
        if (two) {
            mean[row0 + 1] = mu1;
            rstd[row0 + 1] = rs1;
        }
    }
#pragma unroll
    for (int i = 0; i < VPL; i++)
        if (col[i] >= 0) {
            const int r = col[i] >> 30, cc = col[i] & 0xFFFFFF;
            const float mu = r ? mu1 : mu0, rs = r ? rs1 : rs0;
            float g[8], b[8], o[8];
            unpack8(*reinterpret_cast<const u32x4 *>(gamma + cc * 8), g);
            unpack8(*reinterpret_cast<const u32x4 *>(beta + cc * 8), b);
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = (v[i][j] - mu) * rs * g[j] + b[j];
            *reinterpret_cast<u32x4 *>(y + size_t(row0 + r) * D + cc * 8) = pack8(o);
        }
}

// Stochastic depth on a residual site (sfcvit_add_layernorm_path_fwd): s = bf16(x + c[b] * branch), y = LayerNorm(s), one wave
// per row.  c[b] = keep(b) / (1 - rate) with keep(b) element (b, 0) of the dropout mask of `seed`, b = row / N.  A dropped
// image's rows never read the branch and store the bits of x; LayerNorm's statistics and y come from the ROUNDED s, which is
// what backward recomputes x_hat from.
template <int VPL>
__global__ __launch_bounds__(THREADS) void add_ln_path_kernel(const uint16_t *__restrict__ branch, const uint16_t *__restrict__ x,
                                                              const uint16_t *__restrict__ gamma, const uint16_t *__restrict__ beta,
                                                              uint16_t *__restrict__ sum, uint16_t *__restrict__ y,
                                                              float *__restrict__ mean, float *__restrict__ rstd, int M, int N,
                                                              int D, float eps, float rate, uint32_t seed_arg,
                                                              const uint32_t *__restrict__ seed_off) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (row >= M) return;
    const bool keep = drop_keep(drop_row_key(eff_seed(seed_arg, seed_off), uint64_t(row / N)), 0u, drop_thresh(rate));
    const float sc = 1.f / (1.f - rate);
    const int nvec = D >> 3;
    u32x4 xr[VPL], ar[VPL];
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) {
            xr[i] = *reinterpret_cast<const u32x4 *>(x + size_t(row) * D + c * 8);
            if (keep) ar[i] = *reinterpret_cast<const u32x4 *>(branch + size_t(row) * D + c * 8);
        }
    }
    float v[VPL][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) {
            unpack8(xr[i], v[i]);
            if (keep) {
                float a[8];
                unpack8(ar[i], a);
#pragma unroll
                for (int j = 0; j < 8; j++) v[i][j] += sc * a[j];
                xr[i] = pack8(v[i]);
                unpack8(xr[i], v[i]);                           // the rounded sum
            }
            *reinterpret_cast<u32x4 *>(sum + size_t(row) * D + c * 8) = xr[i];
#pragma unroll
            for (int j = 0; j < 8; j++) s += v[i][j];
        }
    }
    const float mu = wave_sum(s) / float(D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++)
        if (lane + 64 * i < nvec) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float d = v[i][j] - mu;
                q += d * d;
            }
        }
    const float rs = rsqrtf(wave_sum(q) / float(D) + eps);
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) {
            float g[8], b[8], o[8];
            unpack8(*reinterpret_cast<const u32x4 *>(gamma + c * 8), g);
            unpack8(*reinterpret_cast<const u32x4 *>(beta + c * 8), b);
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = (v[i][j] - mu) * rs * g[j] + b[j];
            *reinterpret_cast<u32x4 *>(y + size_t(row) * D + c * 8) = pack8(o);
        }
    }
}

// ---------------------------------------------------------------------------
// LayerNorm backward.  Each wave walks rows with a grid stride, keeps its lanes'
// columns of dgamma / dbeta in registers, and the block writes one partial row
// [2][D] to the workspace; ln_bwd_reduce sums the partials.
// ---------------------------------------------------------------------------
template <int VPL, bool ADD>
__global__ __launch_bounds__(THREADS) void ln_bwd_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                         const float *__restrict__ mean, const float *__restrict__ rstd,
                                                         const uint16_t *__restrict__ gamma,
                                                         const uint16_t *__restrict__ dx_add, uint16_t *__restrict__ dx,
                                                         uint16_t *__restrict__ dx_drop, float drop_p, uint32_t drop_seed_arg,
                                                         const uint32_t *__restrict__ seed_off,
                                                         float *__restrict__ partial, int M, int D) {
    const uint32_t drop_seed = eff_seed(drop_seed_arg, seed_off);
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [WAVES][3][D] fp32
    const uint32_t drop_th = drop_thresh(drop_p);
    const float drop_sc = 1.f / (1.f - drop_p);
    float *red = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = D >> 3;
    float g[VPL][8], dg[VPL][8], db[VPL][8], dc[VPL][8];   // dc: column sums of the outgoing gradient
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) unpack8(*reinterpret_cast<const u32x4 *>(gamma + c * 8), g[i]);
#pragma unroll
        for (int j = 0; j < 8; j++) dg[i][j] = db[i][j] = dc[i][j] = 0.f;
    }
    // Rows are software-pipelined: the loads of this wave's next row are issued before the current row is reduced
    // (a row is load -> two wave reductions -> store, and only 8 waves per CU are resident: without the prefetch
    // the kernel sat at 2.7-3.3 TB/s).  Two rows ahead measured slower (54.6 vs 51.3 us at M 50 176, D 768).
    const int stride = gridDim.x * WAVES;
    u32x4 xr[VPL], dr[VPL], ar[VPL], xn[VPL], dn[VPL], an[VPL];
    float mu = 0.f, rs = 0.f, mun = 0.f, rsn = 0.f;
    auto load_row = [&](int row, u32x4 (&xq)[VPL], u32x4 (&dq)[VPL], u32x4 (&aq)[VPL], float &m, float &r) __attribute__((always_inline)) {
        m = mean[row];
        r = rstd[row];
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            const int c = lane + 64 * i;
            if (c < nvec) {
                xq[i] = *reinterpret_cast<const u32x4 *>(x + size_t(row) * D + c * 8);
                dq[i] = *reinterpret_cast<const u32x4 *>(dy + size_t(row) * D + c * 8);
                if (ADD) aq[i] = *reinterpret_cast<const u32x4 *>(dx_add + size_t(row) * D + c * 8);
            }
        }
    };
    int row = blockIdx.x * WAVES + wave;
    if (row < M) load_row(row, xr, dr, ar, mu, rs);
    for (; row < M; row += stride) {
        const bool more = row + stride < M;
        if (more) load_row(row + stride, xn, dn, an, mun, rsn);
        float xh[VPL][8], gy[VPL][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            const int c = lane + 64 * i;
            if (c < nvec) {
                float xv[8], dv[8];
                unpack8(xr[i], xv);
                unpack8(dr[i], dv);
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    xh[i][j] = (xv[j] - mu) * rs;
                    gy[i][j] = dv[j] * g[i][j];
                    s1 += gy[i][j];
                    s2 += gy[i][j] * xh[i][j];
                    dg[i][j] += dv[j] * xh[i][j];
                    db[i][j] += dv[j];
                }
            }
        }
        const float c1 = wave_sum(s1) / float(D), c2 = wave_sum(s2) / float(D);
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            const int c = lane + 64 * i;
            if (c < nvec) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; j++) o[j] = rs * (gy[i][j] - c1 - xh[i][j] * c2);
                if (ADD) {
                    float a[8];
                    unpack8(ar[i], a);
#pragma unroll
                    for (int j = 0; j < 8; j++) o[j] += a[j];
                }
                *reinterpret_cast<u32x4 *>(dx + size_t(row) * D + c * 8) = pack8(o);
                if (!dx_drop) {
#pragma unroll
                    for (int j = 0; j < 8; j++) dc[i][j] += o[j];
                }
                if (dx_drop) {
                    const uint32_t rk = drop_row_key(drop_seed, uint64_t(row));
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        bool k0, k1;
                        drop_keep2(rk, uint32_t(c * 4 + q), drop_th, k0, k1);
                        o[2 * q] = k0 ? o[2 * q] * drop_sc : 0.f;
                        o[2 * q + 1] = k1 ? o[2 * q + 1] * drop_sc : 0.f;
                    }
                    *reinterpret_cast<u32x4 *>(dx_drop + size_t(row) * D + c * 8) = pack8(o);
#pragma unroll
                    for (int j = 0; j < 8; j++) dc[i][j] += o[j];
                }
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < VPL; i++) { xr[i] = xn[i]; dr[i] = dn[i]; ar[i] = an[i]; }
            mu = mun;
            rs = rsn;
        }
    }
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                red[(wave * 3 + 0) * D + c * 8 + j] = dg[i][j];
                red[(wave * 3 + 1) * D + c * 8 + j] = db[i][j];
                red[(wave * 3 + 2) * D + c * 8 + j] = dc[i][j];
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 3 * D; c += THREADS) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += red[w * 3 * D + c];
        partial[size_t(blockIdx.x) * 3 * D + c] = s;
    }
}

// ln_bwd_kernel with stochastic depth (sfcvit_layernorm_bwd_path): the multiplier of the outgoing gradient dx_drop is per row -- image
// b = row / rows_per_image kept ? drop_sc / (1 - path_rate) : 0, the flag regenerated as element (b, 0) of the mask of path_seed --
// and dx_drop is always written; dcol sums the ROUNDED dx_drop; dx, dgamma and dbeta are what they are without it.  Kernels of their own: with the body shared
// (a template parameter, `if constexpr`) hipcc compiled ln_bwd_kernel / ln_bwd_cols_kernel to other instructions than it does alone.
template <int VPL, bool ADD>
__global__ __launch_bounds__(THREADS) void ln_bwd_path_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                              const float *__restrict__ mean, const float *__restrict__ rstd,
                                                              const uint16_t *__restrict__ gamma,
                                                              const uint16_t *__restrict__ dx_add, uint16_t *__restrict__ dx,
                                                              uint16_t *__restrict__ dx_drop, float drop_p, uint32_t drop_seed_arg,
                                                              const uint32_t *__restrict__ seed_off,
                                                              float *__restrict__ partial, int M, int D, int rows_per_image,
                                                              float path_rate, uint32_t path_seed_arg) {
    const uint32_t drop_seed = eff_seed(drop_seed_arg, seed_off);
    const uint32_t path_seed = eff_seed(path_seed_arg, seed_off), path_th = drop_thresh(path_rate);
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [WAVES][3][D] fp32
    const uint32_t drop_th = drop_thresh(drop_p);
    const float drop_sc = 1.f / (1.f - drop_p), path_mul = drop_sc / (1.f - path_rate);
    float *red = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = D >> 3;
    float g[VPL][8], dg[VPL][8], db[VPL][8], dc[VPL][8];   // dc: column sums of the outgoing gradient
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) unpack8(*reinterpret_cast<const u32x4 *>(gamma + c * 8), g[i]);
#pragma unroll
        for (int j = 0; j < 8; j++) dg[i][j] = db[i][j] = dc[i][j] = 0.f;
    }
    // Rows are software-pipelined: the loads of this wave's next row are issued before the current row is reduced
    // (a row is load -> two wave reductions -> store, and only 8 waves per CU are resident: without the prefetch
    // the kernel sat at 2.7-3.3 TB/s).  Two rows ahead measured slower (54.6 vs 51.3 us at M 50 176, D 768).
    const int stride = gridDim.x * WAVES;
    u32x4 xr[VPL], dr[VPL], ar[VPL], xn[VPL], dn[VPL], an[VPL];
    float mu = 0.f, rs = 0.f, mun = 0.f, rsn = 0.f;
    auto load_row = [&](int row, u32x4 (&xq)[VPL], u32x4 (&dq)[VPL], u32x4 (&aq)[VPL], float &m, float &r) __attribute__((always_inline)) {
        m = mean[row];
        r = rstd[row];
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            const int c = lane + 64 * i;
            if (c < nvec) {
                xq[i] = *reinterpret_cast<const u32x4 *>(x + size_t(row) * D + c * 8);
                dq[i] = *reinterpret_cast<const u32x4 *>(dy + size_t(row) * D + c * 8);
                if (ADD) aq[i] = *reinterpret_cast<const u32x4 *>(dx_add + size_t(row) * D + c * 8);
            }
        }
    };
    int row = blockIdx.x * WAVES + wave;
    if (row < M) load_row(row, xr, dr, ar, mu, rs);
    for (; row < M; row += stride) {
        const bool more = row + stride < M;
        if (more) load_row(row + stride, xn, dn, an, mun, rsn);
        float xh[VPL][8], gy[VPL][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            const int c = lane + 64 * i;
            if (c < nvec) {
                float xv[8], dv[8];
                unpack8(xr[i], xv);
                unpack8(dr[i], dv);
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    xh[i][j] = (xv[j] - mu) * rs;
                    gy[i][j] = dv[j] * g[i][j];
                    s1 += gy[i][j];
                    s2 += gy[i][j] * xh[i][j];
                    dg[i][j] += dv[j] * xh[i][j];
                    db[i][j] += dv[j];
                }
            }
        }
        const float c1 = wave_sum(s1) / float(D), c2 = wave_sum(s2) / float(D);
        const bool path_keep = drop_keep(drop_row_key(path_seed, uint64_t(row / rows_per_image)), 0u, path_th);
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            const int c = lane + 64 * i;
            if (c < nvec) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; j++) o[j] = rs * (gy[i][j] - c1 - xh[i][j] * c2);
                if (ADD) {
                    float a[8];
                    unpack8(ar[i], a);
#pragma unroll
                    for (int j = 0; j < 8; j++) o[j] += a[j];
                }
                *reinterpret_cast<u32x4 *>(dx + size_t(row) * D + c * 8) = pack8(o);
                {                                               // (dx_drop is never NULL here: the plan refuses that)
                    const uint32_t rk = drop_row_key(drop_seed, uint64_t(row));
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        bool k0, k1;
                        drop_keep2(rk, uint32_t(c * 4 + q), drop_th, k0, k1);
                        o[2 * q] = (k0 && path_keep) ? o[2 * q] * path_mul : 0.f;
                        o[2 * q + 1] = (k1 && path_keep) ? o[2 * q + 1] * path_mul : 0.f;
                    }
                    const u32x4 stored = pack8(o);
                    *reinterpret_cast<u32x4 *>(dx_drop + size_t(row) * D + c * 8) = stored;
                    unpack8(stored, o);                          // dcol sums what dx_drop holds: the rounded values
#pragma unroll
                    for (int j = 0; j < 8; j++) dc[i][j] += o[j];
                }
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < VPL; i++) { xr[i] = xn[i]; dr[i] = dn[i]; ar[i] = an[i]; }
            mu = mun;
            rs = rsn;
        }
    }
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                red[(wave * 3 + 0) * D + c * 8 + j] = dg[i][j];
                red[(wave * 3 + 1) * D + c * 8 + j] = db[i][j];
                red[(wave * 3 + 2) * D + c * 8 + j] = dc[i][j];
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 3 * D; c += THREADS) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += red[w * 3 * D + c];
        partial[size_t(blockIdx.x) * 3 * D + c] = s;
    }
}

// The same for D = 256 CH with CH odd (ViT-B: 768 = 3 x 256), where the 16-byte-vector form above leaves a quarter of the
// lanes idle in its second vector.  Measured (tools/bench_rowwise.py, M 50 176): that kernel issues ~450 VALU instructions
// per row and wave -- 49 rows per SIMD x 450 x 4 clocks = 46 us of its 51-66 us: it is VALU-bound, not HBM-bound (two rows
// of prefetch, or three waves per SIMD from a register diet, made it slower).  Here a lane owns CH chunks of 4 columns
// (8-byte loads, every lane busy) and all arithmetic is written on float pairs (v_pk_* instructions, no shuffles).
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ f32x2 unpack2(uint32_t w) { return f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)}; }

template <int CH, bool ADD>
__global__ __launch_bounds__(THREADS) void ln_bwd_cols_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                              const float *__restrict__ mean, const float *__restrict__ rstd,
                                                              const uint16_t *__restrict__ gamma,
                                                              const uint16_t *__restrict__ dx_add, uint16_t *__restrict__ dx,
                                                              uint16_t *__restrict__ dx_drop, float drop_p, uint32_t drop_seed_arg,
                                                              const uint32_t *__restrict__ seed_off,
                                                              float *__restrict__ partial, int M) {
    constexpr int D = 256 * CH;
    const uint32_t drop_seed = eff_seed(drop_seed_arg, seed_off);
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [WAVES][3][D] fp32
    const uint32_t drop_th = drop_thresh(drop_p);
    const float drop_sc = 1.f / (1.f - drop_p);
    float *red = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // lane's columns: 256 k + 4 lane + 2 h + {0, 1}, k < CH, h < 2
    f32x2 g[CH][2], dg[CH][2], db[CH][2], dc[CH][2];
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const u32x2 w = *reinterpret_cast<const u32x2 *>(gamma + 256 * k + 4 * lane);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            g[k][h] = unpack2(w[h]);
            dg[k][h] = db[k][h] = dc[k][h] = f32x2{0.f, 0.f};
        }
    }
    const int stride = gridDim.x * WAVES;
    u32x2 xr[CH], dr[CH], ar[CH], xn[CH], dn[CH], an[CH];
    float mu = 0.f, rs = 0.f, mun = 0.f, rsn = 0.f;
    auto load_row = [&](int row, u32x2 (&xq)[CH], u32x2 (&dq)[CH], u32x2 (&aq)[CH], float &m, float &r) __attribute__((always_inline)) {
        m = mean[row];
        r = rstd[row];
        const size_t o = size_t(row) * D + 4 * lane;
#pragma unroll
        for (int k = 0; k < CH; k++) {
            xq[k] = *reinterpret_cast<const u32x2 *>(x + o + 256 * k);
            dq[k] = *reinterpret_cast<const u32x2 *>(dy + o + 256 * k);
            if (ADD) aq[k] = *reinterpret_cast<const u32x2 *>(dx_add + o + 256 * k);
        }
    };
    int row = blockIdx.x * WAVES + wave;
    if (row < M) load_row(row, xr, dr, ar, mu, rs);
    for (; row < M; row += stride) {
        const bool more = row + stride < M;
        if (more) load_row(row + stride, xn, dn, an, mun, rsn);   // the next row's loads fly while this one is reduced
        f32x2 xh[CH][2], gy[CH][2];
        f32x2 s1 = {0.f, 0.f}, s2 = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < CH; k++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const f32x2 xv = unpack2(xr[k][h]), dv = unpack2(dr[k][h]);
                xh[k][h] = (xv - mu) * rs;
                gy[k][h] = dv * g[k][h];
                s1 += gy[k][h];
                s2 += gy[k][h] * xh[k][h];
                dg[k][h] += dv * xh[k][h];
                db[k][h] += dv;
            }
        }
        const float c1 = wave_sum(s1[0] + s1[1]) / float(D), c2 = wave_sum(s2[0] + s2[1]) / float(D);
        const size_t o = size_t(row) * D + 4 * lane;
        const uint32_t rk = drop_row_key(drop_seed, uint64_t(row));
#pragma unroll
        for (int k = 0; k < CH; k++) {
            f32x2 ov[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                ov[h] = rs * (gy[k][h] - c1 - xh[k][h] * c2);
                if (ADD) ov[h] += unpack2(ar[k][h]);
            }
            *reinterpret_cast<u32x2 *>(dx + o + 256 * k) = u32x2{pack2bf(ov[0][0], ov[0][1]), pack2bf(ov[1][0], ov[1][1])};
            if (dx_drop) {
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    bool k0, k1;
                    drop_keep2(rk, uint32_t(128 * k + 2 * lane + h), drop_th, k0, k1);      // pair = column / 2
                    ov[h][0] = k0 ? ov[h][0] * drop_sc : 0.f;
                    ov[h][1] = k1 ? ov[h][1] * drop_sc : 0.f;
                }
                *reinterpret_cast<u32x2 *>(dx_drop + o + 256 * k) = u32x2{pack2bf(ov[0][0], ov[0][1]), pack2bf(ov[1][0], ov[1][1])};
            }
            dc[k][0] += ov[0];
            dc[k][1] += ov[1];
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < CH; k++) { xr[k] = xn[k]; dr[k] = dn[k]; ar[k] = an[k]; }
            mu = mun;
            rs = rsn;
        }
    }
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const int c = 256 * k + 4 * lane;
        *reinterpret_cast<f32x4 *>(red + (wave * 3 + 0) * D + c) = f32x4{dg[k][0][0], dg[k][0][1], dg[k][1][0], dg[k][1][1]};
        *reinterpret_cast<f32x4 *>(red + (wave * 3 + 1) * D + c) = f32x4{db[k][0][0], db[k][0][1], db[k][1][0], db[k][1][1]};
        *reinterpret_cast<f32x4 *>(red + (wave * 3 + 2) * D + c) = f32x4{dc[k][0][0], dc[k][0][1], dc[k][1][0], dc[k][1][1]};
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 3 * D; c += THREADS) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += red[w * 3 * D + c];
        partial[size_t(blockIdx.x) * 3 * D + c] = s;
    }
}

// ln_bwd_cols_kernel with stochastic depth, as ln_bwd_path_kernel is to ln_bwd_kernel.
template <int CH, bool ADD>
__global__ __launch_bounds__(THREADS) void ln_bwd_cols_path_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                                   const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                   const uint16_t *__restrict__ gamma,
                                                                   const uint16_t *__restrict__ dx_add, uint16_t *__restrict__ dx,
                                                                   uint16_t *__restrict__ dx_drop, float drop_p, uint32_t drop_seed_arg,
                                                                   const uint32_t *__restrict__ seed_off,
                                                                   float *__restrict__ partial, int M, int rows_per_image,
                                                                   float path_rate, uint32_t path_seed_arg) {
    constexpr int D = 256 * CH;
    const uint32_t drop_seed = eff_seed(drop_seed_arg, seed_off);
    const uint32_t path_seed = eff_seed(path_seed_arg, seed_off), path_th = drop_thresh(path_rate);
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [WAVES][3][D] fp32
    const uint32_t drop_th = drop_thresh(drop_p);
    const float drop_sc = 1.f / (1.f - drop_p), path_mul = drop_sc / (1.f - path_rate);
    float *red = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // lane's columns: 256 k + 4 lane + 2 h + {0, 1}, k < CH, h < 2
    f32x2 g[CH][2], dg[CH][2], db[CH][2], dc[CH][2];
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const u32x2 w = *reinterpret_cast<const u32x2 *>(gamma + 256 * k + 4 * lane);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            g[k][h] = unpack2(w[h]);
            dg[k][h] = db[k][h] = dc[k][h] = f32x2{0.f, 0.f};
        }
    }
    const int stride = gridDim.x * WAVES;
    u32x2 xr[CH], dr[CH], ar[CH], xn[CH], dn[CH], an[CH];
    float mu = 0.f, rs = 0.f, mun = 0.f, rsn = 0.f;
    auto load_row = [&](int row, u32x2 (&xq)[CH], u32x2 (&dq)[CH], u32x2 (&aq)[CH], float &m, float &r) __attribute__((always_inline)) {
        m = mean[row];
        r = rstd[row];
        const size_t o = size_t(row) * D + 4 * lane;
#pragma unroll
        for (int k = 0; k < CH; k++) {
            xq[k] = *reinterpret_cast<const u32x2 *>(x + o + 256 * k);
            dq[k] = *reinterpret_cast<const u32x2 *>(dy + o + 256 * k);
            if (ADD) aq[k] = *reinterpret_cast<const u32x2 *>(dx_add + o + 256 * k);
        }
    };
    int row = blockIdx.x * WAVES + wave;
    if (row < M) load_row(row, xr, dr, ar, mu, rs);
    for (; row < M; row += stride) {
        const bool more = row + stride < M;
        if (more) load_row(row + stride, xn, dn, an, mun, rsn);   // the next row's loads fly while this one is reduced
        f32x2 xh[CH][2], gy[CH][2];
        f32x2 s1 = {0.f, 0.f}, s2 = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < CH; k++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const f32x2 xv = unpack2(xr[k][h]), dv = unpack2(dr[k][h]);
                xh[k][h] = (xv - mu) * rs;
                gy[k][h] = dv * g[k][h];
                s1 += gy[k][h];
                s2 += gy[k][h] * xh[k][h];
                dg[k][h] += dv * xh[k][h];
                db[k][h] += dv;
            }
        }
        const float c1 = wave_sum(s1[0] + s1[1]) / float(D), c2 = wave_sum(s2[0] + s2[1]) / float(D);
        const size_t o = size_t(row) * D + 4 * lane;
        const uint32_t rk = drop_row_key(drop_seed, uint64_t(row));
        const bool path_keep = drop_keep(drop_row_key(path_seed, uint64_t(row / rows_per_image)), 0u, path_th);
#pragma unroll
        for (int k = 0; k < CH; k++) {
            f32x2 ov[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                ov[h] = rs * (gy[k][h] - c1 - xh[k][h] * c2);
                if (ADD) ov[h] += unpack2(ar[k][h]);
            }
            *reinterpret_cast<u32x2 *>(dx + o + 256 * k) = u32x2{pack2bf(ov[0][0], ov[0][1]), pack2bf(ov[1][0], ov[1][1])};
            if (dx_drop) {
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    bool k0, k1;
                    drop_keep2(rk, uint32_t(128 * k + 2 * lane + h), drop_th, k0, k1);      // pair = column / 2
                    ov[h][0] = (k0 && path_keep) ? ov[h][0] * path_mul : 0.f;
                    ov[h][1] = (k1 && path_keep) ? ov[h][1] * path_mul : 0.f;
                }
                const u32x2 stored = u32x2{pack2bf(ov[0][0], ov[0][1]), pack2bf(ov[1][0], ov[1][1])};
                *reinterpret_cast<u32x2 *>(dx_drop + o + 256 * k) = stored;
                ov[0] = unpack2(stored[0]);                      // dcol sums what dx_drop holds: the rounded values
                ov[1] = unpack2(stored[1]);
            }
            dc[k][0] += ov[0];
            dc[k][1] += ov[1];
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < CH; k++) { xr[k] = xn[k]; dr[k] = dn[k]; ar[k] = an[k]; }
            mu = mun;
            rs = rsn;
        }
    }
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const int c = 256 * k + 4 * lane;
        *reinterpret_cast<f32x4 *>(red + (wave * 3 + 0) * D + c) = f32x4{dg[k][0][0], dg[k][0][1], dg[k][1][0], dg[k][1][1]};
        *reinterpret_cast<f32x4 *>(red + (wave * 3 + 1) * D + c) = f32x4{db[k][0][0], db[k][0][1], db[k][1][0], db[k][1][1]};
        *reinterpret_cast<f32x4 *>(red + (wave * 3 + 2) * D + c) = f32x4{dc[k][0][0], dc[k][0][1], dc[k][1][0], dc[k][1][1]};
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 3 * D; c += THREADS) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += red[w * 3 * D + c];
        partial[size_t(blockIdx.x) * 3 * D + c] = s;
    }
}

// [nblocks][3][D] partials -> dgamma | dbeta | column sums of the outgoing gradient.
__global__ __launch_bounds__(RED_THREADS) void ln_bwd_reduce(const float *__restrict__ partial, void *__restrict__ dgamma,
                                                            void *__restrict__ dbeta, void *__restrict__ dcol, int nblocks,
                                                            int D, int as_bf16) {
    const int c = blockIdx.x * 16 + (threadIdx.x & 15);
    const float t = reduce_partials16(partial, nblocks, 3 * D, c, c < 3 * D);
    if (threadIdx.x < 16 && c < 3 * D) {
        if (c < D) store_grad(dgamma, c, t, as_bf16);
        else if (c < 2 * D) store_grad(dbeta, c - D, t, as_bf16);
        else if (dcol) store_grad(dcol, c - 2 * D, t, as_bf16);
    }
}

// One launch path for sfcvit_layernorm_bwd_drop and sfcvit_layernorm_bwd_path (`path`: N, path_rate and path_seed count): the
// kernel the plan names, then dgamma / dbeta / dcol from its partials.
int launch_ln_bwd(const LnBwdPlan &pl, bool path, const void *dy, const void *x, const float *mean, const float *rstd,
                  const void *gamma, const void *dx_add, void *dx, void *dx_drop, float p, uint32_t seed, const uint32_t *seed_off,
                  void *dgamma, void *dbeta, void *dcol, int grads_bf16, void *ws, int N, float path_rate, uint32_t path_seed,
                  void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(pl.blocks), block(THREADS);
    const int M = pl.M, D = pl.D, nb = pl.blocks;
    const auto *dyp = static_cast<const uint16_t *>(dy);
    const auto *xp = static_cast<const uint16_t *>(x);
    const auto *gp = static_cast<const uint16_t *>(gamma);
    const auto *ap = static_cast<const uint16_t *>(dx_add);
    auto *dxp = static_cast<uint16_t *>(dx);
    auto *ddp = static_cast<uint16_t *>(dx_drop);
    float *part = static_cast<float *>(ws);
    kernel_name(pl, path, g_rowwise.name, sizeof(g_rowwise.name));
#define LN_BWD(KERNEL, INST, ...) do { \
        if (pl.add) hipLaunchKernelGGL((KERNEL<INST, true>), grid, block, pl.lds, s, dyp, xp, mean, rstd, gp, ap, dxp, ddp, p, seed, seed_off, part, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<INST, false>), grid, block, pl.lds, s, dyp, xp, mean, rstd, gp, ap, dxp, ddp, p, seed, seed_off, part, __VA_ARGS__); } while (0)
    if (pl.cols && path) {
        if (pl.inst == 3) LN_BWD(ln_bwd_cols_path_kernel, 3, M, N, path_rate, path_seed);
        else LN_BWD(ln_bwd_cols_path_kernel, 4, M, N, path_rate, path_seed);
    } else if (pl.cols) {
        if (pl.inst == 3) LN_BWD(ln_bwd_cols_kernel, 3, M);
        else LN_BWD(ln_bwd_cols_kernel, 4, M);
    } else if (path) {
        if (pl.inst == 1) LN_BWD(ln_bwd_path_kernel, 1, M, D, N, path_rate, path_seed);
        else if (pl.inst == 2) LN_BWD(ln_bwd_path_kernel, 2, M, D, N, path_rate, path_seed);
        else LN_BWD(ln_bwd_path_kernel, 4, M, D, N, path_rate, path_seed);
    } else {
        if (pl.inst == 1) LN_BWD(ln_bwd_kernel, 1, M, D);
        else if (pl.inst == 2) LN_BWD(ln_bwd_kernel, 2, M, D);
        else LN_BWD(ln_bwd_kernel, 4, M, D);
    }
#undef LN_BWD
    if (int rc = check_launch(path ? "layernorm_bwd_path" : "layernorm_bwd")) return rc;
    if (reduce_deferring()) {            // queued for the batched launch at sfcvit_reduce_flush: partial rows are [3][D]
        reduce_cols(part, nb, 3 * D, D, dgamma, grads_bf16, stream);
        reduce_cols(part + D, nb, 3 * D, D, dbeta, grads_bf16, stream);
        if (dcol) reduce_cols(part + 2 * D, nb, 3 * D, D, dcol, grads_bf16, stream);
        return SFCVIT_OK;
    }
    hipLaunchKernelGGL(ln_bwd_reduce, dim3((3 * D + 15) / 16), dim3(RED_THREADS), 0, s, part, dgamma, dbeta, dcol, nb, D, grads_bf16);
    return check_launch("layernorm_bwd_reduce");
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_layernorm_fwd(const void *x, const void *gamma, const void *beta, void *y, float *mean,
                                    float *rstd, int M, int D, float eps, void *stream) {
    const LnFwdPlan p = ln_fwd_plan(x, gamma, beta, y, mean, rstd, M, D, read_rowwise_knobs());
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(p.blocks), block(THREADS);
    const auto *xp = static_cast<const uint16_t *>(x);
    const auto *gp = static_cast<const uint16_t *>(gamma);
    const auto *bp = static_cast<const uint16_t *>(beta);
    auto *yp = static_cast<uint16_t *>(y);
#define LN_FWD(KERNEL, VPL) hipLaunchKernelGGL(KERNEL<VPL>, grid, block, 0, s, xp, gp, bp, yp, mean, rstd, M, D, eps)
    if (p.two_rows && p.vpl == 3) LN_FWD(ln_fwd2_kernel, 3);
    else if (p.two_rows) LN_FWD(ln_fwd2_kernel, 4);
    else if (p.vpl == 1) LN_FWD(ln_fwd_kernel, 1);
    else if (p.vpl == 2) LN_FWD(ln_fwd_kernel, 2);
    else if (p.vpl == 4) LN_FWD(ln_fwd_kernel, 4);
    else LN_FWD(ln_fwd_kernel, 8);
#undef LN_FWD
    return check_launch("layernorm_fwd");
}

extern "C" int64_t sfcvit_layernorm_bwd_ws(int M, int D) {
    if (M <= 0 || D <= 0) return 0;
    return ln_bwd_geometry(M, D, false, read_rowwise_knobs()).ws_bytes;
}

extern "C" int sfcvit_layernorm_bwd_drop(const void *dy, const void *x, const float *mean, const float *rstd,
                                         const void *gamma, const void *dx_add, void *dx, void *dx_drop, float p,
                                         uint32_t seed, const uint32_t *seed_off, void *dgamma, void *dbeta, void *dcol,
                                         int grads_bf16, int M, int D, void *ws, void *stream) {
    const LnBwdPlan pl = ln_bwd_plan(dy, x, mean, rstd, gamma, dx_add, dx, dx_drop, p, dgamma, dbeta, M, D, ws, read_rowwise_knobs());
    if (pl.err) return fail(pl.err, "%s", pl.msg);
    return launch_ln_bwd(pl, false, dy, x, mean, rstd, gamma, dx_add, dx, dx_drop, p, seed, seed_off, dgamma, dbeta, dcol, grads_bf16,
                         ws, 0, 0.f, 0u, stream);
}

extern "C" int sfcvit_layernorm_bwd(const void *dy, const void *x, const float *mean, const float *rstd,
                                    const void *gamma, const void *dx_add, void *dx, float *dgamma, float *dbeta,
                                    int M, int D, void *ws, void *stream) {
    return sfcvit_layernorm_bwd_drop(dy, x, mean, rstd, gamma, dx_add, dx, nullptr, 0.f, 0u, nullptr, dgamma, dbeta, nullptr, 0, M, D, ws, stream);
}

// Stochastic depth: the two entry points of drop_path.h.
extern "C" int sfcvit_add_layernorm_path_fwd(const void *branch, const void *x, const void *gamma, const void *beta, void *s_out,
                                             void *y, float *mean, float *rstd, int B, int N, int D, float eps, float rate,
                                             uint32_t seed, const uint32_t *seed_off, void *stream) {
    const AddLnPathPlan p = add_ln_path_plan(branch, x, gamma, beta, s_out, y, mean, rstd, B, N, D, rate);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(p.blocks), block(THREADS);
    const auto *ap = static_cast<const uint16_t *>(branch);
    const auto *xp = static_cast<const uint16_t *>(x);
    const auto *gp = static_cast<const uint16_t *>(gamma);
    const auto *bp = static_cast<const uint16_t *>(beta);
    auto *sp = static_cast<uint16_t *>(s_out);
    auto *yp = static_cast<uint16_t *>(y);
    g_rowwise.set("add_ln_path_kernel<%d>", p.vpl);
#define ADD_LN(VPL) hipLaunchKernelGGL(add_ln_path_kernel<VPL>, grid, block, 0, s, ap, xp, gp, bp, sp, yp, mean, rstd, p.M, N, D, eps, rate, seed, seed_off)
    if (p.vpl == 1) ADD_LN(1);
    else if (p.vpl == 2) ADD_LN(2);
    else if (p.vpl == 4) ADD_LN(4);
    else ADD_LN(8);
#undef ADD_LN
    return check_launch("add_layernorm_path_fwd");
}

extern "C" int sfcvit_layernorm_bwd_path(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma,
                                         const void *dx_add, void *dx, void *dx_drop, float p, uint32_t seed,
                                         const uint32_t *seed_off, void *dgamma, void *dbeta, void *dcol, int grads_bf16, int B,
                                         int rows_per_image, int D, void *ws, float path_rate, uint32_t path_seed, void *stream) {
    const LnBwdPathPlan pl = ln_bwd_path_plan(dy, x, mean, rstd, gamma, dx_add, dx, dx_drop, p, dgamma, dbeta, B, rows_per_image, D, ws,
                                              path_rate, read_rowwise_knobs());
    if (pl.err) return fail(pl.err, "%s", pl.msg);
    return launch_ln_bwd(pl, true, dy, x, mean, rstd, gamma, dx_add, dx, dx_drop, p, seed, seed_off, dgamma, dbeta, dcol, grads_bf16,
                         ws, rows_per_image, path_rate, path_seed, stream);
}
