// The LayerScale residual site of a pre-norm encoder layer for gfx950: "residual site + the LayerNorm after it", forward and
// backward, with a per-channel scale lam[D] on the branch and (optionally) stochastic depth.  Kernels of their own next to
// layernorm.hip's add_ln_path_kernel / ln_bwd_path_kernel / ln_bwd_cols_path_kernel, whose geometry (one 64-lane wave per row, 16-byte vectors, wave
// butterflies, per-workgroup partial rows) and arithmetic they keep: with lam = 1 they give those kernels' bits.  The launchers
// run what the plans of layer_scale.h say.
#include "common_host.h"
#include "layer_scale.h"
#include "rowwise_device.h"

namespace sfcvit {
namespace {

constexpr int THREADS = ROW_THREADS;        // the plans (rowwise.h) size the grids for this
constexpr int WAVES = ROW_WAVES;

// s = bf16(x + (c[b] * lam[d]) * branch), y = LayerNorm(s), one wave per row.  c[b] = keep(b) / (1 - rate) with keep(b)
// element (b, 0) of the dropout mask of `seed`, b = row / N; rate = 0: c = 1 and no flag is evaluated.  A dropped image's rows
// never read the branch and store the bits of x; LayerNorm's statistics and y come from the ROUNDED s.
template <int VPL>
__global__ __launch_bounds__(THREADS) void add_ln_scale_kernel(const uint16_t *__restrict__ branch, const uint16_t *__restrict__ x,
                                                               const uint16_t *__restrict__ lam,
                                                               const uint16_t *__restrict__ gamma, const uint16_t *__restrict__ beta,
                                                               uint16_t *__restrict__ sum, uint16_t *__restrict__ y,
                                                               float *__restrict__ mean, float *__restrict__ rstd, int M, int N,
                                                               int D, float eps, float rate, uint32_t seed_arg,
                                                               const uint32_t *__restrict__ seed_off) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (row >= M) return;
    const bool keep = rate > 0.f ? drop_keep(drop_row_key(eff_seed(seed_arg, seed_off), uint64_t(row / N)), 0u, drop_thresh(rate)) : true;
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
                float a[8], l[8];
                unpack8(ar[i], a);
                unpack8(*reinterpret_cast<const u32x4 *>(lam + c * 8), l);
#pragma unroll
                for (int j = 0; j < 8; j++) v[i][j] += (sc * l[j]) * a[j];
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

// ln_bwd_path_kernel (layernorm.hip) plus the channel scale (sfcvit_layernorm_bwd_scale): dx = g, the gradient of s;
// dx_drop = keep_path(b) && keep(m, d) ? g * lam[d] / ((1 - p)(1 - path_rate)) : 0, always written; dcol sums the ROUNDED dx_drop;
// dlam[d] = sum_m dx_stored[m, d] * c[b] * branch[m, d] from the ROUNDED dx, dropped images adding nothing and their branch rows
// never read.  Partial rows are [4][D]: dgamma | dbeta | dcol | dlam.  The four per-wave sums go through the [WAVES][3][D] LDS
// region of the three-sum kernels in two rounds, so the launch needs no more LDS than theirs (96 KiB at D = 2 048).
// At VPL = 4 lam is re-read per row (L2-resident) instead of held: 32 registers less.
template <int VPL, bool ADD>
__global__ __launch_bounds__(THREADS) void ln_bwd_scale_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                               const float *__restrict__ mean, const float *__restrict__ rstd,
                                                               const uint16_t *__restrict__ gamma,
                                                               const uint16_t *__restrict__ dx_add,
                                                               const uint16_t *__restrict__ branch, const uint16_t *__restrict__ lam,
                                                               uint16_t *__restrict__ dx, uint16_t *__restrict__ dx_drop,
                                                               float drop_p, uint32_t drop_seed_arg,
                                                               const uint32_t *__restrict__ seed_off,
                                                               float *__restrict__ partial, int M, int D, int rows_per_image,
                                                               float path_rate, uint32_t path_seed_arg) {
    constexpr bool HOLD = VPL < 4;
    const uint32_t drop_seed = eff_seed(drop_seed_arg, seed_off);
    const uint32_t path_seed = eff_seed(path_seed_arg, seed_off), path_th = drop_thresh(path_rate);
    const bool has_path = path_rate > 0.f;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [WAVES][3][D] fp32
    const uint32_t drop_th = drop_thresh(drop_p);
    const float drop_sc = 1.f / (1.f - drop_p), path_c = 1.f / (1.f - path_rate), path_mul = drop_sc / (1.f - path_rate);
    float *red = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = D >> 3;
    float g[VPL][8], dg[VPL][8], db[VPL][8], dc[VPL][8], dl[VPL][8];
    float lm[HOLD ? VPL : 1][8];                            // lam * path_mul: the multiplier of the outgoing gradient
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) {
            unpack8(*reinterpret_cast<const u32x4 *>(gamma + c * 8), g[i]);
            if (HOLD) {
                unpack8(*reinterpret_cast<const u32x4 *>(lam + c * 8), lm[HOLD ? i : 0]);
#pragma unroll
                for (int j = 0; j < 8; j++) lm[HOLD ? i : 0][j] *= path_mul;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) dg[i][j] = db[i][j] = dc[i][j] = dl[i][j] = 0.f;
    }
    // Rows are software-pipelined as in ln_bwd_kernel: the loads of this wave's next row are issued before the current row is reduced.
    const int stride = gridDim.x * WAVES;
    u32x4 xr[VPL], dr[VPL], ar[VPL], br[VPL], xn[VPL], dn[VPL], an[VPL], bn[VPL];
    float mu = 0.f, rs = 0.f, mun = 0.f, rsn = 0.f;
    bool kc = true, kn = true;                              // the DropPath flag of the current / next row's image
    auto load_row = [&](int row, u32x4 (&xq)[VPL], u32x4 (&dq)[VPL], u32x4 (&aq)[VPL], u32x4 (&bq)[VPL], float &m, float &r,
                        bool &k) __attribute__((always_inline)) {
        m = mean[row];
        r = rstd[row];
        k = has_path ? drop_keep(drop_row_key(path_seed, uint64_t(row / rows_per_image)), 0u, path_th) : true;
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            const int c = lane + 64 * i;
            if (c < nvec) {
                xq[i] = *reinterpret_cast<const u32x4 *>(x + size_t(row) * D + c * 8);
                dq[i] = *reinterpret_cast<const u32x4 *>(dy + size_t(row) * D + c * 8);
                if (ADD) aq[i] = *reinterpret_cast<const u32x4 *>(dx_add + size_t(row) * D + c * 8);
                if (k) bq[i] = *reinterpret_cast<const u32x4 *>(branch + size_t(row) * D + c * 8);
            }
        }
    };
    int row = blockIdx.x * WAVES + wave;
    if (row < M) load_row(row, xr, dr, ar, br, mu, rs, kc);
    for (; row < M; row += stride) {
        const bool more = row + stride < M;
        if (more) load_row(row + stride, xn, dn, an, bn, mun, rsn, kn);
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
        const bool path_keep = kc;
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
                const u32x4 dxs = pack8(o);
                *reinterpret_cast<u32x4 *>(dx + size_t(row) * D + c * 8) = dxs;
                if (path_keep) {                                // dlam from the rounded dx and this row's branch
                    float r8[8], b8[8];
                    unpack8(dxs, r8);
                    unpack8(br[i], b8);
#pragma unroll
                    for (int j = 0; j < 8; j++) dl[i][j] += r8[j] * b8[j];
                }
                {
                    float mulv[8];
                    if constexpr (HOLD) {
#pragma unroll
                        for (int j = 0; j < 8; j++) mulv[j] = lm[i][j];
                    } else {
                        unpack8(*reinterpret_cast<const u32x4 *>(lam + c * 8), mulv);
#pragma unroll
                        for (int j = 0; j < 8; j++) mulv[j] *= path_mul;
                    }
                    const uint32_t rk = drop_row_key(drop_seed, uint64_t(row));
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        bool k0, k1;
                        drop_keep2(rk, uint32_t(c * 4 + q), drop_th, k0, k1);
                        o[2 * q] = (k0 && path_keep) ? o[2 * q] * mulv[2 * q] : 0.f;
                        o[2 * q + 1] = (k1 && path_keep) ? o[2 * q + 1] * mulv[2 * q + 1] : 0.f;
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
            for (int i = 0; i < VPL; i++) { xr[i] = xn[i]; dr[i] = dn[i]; ar[i] = an[i]; br[i] = bn[i]; }
            mu = mun;
            rs = rsn;
            kc = kn;
        }
    }
    // round 1: dgamma | dbeta | dcol through the [WAVES][3][D] region, as the three-sum kernels do
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
        partial[size_t(blockIdx.x) * 4 * D + c] = s;
    }
    __syncthreads();
    // round 2: dlam through the first [WAVES][D] floats of the same region; c[b] = 1 / (1 - path_rate) for every kept row
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const int c = lane + 64 * i;
        if (c < nvec) {
#pragma unroll
            for (int j = 0; j < 8; j++) red[wave * D + c * 8 + j] = dl[i][j] * path_c;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += THREADS) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += red[w * D + c];
        partial[size_t(blockIdx.x) * 4 * D + 3 * D + c] = s;
    }
}

// The same for D = 256 CH (768, 1 024) in the column-chunk layout of ln_bwd_cols_path_kernel (layernorm.hip): a lane owns CH chunks of
// 4 columns, all arithmetic on float pairs, so dx / dx_drop / dgamma / dbeta keep THAT kernel's lane sums and bits at lam = 1.
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ f32x2 unpack2(uint32_t w) { return f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)}; }

template <int CH, bool ADD>
__global__ __launch_bounds__(THREADS) void ln_bwd_cols_scale_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                                    const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                    const uint16_t *__restrict__ gamma,
                                                                    const uint16_t *__restrict__ dx_add,
                                                                    const uint16_t *__restrict__ branch, const uint16_t *__restrict__ lam,
                                                                    uint16_t *__restrict__ dx, uint16_t *__restrict__ dx_drop,
                                                                    float drop_p, uint32_t drop_seed_arg,
                                                                    const uint32_t *__restrict__ seed_off,
                                                                    float *__restrict__ partial, int M, int rows_per_image,
                                                                    float path_rate, uint32_t path_seed_arg) {
    constexpr int D = 256 * CH;
    const uint32_t drop_seed = eff_seed(drop_seed_arg, seed_off);
    const uint32_t path_seed = eff_seed(path_seed_arg, seed_off), path_th = drop_thresh(path_rate);
    const bool has_path = path_rate > 0.f;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [WAVES][3][D] fp32
    const uint32_t drop_th = drop_thresh(drop_p);
    const float drop_sc = 1.f / (1.f - drop_p), path_c = 1.f / (1.f - path_rate), path_mul = drop_sc / (1.f - path_rate);
    float *red = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // lane's columns: 256 k + 4 lane + 2 h + {0, 1}, k < CH, h < 2
    f32x2 g[CH][2], lm[CH][2], dg[CH][2], db[CH][2], dc[CH][2], dl[CH][2];
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const u32x2 w = *reinterpret_cast<const u32x2 *>(gamma + 256 * k + 4 * lane);
        const u32x2 l = *reinterpret_cast<const u32x2 *>(lam + 256 * k + 4 * lane);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            g[k][h] = unpack2(w[h]);
            lm[k][h] = unpack2(l[h]) * path_mul;                // the multiplier of the outgoing gradient
            dg[k][h] = db[k][h] = dc[k][h] = dl[k][h] = f32x2{0.f, 0.f};
        }
    }
    const int stride = gridDim.x * WAVES;
    u32x2 xr[CH], dr[CH], ar[CH], br[CH], xn[CH], dn[CH], an[CH], bn[CH];
    float mu = 0.f, rs = 0.f, mun = 0.f, rsn = 0.f;
    bool kc = true, kn = true;                              // the DropPath flag of the current / next row's image
    auto load_row = [&](int row, u32x2 (&xq)[CH], u32x2 (&dq)[CH], u32x2 (&aq)[CH], u32x2 (&bq)[CH], float &m, float &r,
                        bool &kp) __attribute__((always_inline)) {
        m = mean[row];
        r = rstd[row];
        kp = has_path ? drop_keep(drop_row_key(path_seed, uint64_t(row / rows_per_image)), 0u, path_th) : true;
        const size_t o = size_t(row) * D + 4 * lane;
#pragma unroll
        for (int k = 0; k < CH; k++) {
            xq[k] = *reinterpret_cast<const u32x2 *>(x + o + 256 * k);
            dq[k] = *reinterpret_cast<const u32x2 *>(dy + o + 256 * k);
            if (ADD) aq[k] = *reinterpret_cast<const u32x2 *>(dx_add + o + 256 * k);
            if (kp) bq[k] = *reinterpret_cast<const u32x2 *>(branch + o + 256 * k);
        }
    };
    int row = blockIdx.x * WAVES + wave;
    if (row < M) load_row(row, xr, dr, ar, br, mu, rs, kc);
    for (; row < M; row += stride) {
        const bool more = row + stride < M;
        if (more) load_row(row + stride, xn, dn, an, bn, mun, rsn, kn);   // the next row's loads fly while this one is reduced
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
        const bool path_keep = kc;
#pragma unroll
        for (int k = 0; k < CH; k++) {
            f32x2 ov[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                ov[h] = rs * (gy[k][h] - c1 - xh[k][h] * c2);
                if (ADD) ov[h] += unpack2(ar[k][h]);
            }
            const u32x2 dxs = u32x2{pack2bf(ov[0][0], ov[0][1]), pack2bf(ov[1][0], ov[1][1])};
            *reinterpret_cast<u32x2 *>(dx + o + 256 * k) = dxs;
            if (path_keep) {                                    // dlam from the rounded dx and this row's branch
                dl[k][0] += unpack2(dxs[0]) * unpack2(br[k][0]);
                dl[k][1] += unpack2(dxs[1]) * unpack2(br[k][1]);
            }
#pragma unroll
            for (int h = 0; h < 2; h++) {
                bool k0, k1;
                drop_keep2(rk, uint32_t(128 * k + 2 * lane + h), drop_th, k0, k1);      // pair = column / 2
                ov[h][0] = (k0 && path_keep) ? ov[h][0] * lm[k][h][0] : 0.f;
                ov[h][1] = (k1 && path_keep) ? ov[h][1] * lm[k][h][1] : 0.f;
            }
            const u32x2 stored = u32x2{pack2bf(ov[0][0], ov[0][1]), pack2bf(ov[1][0], ov[1][1])};
            *reinterpret_cast<u32x2 *>(dx_drop + o + 256 * k) = stored;
            dc[k][0] += unpack2(stored[0]);                      // dcol sums what dx_drop holds: the rounded values
            dc[k][1] += unpack2(stored[1]);
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < CH; k++) { xr[k] = xn[k]; dr[k] = dn[k]; ar[k] = an[k]; br[k] = bn[k]; }
            mu = mun;
            rs = rsn;
            kc = kn;
        }
    }
    // two rounds through the [WAVES][3][D] region, as ln_bwd_scale_kernel
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
        partial[size_t(blockIdx.x) * 4 * D + c] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const int c = 256 * k + 4 * lane;
        *reinterpret_cast<f32x4 *>(red + wave * D + c) = f32x4{dl[k][0][0], dl[k][0][1], dl[k][1][0], dl[k][1][1]} * path_c;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += THREADS) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += red[w * D + c];
        partial[size_t(blockIdx.x) * 4 * D + 3 * D + c] = s;
    }
}

// [nblocks][4][D] partials -> dgamma | dbeta | column sums of the outgoing gradient | dlam.
__global__ __launch_bounds__(RED_THREADS) void ln_bwd_scale_reduce(const float *__restrict__ partial, void *__restrict__ dgamma,
                                                                  void *__restrict__ dbeta, void *__restrict__ dcol,
                                                                  void *__restrict__ dlam, int nblocks, int D, int as_bf16) {
    const int c = blockIdx.x * 16 + (threadIdx.x & 15);
    const float t = reduce_partials16(partial, nblocks, 4 * D, c, c < 4 * D);
    if (threadIdx.x < 16 && c < 4 * D) {
        if (c < D) store_grad(dgamma, c, t, as_bf16);
        else if (c < 2 * D) store_grad(dbeta, c - D, t, as_bf16);
        else if (c < 3 * D) { if (dcol) store_grad(dcol, c - 2 * D, t, as_bf16); }
        else store_grad(dlam, c - 3 * D, t, as_bf16);
    }
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_add_layernorm_scale_fwd(const void *branch, const void *x, const void *lam, const void *gamma, const void *beta,
                                              void *s_out, void *y, float *mean, float *rstd, int B, int N, int D, float eps,
                                              float rate, uint32_t seed, const uint32_t *seed_off, void *stream) {
    const AddLnScalePlan p = add_ln_scale_plan(branch, x, lam, gamma, beta, s_out, y, mean, rstd, B, N, D, rate);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(p.blocks), block(THREADS);
    const auto *ap = static_cast<const uint16_t *>(branch);
    const auto *xp = static_cast<const uint16_t *>(x);
    const auto *lp = static_cast<const uint16_t *>(lam);
    const auto *gp = static_cast<const uint16_t *>(gamma);
    const auto *bp = static_cast<const uint16_t *>(beta);
    auto *sp = static_cast<uint16_t *>(s_out);
    auto *yp = static_cast<uint16_t *>(y);
    g_rowwise.set("add_ln_scale_kernel<%d>", p.vpl);
#define ADD_LN(VPL) hipLaunchKernelGGL(add_ln_scale_kernel<VPL>, grid, block, 0, s, ap, xp, lp, gp, bp, sp, yp, mean, rstd, p.M, N, D, eps, rate, seed, seed_off)
    if (p.vpl == 1) ADD_LN(1);
    else if (p.vpl == 2) ADD_LN(2);
    else if (p.vpl == 4) ADD_LN(4);
    else ADD_LN(8);
#undef ADD_LN
    return check_launch("add_layernorm_scale_fwd");
}

extern "C" int64_t sfcvit_layernorm_bwd_scale_ws(int M, int D) {
    if (M <= 0 || D <= 0) return 0;
    return ln_bwd_scale_geometry(M, D, false, read_rowwise_knobs()).ws_bytes;
}

extern "C" int sfcvit_layernorm_bwd_scale(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma,
                                          const void *dx_add, const void *branch, const void *lam, void *dx, void *dx_drop, float p,
                                          uint32_t seed, const uint32_t *seed_off, void *dgamma, void *dbeta, void *dcol, void *dlam,
                                          int grads_bf16, int B, int rows_per_image, int D, void *ws, float path_rate,
                                          uint32_t path_seed, void *stream) {
    const LnBwdScalePlan pl = ln_bwd_scale_plan(dy, x, mean, rstd, gamma, dx_add, branch, lam, dx, dx_drop, p, dgamma, dbeta, dlam, B,
                                                rows_per_image, D, ws, path_rate, read_rowwise_knobs());
    if (pl.err) return fail(pl.err, "%s", pl.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(pl.blocks), block(THREADS);
    const int M = pl.M, nb = pl.blocks;
    const auto *dyp = static_cast<const uint16_t *>(dy);
    const auto *xp = static_cast<const uint16_t *>(x);
    const auto *gp = static_cast<const uint16_t *>(gamma);
    const auto *ap = static_cast<const uint16_t *>(dx_add);
    const auto *bp = static_cast<const uint16_t *>(branch);
    const auto *lp = static_cast<const uint16_t *>(lam);
    auto *dxp = static_cast<uint16_t *>(dx);
    auto *ddp = static_cast<uint16_t *>(dx_drop);
    float *part = static_cast<float *>(ws);
    scale_kernel_name(pl, g_rowwise.name, sizeof(g_rowwise.name));
#define LN_BWD(INST) do { \
        if (pl.add) hipLaunchKernelGGL((ln_bwd_scale_kernel<INST, true>), grid, block, pl.lds, s, dyp, xp, mean, rstd, gp, ap, bp, lp, dxp, ddp, p, seed, seed_off, part, M, D, rows_per_image, path_rate, path_seed); \
        else hipLaunchKernelGGL((ln_bwd_scale_kernel<INST, false>), grid, block, pl.lds, s, dyp, xp, mean, rstd, gp, ap, bp, lp, dxp, ddp, p, seed, seed_off, part, M, D, rows_per_image, path_rate, path_seed); } while (0)
    if (pl.cols) {
#define LN_BWD_COLS(CH) do { \
        if (pl.add) hipLaunchKernelGGL((ln_bwd_cols_scale_kernel<CH, true>), grid, block, pl.lds, s, dyp, xp, mean, rstd, gp, ap, bp, lp, dxp, ddp, p, seed, seed_off, part, M, rows_per_image, path_rate, path_seed); \
        else hipLaunchKernelGGL((ln_bwd_cols_scale_kernel<CH, false>), grid, block, pl.lds, s, dyp, xp, mean, rstd, gp, ap, bp, lp, dxp, ddp, p, seed, seed_off, part, M, rows_per_image, path_rate, path_seed); } while (0)
        if (pl.inst == 3) LN_BWD_COLS(3);
        else LN_BWD_COLS(4);
#undef LN_BWD_COLS
    } else if (pl.inst == 1) LN_BWD(1);
    else if (pl.inst == 2) LN_BWD(2);
    else LN_BWD(4);
#undef LN_BWD
    if (int rc = check_launch("layernorm_bwd_scale")) return rc;
    if (reduce_deferring()) {            // queued for the batched launch at sfcvit_reduce_flush: partial rows are [4][D]
        reduce_cols(part, nb, 4 * D, D, dgamma, grads_bf16, stream);
        reduce_cols(part + D, nb, 4 * D, D, dbeta, grads_bf16, stream);
        if (dcol) reduce_cols(part + 2 * D, nb, 4 * D, D, dcol, grads_bf16, stream);
        reduce_cols(part + 3 * D, nb, 4 * D, D, dlam, grads_bf16, stream);
        return SFCVIT_OK;
    }
    hipLaunchKernelGGL(ln_bwd_scale_reduce, dim3((4 * D + 15) / 16), dim3(RED_THREADS), 0, s, part, dgamma, dbeta, dcol, dlam, nb, D, grads_bf16);
    return check_launch("layernorm_bwd_scale_reduce");
}
