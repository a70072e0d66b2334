// QK-norm for gfx950: LayerNorm over the head dim on the queries and keys of a packed projection qkv [M, 3 * H * hp], in place,
// forward and backward (include/sfcvit.h, "QK-norm").  Geometry of qk_norm.h: 8 lanes own a head row, a wave owns 8 consecutive
// head slots and walks tokens -- with hp = 64 every wave access is 1 KB contiguous -- so a lane's gamma / beta and, in the
// backward, its dgamma / dbeta / column-sum partials stay in registers for the whole token loop.  No statistics are stored: the
// backward recomputes mean and rstd from the raw q | k copy with the forward's own function (qk_stats), so both directions see
// the same fp32 values.  Reductions are deterministic: per-workgroup partials, then one fixed-order second stage; no atomics.
#include "common_host.h"
#include "qk_norm.h"
#include "rowwise_device.h"

namespace sfcvit {
namespace {

constexpr int THREADS = QK_THREADS;         // the plans (qk_norm.h) size the grids for this
constexpr int WAVES = QK_WAVES;

// Sum over the 8 lanes of a head row (lanes that share lane >> 3), result in every one of them.
__device__ __forceinline__ float group8_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// The lane's columns of its head row: vector i covers columns 8 * (sub + 8 i) .. + 7, sub = lane & 7.
__device__ __forceinline__ int qk_col(int sub, int i) { return 8 * (sub + 8 * i); }

// mean and rstd of one head row over its hd real columns, fp32 from the bf16 values, the variance centred (second pass over
// the registers).  The ONE place both directions take them from.  Called by all 64 lanes (shuffles inside).
template <int VPL>
__device__ __forceinline__ void qk_stats(const float (&x)[VPL][8], int sub, int hd, float eps, float &mean, float &rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) s += qk_col(sub, i) + j < hd ? x[i][j] : 0.f;
    mean = group8_sum(s) / float(hd);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float d = x[i][j] - mean;
            q += qk_col(sub, i) + j < hd ? d * d : 0.f;
        }
    rstd = rsqrtf(group8_sum(q) / float(hd) + eps);
}

// The lane's gamma / beta: rows (k ? 2 : 0) and (k ? 3 : 1) of P [4, hd]; columns >= hd read nothing and hold 0.
template <int VPL>
__device__ __forceinline__ void qk_params(const uint16_t *__restrict__ P, bool is_k, int sub, int hd, float (&g)[VPL][8],
                                          float (&b)[VPL][8]) {
    const uint16_t *gw = P + size_t(is_k ? 2 : 0) * hd, *bw = gw + hd;
#pragma unroll
    for (int i = 0; i < VPL; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int c = qk_col(sub, i) + j;
            g[i][j] = c < hd ? bf2f(gw[c]) : 0.f;
            b[i][j] = c < hd ? bf2f(bw[c]) : 0.f;
        }
}

// qkv[m, slot j] <- LayerNorm_hd(q or k head row) * gamma + beta (columns >= hd: +0), raw[m, slot j] <- the bits read.
// The v third is neither read nor written.
template <int HP>
__global__ __launch_bounds__(THREADS) void qk_norm_fwd_kernel(uint16_t *__restrict__ qkv, uint16_t *__restrict__ raw,
                                                              const uint16_t *__restrict__ P, int M, int H, int hd, float eps,
                                                              int chunks) {
    constexpr int VPL = HP / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 7;
    const int sg = blockIdx.x / chunks, chunk = blockIdx.x - sg * chunks;
    const int slot = sg * QK_SLOTS + (lane >> 3);
    const bool active = slot < 2 * H;
    const size_t Da = size_t(H) * HP;
    float g[VPL][8], b[VPL][8];
    qk_params<VPL>(P, slot >= H, sub, hd, g, b);
    const int r0 = chunk * QK_ROWS_PER_WG, r1 = min(M, r0 + QK_ROWS_PER_WG);
    u32x4 xr[VPL], xn[VPL];
    auto load_row = [&](int m, u32x4 (&xq)[VPL]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < VPL; i++)
            xq[i] = active ? *reinterpret_cast<const u32x4 *>(qkv + size_t(m) * 3 * Da + size_t(slot) * HP + qk_col(sub, i))
                           : u32x4{0u, 0u, 0u, 0u};
    };
    int m = r0 + wave;
    if (m < r1) load_row(m, xr);
    for (; m < r1; m += WAVES) {
        const bool more = m + WAVES < r1;
        if (more) load_row(m + WAVES, xn);                      // the next row's loads fly while this one is reduced
        float x[VPL][8];
#pragma unroll
        for (int i = 0; i < VPL; i++) unpack8(xr[i], x[i]);
        float mean, rstd;
        qk_stats<VPL>(x, sub, hd, eps, mean, rstd);
        if (active) {
#pragma unroll
            for (int i = 0; i < VPL; i++) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; j++) o[j] = qk_col(sub, i) + j < hd ? (x[i][j] - mean) * rstd * g[i][j] + b[i][j] : 0.f;
                *reinterpret_cast<u32x4 *>(raw + size_t(m) * 2 * Da + size_t(slot) * HP + qk_col(sub, i)) = xr[i];
                *reinterpret_cast<u32x4 *>(qkv + size_t(m) * 3 * Da + size_t(slot) * HP + qk_col(sub, i)) = pack8(o);
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < VPL; i++) xr[i] = xn[i];
        }
    }
}

// dqkv[m, slot j] <- rstd * (g - mean(g) - xh * mean(g * xh)), g = dy * gamma, over the hd real columns (columns >= hd: +0,
// whatever they held); per-workgroup partials [part_ld]: the column sums of the STORED dq | dk of its 8 slots [8 HP], then
// q dgamma | q dbeta | k dgamma | k dbeta [HP each].
template <int HP>
__global__ __launch_bounds__(THREADS) void qk_norm_bwd_kernel(uint16_t *__restrict__ dqkv, const uint16_t *__restrict__ raw,
                                                              const uint16_t *__restrict__ P, float *__restrict__ partial, int M,
                                                              int H, int hd, float eps, int chunks) {
    constexpr int VPL = HP / 64;
    __shared__ __attribute__((aligned(16))) float red[WAVES][QK_SLOTS * HP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 7, grp = lane >> 3;
    const int sg = blockIdx.x / chunks, chunk = blockIdx.x - sg * chunks;
    const int slot = sg * QK_SLOTS + grp;
    const bool active = slot < 2 * H;
    const size_t Da = size_t(H) * HP;
    float g[VPL][8], dg[VPL][8], db[VPL][8], dc[VPL][8];
    {
        float b[VPL][8];
        qk_params<VPL>(P, slot >= H, sub, hd, g, b);
    }
#pragma unroll
    for (int i = 0; i < VPL; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) dg[i][j] = db[i][j] = dc[i][j] = 0.f;
    const int r0 = chunk * QK_ROWS_PER_WG, r1 = min(M, r0 + QK_ROWS_PER_WG);
    u32x4 xr[VPL], dr[VPL], xn[VPL], dn[VPL];
    auto load_row = [&](int m, u32x4 (&xq)[VPL], u32x4 (&dq)[VPL]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            xq[i] = active ? *reinterpret_cast<const u32x4 *>(raw + size_t(m) * 2 * Da + size_t(slot) * HP + qk_col(sub, i))
                           : u32x4{0u, 0u, 0u, 0u};
            dq[i] = active ? *reinterpret_cast<const u32x4 *>(dqkv + size_t(m) * 3 * Da + size_t(slot) * HP + qk_col(sub, i))
                           : u32x4{0u, 0u, 0u, 0u};
        }
    };
    int m = r0 + wave;
    if (m < r1) load_row(m, xr, dr);
    for (; m < r1; m += WAVES) {
        const bool more = m + WAVES < r1;
        if (more) load_row(m + WAVES, xn, dn);
        float x[VPL][8];
#pragma unroll
        for (int i = 0; i < VPL; i++) unpack8(xr[i], x[i]);
        float mean, rstd;
        qk_stats<VPL>(x, sub, hd, eps, mean, rstd);
        float xh[VPL][8], gy[VPL][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            float dv[8];
            unpack8(dr[i], dv);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const bool real = active && qk_col(sub, i) + j < hd;   // a padded column's dy may hold anything, NaN included: selected out
                const float d = real ? dv[j] : 0.f;
                xh[i][j] = real ? (x[i][j] - mean) * rstd : 0.f;
                gy[i][j] = d * g[i][j];
                s1 += gy[i][j];
                s2 += gy[i][j] * xh[i][j];
                dg[i][j] += d * xh[i][j];
                db[i][j] += d;
            }
        }
        const float c1 = group8_sum(s1) / float(hd), c2 = group8_sum(s2) / float(hd);
        if (active) {
#pragma unroll
            for (int i = 0; i < VPL; i++) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; j++) o[j] = qk_col(sub, i) + j < hd ? rstd * (gy[i][j] - c1 - xh[i][j] * c2) : 0.f;
                const u32x4 stored = pack8(o);
                *reinterpret_cast<u32x4 *>(dqkv + size_t(m) * 3 * Da + size_t(slot) * HP + qk_col(sub, i)) = stored;
                unpack8(stored, o);                              // the column sums are those of what dqkv holds: the rounded values
#pragma unroll
                for (int j = 0; j < 8; j++) dc[i][j] += o[j];
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < VPL; i++) { xr[i] = xn[i]; dr[i] = dn[i]; }
        }
    }
    float *out = partial + size_t(blockIdx.x) * ((QK_SLOTS + 4) * HP);
    auto stage = [&](const float (&v)[VPL][8]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            float *dst = &red[wave][grp * HP + qk_col(sub, i)];
            *reinterpret_cast<f32x4 *>(dst) = f32x4{v[i][0], v[i][1], v[i][2], v[i][3]};
            *reinterpret_cast<f32x4 *>(dst + 4) = f32x4{v[i][4], v[i][5], v[i][6], v[i][7]};
        }
    };
    // round 1: the column sums, waves added in order
    stage(dc);
    __syncthreads();
    for (int c = threadIdx.x; c < QK_SLOTS * HP; c += THREADS) out[c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    __syncthreads();
    // rounds 2, 3: dgamma, dbeta -- the 8 slots of a wave fold onto the head's columns, q slots and k slots apart, in slot order
    for (int round = 0; round < 2; round++) {
        if (round == 0) stage(dg);
        else stage(db);
        __syncthreads();
        for (int e = threadIdx.x; e < 2 * HP; e += THREADS) {
            const int kind = e / HP, col = e - kind * HP;
            float s = 0.f;
            for (int w = 0; w < WAVES; w++)
#pragma unroll
                for (int q = 0; q < QK_SLOTS; q++) {
                    const int sl = sg * QK_SLOTS + q;
                    if (sl < 2 * H && (sl >= H) == (kind == 1)) s += red[w][q * HP + col];
                }
            out[QK_SLOTS * HP + (2 * kind + round) * HP + col] = s;
        }
        __syncthreads();
    }
}

// Second stage, one launch: the workgroups' partials in a fixed order -> the column sums [2 H hp] of dq | dk, dP [4, hd], and,
// with vsum, colsum[2 H hp + i] = vsum[i]: the v third of the in_proj bias gradient, carried over from the attention backward.
__global__ __launch_bounds__(RED_THREADS) void qk_norm_bwd_reduce(const float *__restrict__ partial, void *__restrict__ dparams,
                                                                  int dparams_bf16, void *__restrict__ colsum, int colsum_bf16,
                                                                  const float *__restrict__ vsum, int H, int hd, int hp,
                                                                  int slot_groups, int chunks) {
    const int ld = (QK_SLOTS + 4) * hp, Da2 = 2 * H * hp;
    const int ncb = colsum ? Da2 / 16 : 0, ndb = 4 * hp / 16;
    const int b = blockIdx.x;
    if (b < ncb) {
        const int c = b * 16 + (threadIdx.x & 15);
        const int sg = c / (QK_SLOTS * hp), cc = c - sg * (QK_SLOTS * hp);
        const float t = reduce_partials16(partial + size_t(sg) * chunks * ld, chunks, ld, cc, true);
        if (threadIdx.x < 16) store_grad(colsum, c, t, colsum_bf16);
    } else if (b < ncb + ndb) {
        const int e = (b - ncb) * 16 + (threadIdx.x & 15);
        const int r = e / hp, col = e - r * hp;
        const float t = reduce_partials16(partial + QK_SLOTS * hp, slot_groups * chunks, ld, e, true);
        if (threadIdx.x < 16 && col < hd) store_grad(dparams, r * hd + col, t, dparams_bf16);
    } else {
        const int i = (b - ncb - ndb) * RED_THREADS + threadIdx.x;
        if (vsum && i < H * hp) store_grad(colsum, Da2 + i, vsum[i], colsum_bf16);
    }
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_qk_norm_plan(int M, int H, int hp, int32_t *out) {
    if (!out) return fail(SFCVIT_EINVAL, "qk_norm_plan: null pointer (out)");
    const QkNormPlan p = qk_norm_geometry(M, H, hp, "qk_norm_plan");
    if (p.err) return fail(p.err, "%s", p.msg);
    out[0] = p.rows_per_wg;
    out[1] = p.slot_groups;
    out[2] = p.blocks;
    out[3] = p.vpl;
    return SFCVIT_OK;
}

extern "C" int64_t sfcvit_qk_norm_bwd_ws(int M, int H, int hp) {
    const QkNormPlan p = qk_norm_geometry(M, H, hp, "qk_norm_bwd_ws");
    return p.err ? 0 : p.ws_bytes;
}

extern "C" int sfcvit_qk_norm_fwd(void *qkv, void *raw, const void *params, int M, int H, int hd, int hp, float eps, void *stream) {
    const QkNormPlan p = qk_norm_fwd_plan(qkv, raw, params, M, H, hd, hp, eps);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(p.blocks), block(THREADS);
    auto *qp = static_cast<uint16_t *>(qkv);
    auto *rp = static_cast<uint16_t *>(raw);
    const auto *pp = static_cast<const uint16_t *>(params);
    g_rowwise.set("qk_norm_fwd_kernel<%d>", hp);
#define QK_FWD(HP) hipLaunchKernelGGL(qk_norm_fwd_kernel<HP>, grid, block, 0, s, qp, rp, pp, M, H, hd, eps, p.chunks)
    if (hp == 64) QK_FWD(64);
    else if (hp == 128) QK_FWD(128);
    else if (hp == 192) QK_FWD(192);
    else QK_FWD(256);
#undef QK_FWD
    return check_launch("qk_norm_fwd");
}

extern "C" int sfcvit_qk_norm_bwd(void *dqkv, const void *raw, const void *params, void *dparams, int dparams_is_bf16, void *colsum,
                                  int colsum_is_bf16, const float *vsum, void *ws, int M, int H, int hd, int hp, float eps,
                                  void *stream) {
    const QkNormPlan p = qk_norm_bwd_plan(dqkv, raw, params, dparams, colsum, vsum, ws, M, H, hd, hp, eps);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(p.blocks), block(THREADS);
    auto *dp = static_cast<uint16_t *>(dqkv);
    const auto *rp = static_cast<const uint16_t *>(raw);
    const auto *pp = static_cast<const uint16_t *>(params);
    float *part = static_cast<float *>(ws);
    g_rowwise.set("qk_norm_bwd_kernel<%d>", hp);
#define QK_BWD(HP) hipLaunchKernelGGL(qk_norm_bwd_kernel<HP>, grid, block, 0, s, dp, rp, pp, part, M, H, hd, eps, p.chunks)
    if (hp == 64) QK_BWD(64);
    else if (hp == 128) QK_BWD(128);
    else if (hp == 192) QK_BWD(192);
    else QK_BWD(256);
#undef QK_BWD
    if (int rc = check_launch("qk_norm_bwd")) return rc;
    hipLaunchKernelGGL(qk_norm_bwd_reduce, dim3(p.reduce_blocks), dim3(RED_THREADS), 0, s, part, dparams, dparams_is_bf16, colsum,
                       colsum_is_bf16, vsum, H, hd, hp, p.slot_groups, p.chunks);
    return check_launch("qk_norm_bwd_reduce");
}
