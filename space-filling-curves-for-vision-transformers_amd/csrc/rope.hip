// Rotary position embedding for gfx950: the 2x2 map [c -s; s c] (forward) and its transpose (backward) on the interleaved channel
// pairs of the queries and keys of a packed projection qkv [B * N, 3 * H * hp], in place (include/sfcvit.h, "RoPE").  Geometry of
// rope.h: 8 lanes own a head row, a wave owns 8 consecutive head slots, fixes one token and walks the batch -- with hp = 64
// every wave access is 1 KB contiguous -- so a lane's (c, s) values are loaded once and, in the backward, its column-sum
// partials stay in registers for the whole loop.  A lane's 16-byte vector holds 4 whole pairs: no cross-lane traffic.  Nothing
// is saved between the directions.  The sums are deterministic: per-workgroup partials, one fixed-order second stage, no atomics.
#include "common_host.h"
#include "rope.h"
#include "rowwise_device.h"

namespace sfcvit {
namespace {

constexpr int THREADS = ROPE_THREADS;       // the plans (rope.h) size the grids for this
constexpr int WAVES = ROPE_WAVES;

// The lane's columns of its head row: vector i covers columns 8 * (sub + 8 i) .. + 7, sub = lane & 7.
__device__ __forceinline__ int rope_col(int sub, int i) { return 8 * (sub + 8 * i); }

// The lane's (c, s) of token n: table [N, hd / 2, 2], so the float at column col of a head row is table[n * hd + col] -- c at
// the even column of a pair, s at the odd one.  Columns >= hd read nothing and hold 0.
template <int VPL>
__device__ __forceinline__ void rope_cs(const float *__restrict__ table, int n, int sub, int hd, bool on, float (&cs)[VPL][8]) {
    const float *row = table + size_t(n) * hd;
#pragma unroll
    for (int i = 0; i < VPL; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int c = rope_col(sub, i) + j;
            cs[i][j] = on && c < hd ? row[c] : 0.f;
        }
}

// Workgroup -> (slot group, token block, batch chunk), the order of rope.h.
struct RopeWho {
    int slot, n, b0, b1;
    bool active;
};
__device__ __forceinline__ RopeWho rope_who(int B, int N, int H, int token_blocks, int batch_chunks) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bc = blockIdx.x % batch_chunks, rest = blockIdx.x / batch_chunks;
    const int tb = rest % token_blocks, sg = rest / token_blocks;
    RopeWho w;
    w.slot = sg * ROPE_SLOTS + (lane >> 3);
    w.n = tb * WAVES + wave;
    w.b0 = bc * ROPE_BATCH_PER_WG;
    w.b1 = min(B, w.b0 + ROPE_BATCH_PER_WG);
    w.active = w.slot < 2 * H && w.n < N;
    return w;
}

// qkv[b N + n, slot j, pair p] <- [c -s; s c] (x0, x1) with (c, s) = table[n, p] (columns >= hd: +0, whatever they held).
// The v third is neither read nor written.
template <int HP>
__global__ __launch_bounds__(THREADS) void rope_fwd_kernel(uint16_t *__restrict__ qkv, const float *__restrict__ table, int B, int N,
                                                           int H, int hd, int token_blocks, int batch_chunks) {
    constexpr int VPL = HP / 64;
    const int sub = threadIdx.x & 7;
    const RopeWho w = rope_who(B, N, H, token_blocks, batch_chunks);
    if (!w.active) return;
    const size_t Da = size_t(H) * HP;
    float cs[VPL][8];
    rope_cs<VPL>(table, w.n, sub, hd, true, cs);
    uint16_t *base = qkv + size_t(w.slot) * HP;
    u32x4 xr[VPL], xn[VPL];
    auto load_row = [&](int b, u32x4 (&xq)[VPL]) __attribute__((always_inline)) {
        const size_t m = size_t(b) * N + w.n;
#pragma unroll
        for (int i = 0; i < VPL; i++) xq[i] = *reinterpret_cast<const u32x4 *>(base + m * 3 * Da + rope_col(sub, i));
    };
    load_row(w.b0, xr);
    for (int b = w.b0; b < w.b1; b++) {
        const bool more = b + 1 < w.b1;
        if (more) load_row(b + 1, xn);                          // the next row's loads fly while this one is rotated
        const size_t m = size_t(b) * N + w.n;
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            float x[8], o[8];
            unpack8(xr[i], x);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const bool real = rope_col(sub, i) + 2 * q < hd;    // hd is even: a pair is real or padding as a whole
                const float c = cs[i][2 * q], s = cs[i][2 * q + 1];
                o[2 * q] = real ? x[2 * q] * c - x[2 * q + 1] * s : 0.f;
                o[2 * q + 1] = real ? x[2 * q] * s + x[2 * q + 1] * c : 0.f;
            }
            *reinterpret_cast<u32x4 *>(base + m * 3 * Da + rope_col(sub, i)) = pack8(o);
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < VPL; i++) xr[i] = xn[i];
        }
    }
}

// dqkv[b N + n, slot j, pair p] <- [c s; -s c] (g0, g1), the transposed map (columns >= hd: +0, whatever they held, NaN
// included).  SUMS: per-workgroup partials [8 HP], the column sums of the STORED dq | dk of its 8 slots over its rows.
template <int HP, bool SUMS>
__global__ __launch_bounds__(THREADS) void rope_bwd_kernel(uint16_t *__restrict__ dqkv, const float *__restrict__ table,
                                                           float *__restrict__ partial, int B, int N, int H, int hd, int token_blocks,
                                                           int batch_chunks) {
    constexpr int VPL = HP / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 7, grp = lane >> 3;
    const RopeWho w = rope_who(B, N, H, token_blocks, batch_chunks);
    if (!SUMS && !w.active) return;
    const size_t Da = size_t(H) * HP;
    float cs[VPL][8], dc[VPL][8];
    rope_cs<VPL>(table, w.n, sub, hd, w.active, cs);
#pragma unroll
    for (int i = 0; i < VPL; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) dc[i][j] = 0.f;
    if (w.active) {
        uint16_t *base = dqkv + size_t(w.slot) * HP;
        u32x4 gr[VPL], gn[VPL];
        auto load_row = [&](int b, u32x4 (&gq)[VPL]) __attribute__((always_inline)) {
            const size_t m = size_t(b) * N + w.n;
#pragma unroll
            for (int i = 0; i < VPL; i++) gq[i] = *reinterpret_cast<const u32x4 *>(base + m * 3 * Da + rope_col(sub, i));
        };
        load_row(w.b0, gr);
        for (int b = w.b0; b < w.b1; b++) {
            const bool more = b + 1 < w.b1;
            if (more) load_row(b + 1, gn);
            const size_t m = size_t(b) * N + w.n;
#pragma unroll
            for (int i = 0; i < VPL; i++) {
                float g[8], o[8];
                unpack8(gr[i], g);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const bool real = rope_col(sub, i) + 2 * q < hd;    // a padded column's gradient may hold anything: selected out
                    const float c = cs[i][2 * q], s = cs[i][2 * q + 1];
                    o[2 * q] = real ? g[2 * q] * c + g[2 * q + 1] * s : 0.f;
                    o[2 * q + 1] = real ? g[2 * q + 1] * c - g[2 * q] * s : 0.f;
                }
                const u32x4 stored = pack8(o);
                *reinterpret_cast<u32x4 *>(base + m * 3 * Da + rope_col(sub, i)) = stored;
                if (SUMS) {
                    unpack8(stored, o);                          // the column sums are those of what dqkv holds: the rounded values
#pragma unroll
                    for (int j = 0; j < 8; j++) dc[i][j] += o[j];
                }
            }
            if (more) {
#pragma unroll
                for (int i = 0; i < VPL; i++) gr[i] = gn[i];
            }
        }
    }
    if (SUMS) {
        __shared__ __attribute__((aligned(16))) float red[WAVES][ROPE_SLOTS * HP];
#pragma unroll
        for (int i = 0; i < VPL; i++) {
            float *dst = &red[wave][grp * HP + rope_col(sub, i)];
            *reinterpret_cast<f32x4 *>(dst) = f32x4{dc[i][0], dc[i][1], dc[i][2], dc[i][3]};
            *reinterpret_cast<f32x4 *>(dst + 4) = f32x4{dc[i][4], dc[i][5], dc[i][6], dc[i][7]};
        }
        __syncthreads();
        float *out = partial + size_t(blockIdx.x) * (ROPE_SLOTS * HP);
        for (int c = threadIdx.x; c < ROPE_SLOTS * HP; c += THREADS) out[c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

// Second stage, one launch: the workgroups' partials in a fixed order -> colsum [2 H hp], the column sums of dq | dk, and, with
// vsum, colsum[2 H hp + i] = vsum[i]: the v third of the in_proj bias gradient, carried over from the attention backward.
__global__ __launch_bounds__(RED_THREADS) void rope_bwd_reduce(const float *__restrict__ partial, void *__restrict__ colsum,
                                                               int colsum_bf16, const float *__restrict__ vsum, int H, int hp,
                                                               int parts_per_group) {
    const int ld = ROPE_SLOTS * hp, Da2 = 2 * H * hp;
    const int ncb = Da2 / 16;
    const int b = blockIdx.x;
    if (b < ncb) {
        const int c = b * 16 + (threadIdx.x & 15);
        const int sg = c / ld, cc = c - sg * ld;
        const float t = reduce_partials16(partial + size_t(sg) * parts_per_group * ld, parts_per_group, ld, cc, true);
        if (threadIdx.x < 16) store_grad(colsum, c, t, colsum_bf16);
    } else {
        const int i = (b - ncb) * RED_THREADS + threadIdx.x;
        if (vsum && i < H * hp) store_grad(colsum, Da2 + i, vsum[i], colsum_bf16);
    }
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_rope_plan(int B, int N, int H, int hp, int32_t *out) {
    if (!out) return fail(SFCVIT_EINVAL, "rope_plan: null pointer (out)");
    const RopePlan p = rope_geometry(B, N, H, hp, "rope_plan");
    if (p.err) return fail(p.err, "%s", p.msg);
    out[0] = ROPE_WAVES;
    out[1] = ROPE_BATCH_PER_WG;
    out[2] = p.slot_groups;
    out[3] = p.blocks;
    out[4] = p.vpl;
    return SFCVIT_OK;
}

extern "C" int64_t sfcvit_rope_bwd_ws(int B, int N, int H, int hp) {
    const RopePlan p = rope_geometry(B, N, H, hp, "rope_bwd_ws");
    return p.err ? 0 : p.ws_bytes;
}

extern "C" int sfcvit_rope_fwd(void *qkv, const float *table, int B, int N, int H, int hd, int hp, void *stream) {
    const RopePlan p = rope_fwd_plan(qkv, table, B, N, H, hd, hp);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(p.blocks), block(THREADS);
    auto *qp = static_cast<uint16_t *>(qkv);
    g_rowwise.set("rope_fwd_kernel<%d>", hp);
#define ROPE_FWD(HP) hipLaunchKernelGGL(rope_fwd_kernel<HP>, grid, block, 0, s, qp, table, B, N, H, hd, p.token_blocks, p.batch_chunks)
    if (hp == 64) ROPE_FWD(64);
    else if (hp == 128) ROPE_FWD(128);
    else if (hp == 192) ROPE_FWD(192);
    else ROPE_FWD(256);
#undef ROPE_FWD
    return check_launch("rope_fwd");
}

extern "C" int sfcvit_rope_bwd(void *dqkv, const float *table, void *colsum, int colsum_is_bf16, const float *vsum, void *ws, int B,
                               int N, int H, int hd, int hp, void *stream) {
    const RopePlan p = rope_bwd_plan(dqkv, table, colsum, vsum, ws, B, N, H, hd, hp);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(p.blocks), block(THREADS);
    auto *dp = static_cast<uint16_t *>(dqkv);
    float *part = static_cast<float *>(ws);
    g_rowwise.set("rope_bwd_kernel<%d>", hp);
#define ROPE_BWD(HP)                                                                                                              \
    do {                                                                                                                          \
        if (p.sums)                                                                                                               \
            hipLaunchKernelGGL((rope_bwd_kernel<HP, true>), grid, block, 0, s, dp, table, part, B, N, H, hd, p.token_blocks,       \
                               p.batch_chunks);                                                                                   \
        else                                                                                                                      \
            hipLaunchKernelGGL((rope_bwd_kernel<HP, false>), grid, block, 0, s, dp, table, (float *)nullptr, B, N, H, hd,          \
                               p.token_blocks, p.batch_chunks);                                                                   \
    } while (0)
    if (hp == 64) ROPE_BWD(64);
    else if (hp == 128) ROPE_BWD(128);
    else if (hp == 192) ROPE_BWD(192);
    else ROPE_BWD(256);
#undef ROPE_BWD
    if (int rc = check_launch("rope_bwd")) return rc;
    if (!p.sums) return SFCVIT_OK;
    hipLaunchKernelGGL(rope_bwd_reduce, dim3(p.reduce_blocks), dim3(RED_THREADS), 0, s, part, colsum, colsum_is_bf16, vsum, H, hp,
                       p.token_blocks * p.batch_chunks);
    return check_launch("rope_bwd_reduce");
}
