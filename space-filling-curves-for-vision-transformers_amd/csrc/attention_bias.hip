// Self-attention core with a learned relative position bias per head for gfx950, head dim 64
// (sfcvit_attention_bias_fwd / _bwd in include/sfcvit.h).
//
// The masked kernels of attention_masked.hip -- same 64-row tiles, same LDS images, same MFMA orientations, same block-map
// ballots, same m_safe handling of a row that has seen no key, same fence rule -- with the additive term looked up instead
// of loaded:
//     s_ij = scale * q_i . k_j + table[h, index[i,j]]        (index[i,j] == -1: -inf, the pair is hidden)
// Head h's table row (T <= 4096 floats, 16 KiB) is staged in LDS once per workgroup.  The lane's 16 index values of a
// block are loaded BEFORE the staging and the MFMAs, with clamped addresses so that no load is exec-masked, and the
// bias is read from LDS after them without a branch in between.  The block map has two values: 0 = every entry of the
// block is -1 (skipped), anything else = visited; every visited block reads its index.
//
// Table gradient (attn_bias_bwd_table_kernel, attn_bias_chunk_sum_kernel, attn_bias_bucket_sum_kernel): no atomics.
//   1. A workgroup owns one visited 64 x 64 block of one head and a chunk of the batch.  Per image it recomputes S = Q K^T
//      and dP = dO V^T of its block (two of the backward's five MFMA groups), forms g = P (keep dP - delta) in fp32 and adds
//      it to 16 registers per lane, images in ascending order; then it stores the block with plain stores into the
//      workspace [chunks][H][visited blocks][64][64].  g never passes through bf16.
//   2. The chunks are summed element-wise, in ascending order, into chunk 0's slab.
//   3. One wave per dTable[h, t] walks the bucket's positions (the host's inverted index, ascending (i, j)): lane l takes
//      positions l, l + 64, ... in order, then a butterfly over the wave.  One writer per element, a fixed order.
// Every output element is written once after sums in a fixed order: two runs give the same bits.
#include "attention_bias.h"
#include "attention_common.h"
#include "common_host.h"

namespace sfcvit {
namespace {

using namespace attn;

static_assert(RELB_BLK == BLK, "the block map's granularity is the workgroup's tile");
static_assert(RELB_MAX_N / RELB_BLK <= 64, "one map entry per lane");
static_assert((RELB_MAX_N / RELB_BLK) * (RELB_MAX_N / RELB_BLK) <= THREADS, "one map entry per thread (block_ordinal)");

typedef __attribute__((ext_vector_type(4))) int i32x4;

// A workgroup's row (stride 1) or column (stride nb) of the block map as a wave-uniform 64-bit mask, read once before
// the block loop (attention_masked.hip, map_bits).  All 64 lanes must be active.
__device__ __forceinline__ uint64_t visit_bits(const uint8_t *map, int first, int stride, int nb, int lane) {
    const int e = lane < nb ? int(map[first + lane * stride]) : 0;
    return __ballot(e != 0);
}

// Four index values I[row][col0 .. col0 + 3] (col0 % 4 == 0) of a lane that holds one row and 4 consecutive columns.
// Addresses are clamped into the matrix: rows / columns >= N are don't-care (their scores are replaced or never stored).
// vec4: N % 4 == 0 (every row 16-byte aligned), one 16-byte load.
__device__ __forceinline__ i32x4 idx_row4(const int32_t *__restrict__ I, int N, int row, int col0, bool vec4) {
    const size_t base = size_t(min(row, N - 1)) * N;
    if (vec4) return *reinterpret_cast<const i32x4 *>(I + base + min(col0, N - 4));
    i32x4 v;
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = I[base + min(col0 + r, N - 1)];
    return v;
}
// Four index values I[row0 .. row0 + 3][col] of a lane that holds one column and 4 consecutive rows.
__device__ __forceinline__ i32x4 idx_col4(const int32_t *__restrict__ I, int N, int row0, int col) {
    const int c = min(col, N - 1);
    i32x4 v;
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = I[size_t(min(row0 + r, N - 1)) * N + c];
    return v;
}
// The bias of four index values from the staged table row: -1 -> -inf.  The LDS address is clamped into the row, so an
// index outside the contract reads a wrong bucket, never outside the array; the select is a v_cndmask, not a branch.
__device__ __forceinline__ f32x4 bias4(const float *tab, int T, const i32x4 &idx) {
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float t = tab[min(max(idx[r], 0), T - 1)];
        v[r] = idx[r] >= 0 ? t : -INFINITY;
    }
    return v;
}
// Head h's table row into LDS, by the whole workgroup; the caller's next barrier publishes it.
__device__ __forceinline__ void stage_table(float *tab, const float *__restrict__ table, int h, int T, int tid) {
    for (int t = tid; t < T; t += THREADS) tab[t] = table[size_t(h) * T + t];
}

// ---------------------------------------------------------------------------
// forward: one workgroup = 64 queries of one (b, h), walks row qb of the map
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void attn_bias_fwd_kernel(const sfcvit_attn_bias_args a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG_BYTES];
    __shared__ float tab[RELB_MAX_T];
    char *kimg = smem, *vimg = smem + IMG_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, T = a.T, D = a.H * HD, ld = 3 * D;
    const int nb = (N + BLK - 1) / BLK;
    const HeadView hv = head_view(a, b, h, HD);
    const uint16_t *qp = hv.qp, *kp = hv.kp, *vp = hv.vp;
    const int q0 = blockIdx.x * BLK + wave * 16;
    const int q = q0 + (lane & 15);
    const float scale = a.scale;
    const bool drop = a.dropout_p > 0.f;
    const uint32_t dth = drop_thresh(a.dropout_p);
    const float dsc = 1.f / (1.f - a.dropout_p);
    const uint32_t drk = mask_row_key(eff_seed(a.dropout_seed, a.seed_off), b, a.H, h, N, q);
    const uint64_t visit = visit_bits(a.block_map, int(blockIdx.x) * nb, 1, nb, lane);
    const bool vec4 = (N & 3) == 0;

    bf16x8 qf[2];
    qf[0] = global_frag(qp, ld, q0, N, 0, lane);
    qf[1] = global_frag(qp, ld, q0, N, 1, lane);
    stage_table(tab, a.table, h, T, tid);

    f32x4 o[4];
#pragma unroll
    for (int hf = 0; hf < 4; hf++) o[hf] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    for (int kb = 0; kb < nb; kb++) {
        if (!((visit >> kb) & 1)) continue;                 // uniform over the workgroup
        const int k0 = kb * BLK;
        i32x4 ix[4];
#pragma unroll
        for (int kf = 0; kf < 4; kf++) ix[kf] = idx_row4(a.index, N, q, k0 + 16 * kf + 4 * (lane >> 4), vec4);
        __syncthreads();
        stage64<false>(kimg, kp, ld, k0, N, tid);
        stage64<true>(vimg, vp, ld, k0, N, tid);
        __syncthreads();                                    // (the first one also publishes the table row)

        f32x4 s[4];
#pragma unroll
        for (int kf = 0; kf < 4; kf++) {
            s[kf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; kk++)
                s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag(kimg, 16 * kf, kk, lane), qf[kk], s[kf], 0, 0, 0);
        }
        // s[kf][r] = S^T[key = k0 + 16kf + 4g + r][q = lane & 15]
        float mb = -INFINITY;
#pragma unroll
        for (int kf = 0; kf < 4; kf++) {
            const f32x4 bs = bias4(tab, T, ix[kf]);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int key = k0 + 16 * kf + 4 * (lane >> 4) + r;
                s[kf][r] = key < N ? s[kf][r] * scale + bs[r] : -INFINITY;
                mb = fmaxf(mb, s[kf][r]);
            }
        }
        mb = group_max(mb);
        const float m_new = fmaxf(m_run, mb);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;      // a row that has seen no key yet: every exp below is 0
        const float alpha = __expf(m_run - m_safe);
        float ls = 0.f;
#pragma unroll
        for (int kf = 0; kf < 4; kf++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                s[kf][r] = __expf(s[kf][r] - m_safe);
                ls += s[kf][r];
            }
        l_run = l_run * alpha + ls;      // the normaliser uses the un-dropped probabilities
        m_run = m_new;
        if (drop) {
#pragma unroll
            for (int kf = 0; kf < 4; kf++) {
                float keep[4];
                drop_keep4(drk, k0 + 16 * kf + 4 * (lane >> 4), dth, dsc, keep);
#pragma unroll
                for (int r = 0; r < 4; r++) s[kf][r] *= keep[r];
            }
        }
#pragma unroll
        for (int hf = 0; hf < 4; hf++) o[hf] *= alpha;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const bf16x8 pf = pack_frag(s[2 * c], s[2 * c + 1]);
#pragma unroll
            for (int hf = 0; hf < 4; hf++)
                o[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<true>(vimg, 32 * c, 32 * c + 16, 16 * hf, lane), pf,
                                                                o[hf], 0, 0, 0);
        }
        mfma_fence();                    // the skip branch of the next block must not sit between these MFMAs and a reader of o
    }
    mfma_fence();
    const float l_tot = group_sum(l_run);
    uint16_t *out = hv.rows(a.out);
    store_rows(out, D, q, q < N, o, 1.f / l_tot, lane);
    if (q < N && lane < 16) a.lse[bh_row(b, a.H, h, N, q)] = m_run + __logf(l_tot);
}

// ---------------------------------------------------------------------------
// delta[b,h,q] = sum_d dO[b,q,h,d] * O[b,q,h,d]   (as attention_masked.hip's attn_masked_delta_kernel)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void attn_bias_delta_kernel(const uint16_t *__restrict__ dout,
                                                                  const uint16_t *__restrict__ out, float *__restrict__ delta,
                                                                  int B, int N, int H) {
    // one 8-lane group per (b, q, h): 8 lanes x 8 elements
    const int64_t grp = (int64_t(blockIdx.x) * THREADS + threadIdx.x) >> 3;
    const int sub = threadIdx.x & 7;
    const int64_t total = int64_t(B) * N * H;
    float s = 0.f;
    if (grp < total) {
        const size_t off = size_t(grp) * HD + sub * 8;   // [B, N, H, hd] is contiguous
        const u32x4 x = *reinterpret_cast<const u32x4 *>(dout + off), y = *reinterpret_cast<const u32x4 *>(out + off);
#pragma unroll
        for (int i = 0; i < 4; i++)
            s += bf2f(uint16_t(x[i])) * bf2f(uint16_t(y[i])) + bf2f(uint16_t(x[i] >> 16)) * bf2f(uint16_t(y[i] >> 16));
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (grp < total && sub == 0) {
        const int64_t bq = grp / H;
        const int hh = int(grp % H);
        const int64_t bb = bq / N, qq = bq % N;
        delta[(bb * H + hh) * N + qq] = s;
    }
}

// ---------------------------------------------------------------------------
// backward: dK, dV (one workgroup = 64 keys of one (b, h), walks column kb of the map; wave = 16 keys)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void attn_bias_bwd_kv_kernel(const sfcvit_attn_bias_args a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG_BYTES + 2 * BLK * 4];
    __shared__ float tab[RELB_MAX_T];
    char *qimg = smem, *doimg = smem + IMG_BYTES;
    float *lse_s = reinterpret_cast<float *>(smem + 2 * IMG_BYTES), *del_s = lse_s + BLK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, T = a.T, D = a.H * HD, ld = 3 * D;
    const int nb = (N + BLK - 1) / BLK;
    const HeadView hv = head_view(a, b, h, HD);
    const uint16_t *qp = hv.qp, *kp = hv.kp, *vp = hv.vp;
    const uint16_t *dop = hv.rows(a.dout);
    const float *lse = a.lse + bh_row(b, a.H, h, N, 0), *del = a.delta + bh_row(b, a.H, h, N, 0);
    const int key0 = blockIdx.x * BLK + wave * 16;
    const float scale = a.scale;
    const bool drop = a.dropout_p > 0.f;
    const uint32_t dth = drop_thresh(a.dropout_p);
    const float dsc = 1.f / (1.f - a.dropout_p);
    const uint32_t seed = eff_seed(a.dropout_seed, a.seed_off);
    const int key = key0 + (lane & 15);
    const uint64_t visit = visit_bits(a.block_map, int(blockIdx.x), nb, nb, lane);

    bf16x8 kf[2], vf[2];
#pragma unroll
    for (int kk = 0; kk < 2; kk++) {
        kf[kk] = global_frag(kp, ld, key0, N, kk, lane);
        vf[kk] = global_frag(vp, ld, key0, N, kk, lane);
    }
    stage_table(tab, a.table, h, T, tid);
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int hf = 0; hf < 4; hf++) dk[hf] = dv[hf] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int qb = 0; qb < nb; qb++) {
        if (!((visit >> qb) & 1)) continue;                 // uniform over the workgroup
        const int q0 = qb * BLK;
        i32x4 ix[4];                                        // ix[qf][r] = I[q0 + 16qf + 4g + r][key]
#pragma unroll
        for (int qf = 0; qf < 4; qf++) ix[qf] = idx_col4(a.index, N, q0 + 16 * qf + 4 * (lane >> 4), key);
        __syncthreads();
        stage64<false>(qimg, qp, ld, q0, N, tid);
        stage64<false>(doimg, dop, D, q0, N, tid);
        if (tid < BLK) {
            lse_s[tid] = q0 + tid < N ? lse[q0 + tid] : 0.f;
            del_s[tid] = q0 + tid < N ? del[q0 + tid] : 0.f;
        }
        __syncthreads();                                    // (the first one also publishes the table row)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            f32x4 p[2], ds[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int qf = 2 * c + t;
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 2; kk++) {
                    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag(qimg, 16 * qf, kk, lane), kf[kk], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag(doimg, 16 * qf, kk, lane), vf[kk], dp, 0, 0, 0);
                }
                // s[r] = S[q = q0 + 16qf + 4g + r][key]; a hidden pair has bias -inf and P = exp(-inf) = 0.  Queries >= N have
                // Q = dO = 0 rows: whatever P they get multiplies zeros.
                const f32x4 bs = bias4(tab, T, ix[qf]);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int ql = 16 * qf + 4 * (lane >> 4) + r;
                    const float pv = __expf(s[r] * scale + bs[r] - lse_s[ql]);
                    float keep = 1.f;
                    if (drop) {
                        bool k0b, k1b;
                        drop_keep2(mask_row_key(seed, b, a.H, h, N, q0 + ql), uint32_t(key >> 1), dth, k0b, k1b);
                        keep = ((key & 1) ? k1b : k0b) ? dsc : 0.f;
                    }
                    p[t][r] = pv * keep;                                   // dropped probabilities feed dV
                    ds[t][r] = pv * (dp[r] * keep - del_s[ql]) * scale;
                }
            }
            const bf16x8 pf = pack_frag(p[0], p[1]), dsf = pack_frag(ds[0], ds[1]);
#pragma unroll
            for (int hf = 0; hf < 4; hf++) {
                dv[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<false>(doimg, 32 * c, 32 * c + 16, 16 * hf, lane), pf,
                                                                 dv[hf], 0, 0, 0);
                dk[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<false>(qimg, 32 * c, 32 * c + 16, 16 * hf, lane), dsf,
                                                                 dk[hf], 0, 0, 0);
            }
        }
        mfma_fence();
    }
    // a key block no query sees arrives here with dk = dv = 0 and writes them: dqkv is not initialised by the caller
    uint16_t *dbase = hv.packed(a.dqkv);
    mfma_fence();
    store_rows(dbase + D, ld, key, key < N, dk, 1.f, lane);
    store_rows(dbase + 2 * D, ld, key, key < N, dv, 1.f, lane);
}

// ---------------------------------------------------------------------------
// backward: dQ (one workgroup = 64 queries of one (b, h), walks row qb of the map; wave = 16 queries)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void attn_bias_bwd_q_kernel(const sfcvit_attn_bias_args a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG_BYTES];
    __shared__ float tab[RELB_MAX_T];
    char *kimg = smem, *vimg = smem + IMG_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, T = a.T, D = a.H * HD, ld = 3 * D;
    const int nb = (N + BLK - 1) / BLK;
    const HeadView hv = head_view(a, b, h, HD);
    const uint16_t *qp = hv.qp, *kp = hv.kp, *vp = hv.vp;
    const uint16_t *dop = hv.rows(a.dout);
    const int q0 = blockIdx.x * BLK + wave * 16;
    const int q = q0 + (lane & 15);
    const float scale = a.scale;
    const float lse_q = q < N ? a.lse[bh_row(b, a.H, h, N, q)] : 0.f;
    const float del_q = q < N ? a.delta[bh_row(b, a.H, h, N, q)] : 0.f;
    const bool drop = a.dropout_p > 0.f;
    const uint32_t dth = drop_thresh(a.dropout_p);
    const float dsc = 1.f / (1.f - a.dropout_p);
    const uint32_t drk = mask_row_key(eff_seed(a.dropout_seed, a.seed_off), b, a.H, h, N, q);
    const uint64_t visit = visit_bits(a.block_map, int(blockIdx.x) * nb, 1, nb, lane);
    const bool vec4 = (N & 3) == 0;

    bf16x8 qf[2], dof[2];
#pragma unroll
    for (int kk = 0; kk < 2; kk++) {
        qf[kk] = global_frag(qp, ld, q0, N, kk, lane);
        dof[kk] = global_frag(dop, D, q0, N, kk, lane);
    }
    stage_table(tab, a.table, h, T, tid);
    f32x4 dq[4];
#pragma unroll
    for (int hf = 0; hf < 4; hf++) dq[hf] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < nb; kb++) {
        if (!((visit >> kb) & 1)) continue;                 // uniform over the workgroup
        const int k0 = kb * BLK;
        i32x4 ix[4];
#pragma unroll
        for (int kfi = 0; kfi < 4; kfi++) ix[kfi] = idx_row4(a.index, N, q, k0 + 16 * kfi + 4 * (lane >> 4), vec4);
        __syncthreads();
        stage64<false>(kimg, kp, ld, k0, N, tid);
        stage64<false>(vimg, vp, ld, k0, N, tid);
        __syncthreads();                                    // (the first one also publishes the table row)
        // lse - bias per key: exp(s scale - (lse - bias)) = exp(s scale + bias - lse); a hidden key has lse - bias = +inf and P = 0
        f32x4 lm[4];
#pragma unroll
        for (int kfi = 0; kfi < 4; kfi++) lm[kfi] = splat4(lse_q) - bias4(tab, T, ix[kfi]);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            f32x4 ds[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int kfi = 2 * c + t;
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 2; kk++) {
                    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag(kimg, 16 * kfi, kk, lane), qf[kk], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag(vimg, 16 * kfi, kk, lane), dof[kk], dp, 0, 0, 0);
                }
                // s[r] = S^T[key = k0 + 16kfi + 4g + r][q]; keys >= N have K = V = 0 and add nothing
                float keep[4] = {1.f, 1.f, 1.f, 1.f};
                if (drop) drop_keep4(drk, k0 + 16 * kfi + 4 * (lane >> 4), dth, dsc, keep);
                ds[t] = ds_from_scores<false>(s, dp, lm[kfi], splat4(del_q), keep, scale, scale);
            }
            const bf16x8 dsf = pack_frag(ds[0], ds[1]);
#pragma unroll
            for (int hf = 0; hf < 4; hf++)
                dq[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<false>(kimg, 32 * c, 32 * c + 16, 16 * hf, lane), dsf,
                                                                 dq[hf], 0, 0, 0);
        }
        mfma_fence();
    }
    uint16_t *dbase = hv.packed(a.dqkv);
    mfma_fence();
    store_rows(dbase, ld, q, q < N, dq, 1.f, lane);
}

// ---------------------------------------------------------------------------
// table gradient
// ---------------------------------------------------------------------------
// The ordinal of map entry `tid` among the non-zero entries (row-major), for every thread of the workgroup at once:
// one ballot per wave, the waves' counts through LDS.  nz: the thread's own entry is non-zero.  Contains a barrier.
__device__ __forceinline__ int block_ordinal(const uint8_t *__restrict__ map, int nbnb, int tid, int *wave_tot, bool &nz) {
    nz = tid < nbnb && map[min(tid, nbnb - 1)] != 0;
    const uint64_t bal = __ballot(nz);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int ord = __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < THREADS / 64; w++) ord += w < wave ? wave_tot[w] : 0;
    return ord;
}

// grid (visited blocks, H, chunks).  The dQ kernel's orientation: wave = 16 queries of the block, the block's 64 keys
// staged per image; lane (g, i) holds g[q = 16 wave + i][key = 16 kf + 4 g + r] in acc[kf][r].
__global__ __launch_bounds__(THREADS) void attn_bias_bwd_table_kernel(const sfcvit_attn_bias_args a, int per) {
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG_BYTES];
    __shared__ float tab[RELB_MAX_T];
    __shared__ int wave_tot[THREADS / 64];
    __shared__ int mine;
    char *kimg = smem, *vimg = smem + IMG_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.y, N = a.N, T = a.T, D = a.H * HD, ld = 3 * D;
    const int nb = (N + BLK - 1) / BLK;
    const int vb = blockIdx.x, VB = a.visited_blocks;
    if (tid == 0) mine = -1;
    bool nz;
    const int ord = block_ordinal(a.block_map, nb * nb, tid, wave_tot, nz);     // (its barrier orders `mine = -1` first)
    if (nz && ord == vb) mine = tid;
    stage_table(tab, a.table, h, T, tid);
    __syncthreads();
    const int blk = mine;
    if (blk < 0) return;                                    // uniform: a map with fewer visited blocks than the caller said
    const int qb = blk / nb, kb = blk - qb * nb;
    const int q0 = qb * BLK + wave * 16, k0 = kb * BLK;
    const int q = q0 + (lane & 15);
    const float scale = a.scale;
    const bool drop = a.dropout_p > 0.f;
    const uint32_t dth = drop_thresh(a.dropout_p);
    const float dsc = 1.f / (1.f - a.dropout_p);
    const uint32_t seed = eff_seed(a.dropout_seed, a.seed_off);
    const bool vec4 = (N & 3) == 0;

    // the bias of the lane's 16 pairs, the same for every image; pairs outside the sequence count as hidden
    f32x4 bs[4];
#pragma unroll
    for (int kf = 0; kf < 4; kf++) {
        const int key0 = k0 + 16 * kf + 4 * (lane >> 4);
        bs[kf] = bias4(tab, T, idx_row4(a.index, N, q, key0, vec4));
#pragma unroll
        for (int r = 0; r < 4; r++) bs[kf][r] = (q < N && key0 + r < N) ? bs[kf][r] : -INFINITY;
    }
    f32x4 acc[4];
#pragma unroll
    for (int kf = 0; kf < 4; kf++) acc[kf] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int b0 = int(blockIdx.z) * per, b1 = min(b0 + per, int(a.B));
    for (int b = b0; b < b1; b++) {
        const HeadView hv = head_view(a, b, h, HD);
        const uint16_t *dop = hv.rows(a.dout);
        bf16x8 qf[2], dof[2];
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
            qf[kk] = global_frag(hv.qp, ld, q0, N, kk, lane);
            dof[kk] = global_frag(dop, D, q0, N, kk, lane);
        }
        const float lse_q = q < N ? a.lse[bh_row(b, a.H, h, N, q)] : 0.f;
        const float del_q = q < N ? a.delta[bh_row(b, a.H, h, N, q)] : 0.f;
        const uint32_t drk = mask_row_key(seed, b, a.H, h, N, q);
        __syncthreads();
        stage64<false>(kimg, hv.kp, ld, k0, N, tid);
        stage64<false>(vimg, hv.vp, ld, k0, N, tid);
        __syncthreads();
#pragma unroll
        for (int kf = 0; kf < 4; kf++) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; kk++) {
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag(kimg, 16 * kf, kk, lane), qf[kk], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag(vimg, 16 * kf, kk, lane), dof[kk], dp, 0, 0, 0);
            }
            float keep[4] = {1.f, 1.f, 1.f, 1.f};
            if (drop) drop_keep4(drk, k0 + 16 * kf + 4 * (lane >> 4), dth, dsc, keep);
            // P (keep dP - delta), fp32 throughout: the bias sits after the scale, so no scale factor here
            acc[kf] += ds_from_scores<false>(s, dp, splat4(lse_q) - bs[kf], splat4(del_q), keep, scale, 1.f);
        }
        mfma_fence();
    }
    float *ws = static_cast<float *>(a.workspace) + ((size_t(blockIdx.z) * a.H + h) * VB + vb) * size_t(BLK * BLK);
    const int ql = wave * 16 + (lane & 15);
#pragma unroll
    for (int kf = 0; kf < 4; kf++) *reinterpret_cast<f32x4 *>(ws + ql * BLK + 16 * kf + 4 * (lane >> 4)) = acc[kf];
}

// ws[0][e] = sum over chunks c, ascending, of ws[c][e]; e counts 16-byte vectors of one chunk's slab.
__global__ __launch_bounds__(THREADS) void attn_bias_chunk_sum_kernel(float *__restrict__ ws, int64_t vecs, int chunks) {
    const int64_t e = int64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (e >= vecs) return;
    f32x4 *p = reinterpret_cast<f32x4 *>(ws) + e;
    f32x4 s = p[0];
    for (int c = 1; c < chunks; c++) s += p[int64_t(c) * vecs];
    p[0] = s;
}

// grid (ceil(T / 4), H): one wave per dTable[h, t], over the bucket's positions in the order of the inverted index.
__global__ __launch_bounds__(THREADS) void attn_bias_bucket_sum_kernel(const sfcvit_attn_bias_args a) {
    __shared__ int wave_tot[THREADS / 64];
    __shared__ int ord_s[THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.y, N = a.N, T = a.T, VB = a.visited_blocks;
    const int nb = (N + BLK - 1) / BLK;
    bool nz;
    const int ord = block_ordinal(a.block_map, nb * nb, tid, wave_tot, nz);
    ord_s[tid] = nz && ord < VB ? ord : -1;
    __syncthreads();
    const int t = int(blockIdx.x) * (THREADS / 64) + wave;
    if (t >= T) return;                                     // uniform over the wave; no barrier follows
    const float *ws = static_cast<const float *>(a.workspace) + size_t(h) * VB * size_t(BLK * BLK);
    const int first = a.offsets[t], last = a.offsets[t + 1];
    float s = 0.f;
    for (int k = first + lane; k < last; k += 64) {
        const int p = a.positions[k];
        const int i = p / N, j = p - i * N;
        const int o = uint32_t(p) < uint32_t(N * N) ? ord_s[(i >> 6) * nb + (j >> 6)] : -1;
        if (o >= 0) s += ws[size_t(o) * (BLK * BLK) + (i & 63) * BLK + (j & 63)];
    }
    s = wave_sum(s);
    if (lane == 0) a.dtable[size_t(h) * T + t] = s;
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_attention_bias_fwd(const sfcvit_attn_bias_args *a, void *stream) {
    if (const int rc = attn_bias_check(a, false, "attention_bias_fwd")) return rc;
    g_attn.set("attn_bias_fwd_kernel");
    hipLaunchKernelGGL(attn_bias_fwd_kernel, dim3(bias_blocks(a->N), a->H, a->B), dim3(attn::THREADS), 0,
                       static_cast<hipStream_t>(stream), *a);
    return check_launch("attention_bias_fwd");
}

extern "C" int sfcvit_attention_bias_bwd(const sfcvit_attn_bias_args *a, void *stream) {
    if (const int rc = attn_bias_check(a, true, "attention_bias_bwd")) return rc;
    if (a->colsum_out && (!a->colsum_part || a->colsum_part_bytes < sfcvit_attention_colsum_workspace(a->B, a->N, a->H, a->hd)))
        return fail(SFCVIT_EINVAL, "attention_bias_bwd: colsum_out needs colsum_part of sfcvit_attention_colsum_workspace bytes");
    g_attn.set("attn_bias_bwd_kv_kernel");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = SFCVIT_OK;
    const int64_t groups = int64_t(a->B) * a->N * a->H;
    hipLaunchKernelGGL(attn_bias_delta_kernel, dim3(unsigned((groups * 8 + attn::THREADS - 1) / attn::THREADS)), dim3(attn::THREADS), 0, s,
                       static_cast<const uint16_t *>(a->dout), static_cast<const uint16_t *>(a->out), a->delta, a->B, a->N, a->H);
    if ((rc = check_launch("attention_bias_bwd delta"))) return rc;
    const dim3 grid(bias_blocks(a->N), a->H, a->B);
    hipLaunchKernelGGL(attn_bias_bwd_kv_kernel, grid, dim3(attn::THREADS), 0, s, *a);
    if ((rc = check_launch("attention_bias_bwd kv"))) return rc;
    hipLaunchKernelGGL(attn_bias_bwd_q_kernel, grid, dim3(attn::THREADS), 0, s, *a);
    if ((rc = check_launch("attention_bias_bwd q"))) return rc;
    if (a->dtable) {                                        // NULL: a frozen table
        const BiasChunks ch = bias_chunks(a->B, a->H, a->visited_blocks);
        hipLaunchKernelGGL(attn_bias_bwd_table_kernel, dim3(a->visited_blocks, a->H, ch.chunks), dim3(attn::THREADS), 0, s, *a, ch.per);
        if ((rc = check_launch("attention_bias_bwd table"))) return rc;
        if (ch.chunks > 1) {
            const int64_t vecs = int64_t(a->H) * a->visited_blocks * (attn::BLK * attn::BLK / 4);
            hipLaunchKernelGGL(attn_bias_chunk_sum_kernel, dim3(unsigned((vecs + attn::THREADS - 1) / attn::THREADS)), dim3(attn::THREADS), 0, s,
                               static_cast<float *>(a->workspace), vecs, ch.chunks);
            if ((rc = check_launch("attention_bias_bwd chunk sum"))) return rc;
        }
        hipLaunchKernelGGL(attn_bias_bucket_sum_kernel, dim3((a->T + attn::THREADS / 64 - 1) / (attn::THREADS / 64), a->H), dim3(attn::THREADS), 0, s, *a);
        if ((rc = check_launch("attention_bias_bwd bucket sum"))) return rc;
    }
    if (!a->colsum_out) return SFCVIT_OK;
    const int D3 = 3 * a->H * a->hd;
    return sfcvit_colsum(a->dqkv, a->B * a->N, D3, D3, a->colsum_out, a->colsum_bf16, a->colsum_part, a->colsum_part_bytes, stream);
}
