// Masked / windowed self-attention core for gfx950, head dim 64 (sfcvit_attention_masked_fwd / _bwd in include/sfcvit.h).
//
// The tiled kernels of attention.hip -- same 64-row tiles, same LDS images, same MFMA orientations (that file's header)
// -- with an additive fp32 mask M [N, N] and a block map [nb][nb] (attention_masked.h):
//     s_ij = scale * q_i . k_j + M_ij
// "for every 64-row block" becomes "for every block whose map entry is non-zero".  The map's granularity is the
// workgroup's tile, so all four waves of a workgroup walk the same block list and the barriers around the staging stay
// uniform (the entries are ballot bits in scalar registers: a scalar branch, never an exec mask).  On a MIXED block the lane's 16
// mask values are loaded BEFORE the staging and the MFMAs -- with clamped indices, so no load is exec-masked -- and added
// after them without a branch in between (fence rule, device_common.h); on a ZERO block the mask is not read.
//
// What a mask adds to the online softmax: in a visited block a query row may see no key at all (its running maximum is
// still -inf).  exp(m_run - m_new) and exp(s - m_new) would then be exp(-inf + inf) = NaN, so the subtrahend is
// max-or-zero (m_safe): exp(-inf - 0) = 0 and the row simply carries on empty.  Every row < N has a finite entry
// somewhere (precondition, enforced on the host), so its final normaliser is positive.
//
// No atomics; every output element is written once, sums run in block order: two runs give the same bits.
#include "attention_common.h"
#include "attention_masked.h"
#include "common_host.h"

namespace sfcvit {
namespace {

using namespace attn;

static_assert(MASK_BLK == BLK, "the block map's granularity is the workgroup's tile");

// A workgroup's row (stride 1) or column (stride nb) of the block map as two wave-uniform 64-bit masks: nb <= 64, so one
// entry per lane and one ballot each.  Read once, before the block loop: a load inside the loop sits in front of every
// block's branch with its full latency (measured: 5-28 % of the forward, 3-22 % of the backward).
// Every wave reads the same entries, so the masks agree across the workgroup.  All 64 lanes must be active.
static_assert(MASK_MAX_N / MASK_BLK <= 64, "one map entry per lane");
struct BlockBits { uint64_t visit, mixed; };
__device__ __forceinline__ BlockBits map_bits(const uint8_t *map, int first, int stride, int nb, int lane) {
    const int e = lane < nb ? int(map[first + lane * stride]) : int(MASK_SKIP);
    return BlockBits{__ballot(e != MASK_SKIP), __ballot(e == MASK_MIXED)};
}

// Four mask values M[row][col0 .. col0 + 3] (col0 % 4 == 0) of a lane that holds one row and 4 consecutive columns.
// Indices are clamped into the matrix: rows / columns >= N are don't-care (their scores are replaced or never stored).
// vec4: N % 4 == 0 (every row 16-byte aligned), one 16-byte load.
__device__ __forceinline__ f32x4 mask_row4(const float *__restrict__ M, int N, int row, int col0, bool vec4) {
    const size_t base = size_t(min(row, N - 1)) * N;
    if (vec4) return *reinterpret_cast<const f32x4 *>(M + base + min(col0, N - 4));
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = M[base + min(col0 + r, N - 1)];
    return v;
}
// Four mask values M[row0 .. row0 + 3][col] of a lane that holds one column and 4 consecutive rows.
__device__ __forceinline__ f32x4 mask_col4(const float *__restrict__ M, int N, int row0, int col) {
    const int c = min(col, N - 1);
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = M[size_t(min(row0 + r, N - 1)) * N + c];
    return v;
}

// ---------------------------------------------------------------------------
// forward: one workgroup = 64 queries of one (b, h), walks row qb of the map
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void attn_masked_fwd_kernel(const sfcvit_attn_mask_args a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG_BYTES];
    char *kimg = smem, *vimg = smem + IMG_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, D = a.H * HD, ld = 3 * D;
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
    const BlockBits bits = map_bits(a.block_map, int(blockIdx.x) * nb, 1, nb, lane);
    const bool vec4 = (N & 3) == 0;

    bf16x8 qf[2];
    qf[0] = global_frag(qp, ld, q0, N, 0, lane);
    qf[1] = global_frag(qp, ld, q0, N, 1, lane);

    f32x4 o[4];
#pragma unroll
    for (int hf = 0; hf < 4; hf++) o[hf] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    for (int kb = 0; kb < nb; kb++) {
        if (!((bits.visit >> kb) & 1)) continue;            // uniform over the workgroup
        const bool mixed = (bits.mixed >> kb) & 1;
        const int k0 = kb * BLK;
        f32x4 mk[4];
#pragma unroll
        for (int kf = 0; kf < 4; kf++) mk[kf] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (mixed) {
#pragma unroll
            for (int kf = 0; kf < 4; kf++) mk[kf] = mask_row4(a.mask, N, q, k0 + 16 * kf + 4 * (lane >> 4), vec4);
        }
        __syncthreads();
        stage64<false>(kimg, kp, ld, k0, N, tid);
        stage64<true>(vimg, vp, ld, k0, N, tid);
        __syncthreads();

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
        for (int kf = 0; kf < 4; kf++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int key = k0 + 16 * kf + 4 * (lane >> 4) + r;
                s[kf][r] = key < N ? s[kf][r] * scale + mk[kf][r] : -INFINITY;
                mb = fmaxf(mb, s[kf][r]);
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
// delta[b,h,q] = sum_d dO[b,q,h,d] * O[b,q,h,d]   (as attention.hip's attn_delta_kernel, head dim 64)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void attn_masked_delta_kernel(const uint16_t *__restrict__ dout,
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
__global__ __launch_bounds__(THREADS) void attn_masked_bwd_kv_kernel(const sfcvit_attn_mask_args a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG_BYTES + 2 * BLK * 4];
    char *qimg = smem, *doimg = smem + IMG_BYTES;
    float *lse_s = reinterpret_cast<float *>(smem + 2 * IMG_BYTES), *del_s = lse_s + BLK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, D = a.H * HD, ld = 3 * D;
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
    const BlockBits bits = map_bits(a.block_map, int(blockIdx.x), nb, nb, lane);

    bf16x8 kf[2], vf[2];
#pragma unroll
    for (int kk = 0; kk < 2; kk++) {
        kf[kk] = global_frag(kp, ld, key0, N, kk, lane);
        vf[kk] = global_frag(vp, ld, key0, N, kk, lane);
    }
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int hf = 0; hf < 4; hf++) dk[hf] = dv[hf] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int qb = 0; qb < nb; qb++) {
        if (!((bits.visit >> qb) & 1)) continue;            // uniform over the workgroup
        const bool mixed = (bits.mixed >> qb) & 1;
        const int q0 = qb * BLK;
        f32x4 mk[4];                                        // mk[qf][r] = M[q0 + 16qf + 4g + r][key]
#pragma unroll
        for (int qf = 0; qf < 4; qf++) mk[qf] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (mixed) {
#pragma unroll
            for (int qf = 0; qf < 4; qf++) mk[qf] = mask_col4(a.mask, N, q0 + 16 * qf + 4 * (lane >> 4), key);
        }
        __syncthreads();
        stage64<false>(qimg, qp, ld, q0, N, tid);
        stage64<false>(doimg, dop, D, q0, N, tid);
        if (tid < BLK) {
            lse_s[tid] = q0 + tid < N ? lse[q0 + tid] : 0.f;
            del_s[tid] = q0 + tid < N ? del[q0 + tid] : 0.f;
        }
        __syncthreads();
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
                // s[r] = S[q = q0 + 16qf + 4g + r][key]; a hidden pair has M = -inf and P = exp(-inf) = 0.  Queries >= N have
                // Q = dO = 0 rows: whatever P they get multiplies zeros.
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int ql = 16 * qf + 4 * (lane >> 4) + r;
                    const float pv = __expf(s[r] * scale + mk[qf][r] - lse_s[ql]);
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
__global__ __launch_bounds__(THREADS) void attn_masked_bwd_q_kernel(const sfcvit_attn_mask_args a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG_BYTES];
    char *kimg = smem, *vimg = smem + IMG_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, D = a.H * HD, ld = 3 * D;
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
    const BlockBits bits = map_bits(a.block_map, int(blockIdx.x) * nb, 1, nb, lane);
    const bool vec4 = (N & 3) == 0;

    bf16x8 qf[2], dof[2];
#pragma unroll
    for (int kk = 0; kk < 2; kk++) {
        qf[kk] = global_frag(qp, ld, q0, N, kk, lane);
        dof[kk] = global_frag(dop, D, q0, N, kk, lane);
    }
    f32x4 dq[4];
#pragma unroll
    for (int hf = 0; hf < 4; hf++) dq[hf] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < nb; kb++) {
        if (!((bits.visit >> kb) & 1)) continue;            // uniform over the workgroup
        const bool mixed = (bits.mixed >> kb) & 1;
        const int k0 = kb * BLK;
        // lse - M per key: exp(s scale - (lse - M)) = exp(s scale + M - lse); a hidden key has lse - M = +inf and P = 0
        f32x4 lm[4];
#pragma unroll
        for (int kfi = 0; kfi < 4; kfi++) lm[kfi] = splat4(lse_q);
        if (mixed) {
#pragma unroll
            for (int kfi = 0; kfi < 4; kfi++) lm[kfi] -= mask_row4(a.mask, N, q, k0 + 16 * kfi + 4 * (lane >> 4), vec4);
        }
        __syncthreads();
        stage64<false>(kimg, kp, ld, k0, N, tid);
        stage64<false>(vimg, vp, ld, k0, N, tid);
        __syncthreads();
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

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_attention_masked_fwd(const sfcvit_attn_mask_args *a, void *stream) {
    if (const int rc = attn_masked_check(a, false, "attention_masked_fwd")) return rc;
    g_attn.set("attn_masked_fwd_kernel");
    hipLaunchKernelGGL(attn_masked_fwd_kernel, dim3(mask_blocks(a->N), a->H, a->B), dim3(attn::THREADS), 0,
                       static_cast<hipStream_t>(stream), *a);
    return check_launch("attention_masked_fwd");
}

extern "C" int sfcvit_attention_masked_bwd(const sfcvit_attn_mask_args *a, void *stream) {
    if (const int rc = attn_masked_check(a, true, "attention_masked_bwd")) return rc;
    if (a->colsum_out && (!a->colsum_part || a->colsum_part_bytes < sfcvit_attention_colsum_workspace(a->B, a->N, a->H, a->hd)))
        return fail(SFCVIT_EINVAL, "attention_masked_bwd: colsum_out needs colsum_part of sfcvit_attention_colsum_workspace bytes");
    g_attn.set("attn_masked_bwd_kv_kernel");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = SFCVIT_OK;
    const int64_t groups = int64_t(a->B) * a->N * a->H;
    hipLaunchKernelGGL(attn_masked_delta_kernel, dim3(unsigned((groups * 8 + attn::THREADS - 1) / attn::THREADS)), dim3(attn::THREADS), 0, s,
                       static_cast<const uint16_t *>(a->dout), static_cast<const uint16_t *>(a->out), a->delta, a->B, a->N, a->H);
    if ((rc = check_launch("attention_masked_bwd delta"))) return rc;
    const dim3 grid(mask_blocks(a->N), a->H, a->B);
    hipLaunchKernelGGL(attn_masked_bwd_kv_kernel, grid, dim3(attn::THREADS), 0, s, *a);
    if ((rc = check_launch("attention_masked_bwd kv"))) return rc;
    hipLaunchKernelGGL(attn_masked_bwd_q_kernel, grid, dim3(attn::THREADS), 0, s, *a);
    if ((rc = check_launch("attention_masked_bwd q"))) return rc;
    if (!a->colsum_out) return SFCVIT_OK;
    const int D3 = 3 * a->H * a->hd;
    return sfcvit_colsum(a->dqkv, a->B * a->N, D3, D3, a->colsum_out, a->colsum_bf16, a->colsum_part, a->colsum_part_bytes, stream);
}
