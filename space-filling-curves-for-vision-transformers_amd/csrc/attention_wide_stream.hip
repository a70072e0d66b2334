// Streaming attention for head dims 128 / 192 / 256 (= 64 S, S = 2..4), any N.
//
// attention.hip's tiled kernels with the head dimension cut into S slices of 64 columns, the way attention_wide.hip cut
// attention_seq.hip's (one LDS image per slice: attention_wide.hip's header); scores sum over the slices, outputs are per slice.
// LDS is two 64-row blocks of S slices whatever N is -- 32 / 48 / 64 KiB (+ 768 B of row data in the dK / dV kernel) --
// so two workgroups fit on a CU at S = 4.
//   forward         workgroup = 64 queries of one (batch, head), wave = 16; loop over 64-key blocks of K | V, online softmax
//   dK / dV kernel  workgroup = 64 keys, wave = 16; loop over 64-query blocks of Q | dO (+ lse, delta, mask row keys)
//   dQ kernel       workgroup = 64 queries, wave = 16; loop over 64-key blocks of K | V
// delta comes from attention.hip's attn_delta_kernel, launched first by sfcvit_attention_bwd.  Every output element is
// written once, by one lane, after a loop in a fixed order: no atomics, bitwise reproducible.
// MFMA rule (device_common.h): each batch of score MFMAs is followed by mfma_fence() before the softmax / dropout code
// (which branches on the dropout switch) reads it, and each loop iteration ends with one; the key / query tail masks are
// selects, not branches.
#include "attention_common.h"
#include "common_host.h"

namespace sfcvit {
namespace {

using namespace attn;

template <int S>
__global__ __launch_bounds__(THREADS) void attn_wide_stream_fwd_kernel(const sfcvit_attn_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *kimg = smem, *vimg = smem + S * IMG_BYTES;            // slice sl of a block at + sl * IMG_BYTES
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, hd = 64 * S, D = a.H * hd, ld = 3 * D;
    const HeadView hv = head_view(a, b, h, hd);
    const uint16_t *qp = hv.qp, *kp = hv.kp, *vp = hv.vp;
    const int q0 = blockIdx.x * BLK + wave * 16;
    const float scale = a.scale;
    const bool drop = a.dropout_p > 0.f;
    const uint32_t dth = drop_thresh(a.dropout_p);
    const float dsc = 1.f / (1.f - a.dropout_p);
    const uint64_t row0 = bh_row(b, a.H, h, N, 0);
    const uint32_t drk = mask_row_key(eff_seed(a.dropout_seed, a.seed_off), row0 + uint64_t(q0 + (lane & 15)));
    const LaneOff lo = lane_offsets(lane);

    bf16x8 qf[S][2];
    f32x4 o[S][4];
    static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
        constexpr int sl = decltype(ic)::value;
#pragma unroll
        for (int kk = 0; kk < 2; kk++) qf[sl][kk] = global_frag(qp + 64 * sl, ld, q0, N, kk, lane);
#pragma unroll
        for (int hf = 0; hf < 4; hf++) o[sl][hf] = f32x4{0.f, 0.f, 0.f, 0.f};
    });
    float m_run = -INFINITY, l_run = 0.f;

    for (int k0 = 0; k0 < N; k0 += BLK) {
        __syncthreads();
        static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
            constexpr int sl = decltype(ic)::value;
            stage64<false>(kimg + sl * IMG_BYTES, kp + 64 * sl, ld, k0, N, tid);
            stage64<true>(vimg + sl * IMG_BYTES, vp + 64 * sl, ld, k0, N, tid);
        });
        __syncthreads();

        f32x4 s[4];
#pragma unroll
        for (int kf = 0; kf < 4; kf++) s[kf] = f32x4{0.f, 0.f, 0.f, 0.f};
        static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
            constexpr int sl = decltype(ic)::value;
#pragma unroll
            for (int kf = 0; kf < 4; kf++)
#pragma unroll
                for (int kk = 0; kk < 2; kk++)
                    s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag_at(kimg + sl * IMG_BYTES, 16 * kf, lo.k[kk]), qf[sl][kk], s[kf], 0, 0, 0);
        });
        mfma_fence();
        // s[kf][r] = S^T[key = k0 + 16kf + 4g + r][q = lane & 15]; keys >= N (zero rows of the image) -> -inf
        float mb = -INFINITY;
#pragma unroll
        for (int kf = 0; kf < 4; kf++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int key = k0 + 16 * kf + 4 * (lane >> 4) + r;
                s[kf][r] = key < N ? s[kf][r] * scale : -INFINITY;
                mb = fmaxf(mb, s[kf][r]);
            }
        mb = group_max(mb);                                      // finite: every block holds a key < N
        const float m_new = fmaxf(m_run, mb);
        const float alpha = __expf(m_run - m_new);
        float ls = 0.f;
#pragma unroll
        for (int kf = 0; kf < 4; kf++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                s[kf][r] = __expf(s[kf][r] - m_new);
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
        const bf16x8 pf[2] = {pack_frag(s[0], s[1]), pack_frag(s[2], s[3])};
        static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
            constexpr int sl = decltype(ic)::value;
#pragma unroll
            for (int hf = 0; hf < 4; hf++) {
                o[sl][hf] *= alpha;
#pragma unroll
                for (int c = 0; c < 2; c++)
                    o[sl][hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag_at(vimg + sl * IMG_BYTES, 32 * c, lo.tv[hf]), pf[c], o[sl][hf], 0, 0, 0);
            }
        });
        mfma_fence();
    }
    const float l_tot = group_sum(l_run);
    const int q = q0 + (lane & 15);
    uint16_t *out = hv.rows(a.out);
    static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
        constexpr int sl = decltype(ic)::value;
        store_rows(out + 64 * sl, D, q, q < N, o[sl], 1.f / l_tot, lane);
    });
    if (q < N && lane < 16) a.lse[row0 + q] = m_run + __logf(l_tot);
}

// dK, dV: one workgroup = 64 keys of one (b, h), wave = 16 keys; K / V fragments of all slices stay in registers.
template <int S>
__global__ __launch_bounds__(THREADS) void attn_wide_stream_bwd_kv_kernel(const sfcvit_attn_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *qimg = smem, *doimg = smem + S * IMG_BYTES;
    float *lse_s = reinterpret_cast<float *>(smem + 2 * S * IMG_BYTES), *del_s = lse_s + BLK;
    uint32_t *rkey_s = reinterpret_cast<uint32_t *>(del_s + BLK);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, hd = 64 * S, D = a.H * hd, ld = 3 * D;
    const HeadView hv = head_view(a, b, h, hd);
    const uint16_t *qp = hv.qp, *kp = hv.kp, *vp = hv.vp;
    const uint16_t *dop = hv.rows(a.dout);
    const float *lse = a.lse + bh_row(b, a.H, h, N, 0), *del = a.delta + bh_row(b, a.H, h, N, 0);
    const int key0 = blockIdx.x * BLK + wave * 16, key = key0 + (lane & 15);
    const float scale = a.scale, c2 = a.scale * LOG2E;
    const bool drop = a.dropout_p > 0.f;
    const uint32_t dth = drop_thresh(a.dropout_p);
    const float dsc = 1.f / (1.f - a.dropout_p);
    const uint32_t seed = eff_seed(a.dropout_seed, a.seed_off);
    const LaneOff lo = lane_offsets(lane);

    bf16x8 kf[S][2], vf[S][2];
    f32x4 dk[S][4], dv[S][4];
    static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
        constexpr int sl = decltype(ic)::value;
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
            kf[sl][kk] = global_frag(kp + 64 * sl, ld, key0, N, kk, lane);
            vf[sl][kk] = global_frag(vp + 64 * sl, ld, key0, N, kk, lane);
        }
#pragma unroll
        for (int hf = 0; hf < 4; hf++) dk[sl][hf] = dv[sl][hf] = f32x4{0.f, 0.f, 0.f, 0.f};
    });

    for (int q0 = 0; q0 < N; q0 += BLK) {
        __syncthreads();
        static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
            constexpr int sl = decltype(ic)::value;
            stage64<false>(qimg + sl * IMG_BYTES, qp + 64 * sl, ld, q0, N, tid);
            stage64<false>(doimg + sl * IMG_BYTES, dop + 64 * sl, D, q0, N, tid);
        });
        if (tid < BLK) {                                         // queries >= N: lse = +inf gives P = 0
            const int q = q0 + tid;
            lse_s[tid] = lse_log2(lse, q, q < N, INFINITY);
            del_s[tid] = q < N ? del[q] : 0.f;
            rkey_s[tid] = mask_row_key(seed, b, a.H, h, N, q);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 2; c++) {
            f32x4 s[2], dp[2];
#pragma unroll
            for (int t = 0; t < 2; t++) s[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
                constexpr int sl = decltype(ic)::value;
#pragma unroll
                for (int t = 0; t < 2; t++)
#pragma unroll
                    for (int kk = 0; kk < 2; kk++) {
                        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag_at(qimg + sl * IMG_BYTES, 16 * (2 * c + t), lo.k[kk]), kf[sl][kk], s[t], 0, 0, 0);
                        dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag_at(doimg + sl * IMG_BYTES, 16 * (2 * c + t), lo.k[kk]), vf[sl][kk], dp[t], 0, 0, 0);
                    }
            });
            mfma_fence();
            // s[t][r] = S[q = q0 + 16(2c + t) + 4g + r][key]
            f32x4 p[2], ds[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int ql0 = 16 * (2 * c + t) + 4 * (lane >> 4);
                const f32x4 lse4 = *reinterpret_cast<const f32x4 *>(lse_s + ql0);
                const f32x4 del4 = *reinterpret_cast<const f32x4 *>(del_s + ql0);
                const u32x4 rk4 = *reinterpret_cast<const u32x4 *>(rkey_s + ql0);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float pv = fast_exp2(s[t][r] * c2 - lse4[r]);
                    float keep = 1.f;
                    if (drop) {
                        bool k0b, k1b;
                        drop_keep2(rk4[r], uint32_t(key >> 1), dth, k0b, k1b);
                        keep = ((key & 1) ? k1b : k0b) ? dsc : 0.f;
                    }
                    p[t][r] = pv * keep;                         // dropped probabilities feed dV
                    ds[t][r] = pv * (dp[t][r] * keep - del4[r]) * scale;
                }
            }
            const bf16x8 pf = pack_frag(p[0], p[1]), dsf = pack_frag(ds[0], ds[1]);
            static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
                constexpr int sl = decltype(ic)::value;
#pragma unroll
                for (int hf = 0; hf < 4; hf++) {
                    dv[sl][hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag_at(doimg + sl * IMG_BYTES, 32 * c, lo.t[hf]), pf, dv[sl][hf], 0, 0, 0);
                    dk[sl][hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag_at(qimg + sl * IMG_BYTES, 32 * c, lo.t[hf]), dsf, dk[sl][hf], 0, 0, 0);
                }
            });
        }
        mfma_fence();
    }
    uint16_t *dbase = hv.packed(a.dqkv);
    static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
        constexpr int sl = decltype(ic)::value;
        store_rows(dbase + D + 64 * sl, ld, key, key < N, dk[sl], 1.f, lane);
        store_rows(dbase + 2 * D + 64 * sl, ld, key, key < N, dv[sl], 1.f, lane);
    });
}

// dQ: one workgroup = 64 queries of one (b, h), wave = 16 queries; Q / dO fragments of all slices stay in registers.
template <int S>
__global__ __launch_bounds__(THREADS) void attn_wide_stream_bwd_q_kernel(const sfcvit_attn_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *kimg = smem, *vimg = smem + S * IMG_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, hd = 64 * S, D = a.H * hd, ld = 3 * D;
    const HeadView hv = head_view(a, b, h, hd);
    const uint16_t *qp = hv.qp, *kp = hv.kp, *vp = hv.vp;
    const uint16_t *dop = hv.rows(a.dout);
    const int q0 = blockIdx.x * BLK + wave * 16, q = q0 + (lane & 15);
    const float scale = a.scale, c2 = a.scale * LOG2E;
    const float lse_q = q < N ? a.lse[bh_row(b, a.H, h, N, q)] * LOG2E : 0.f;
    const float del_q = q < N ? a.delta[bh_row(b, a.H, h, N, q)] : 0.f;
    const bool drop = a.dropout_p > 0.f;
    const uint32_t dth = drop_thresh(a.dropout_p);
    const float dsc = 1.f / (1.f - a.dropout_p);
    const uint32_t drk = mask_row_key(eff_seed(a.dropout_seed, a.seed_off), b, a.H, h, N, q);
    const LaneOff lo = lane_offsets(lane);

    bf16x8 qf[S][2], dof[S][2];
    f32x4 dq[S][4];
    static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
        constexpr int sl = decltype(ic)::value;
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
            qf[sl][kk] = global_frag(qp + 64 * sl, ld, q0, N, kk, lane);
            dof[sl][kk] = global_frag(dop + 64 * sl, D, q0, N, kk, lane);
        }
#pragma unroll
        for (int hf = 0; hf < 4; hf++) dq[sl][hf] = f32x4{0.f, 0.f, 0.f, 0.f};
    });

    for (int k0 = 0; k0 < N; k0 += BLK) {
        __syncthreads();
        static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
            constexpr int sl = decltype(ic)::value;
            stage64<false>(kimg + sl * IMG_BYTES, kp + 64 * sl, ld, k0, N, tid);
            stage64<false>(vimg + sl * IMG_BYTES, vp + 64 * sl, ld, k0, N, tid);
        });
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 2; c++) {
            f32x4 s[2], dp[2];
#pragma unroll
            for (int t = 0; t < 2; t++) s[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
                constexpr int sl = decltype(ic)::value;
#pragma unroll
                for (int t = 0; t < 2; t++)
#pragma unroll
                    for (int kk = 0; kk < 2; kk++) {
                        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag_at(kimg + sl * IMG_BYTES, 16 * (2 * c + t), lo.k[kk]), qf[sl][kk], s[t], 0, 0, 0);
                        dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag_at(vimg + sl * IMG_BYTES, 16 * (2 * c + t), lo.k[kk]), dof[sl][kk], dp[t], 0, 0, 0);
                    }
            });
            mfma_fence();
            // s[t][r] = S^T[key = k0 + 16(2c + t) + 4g + r][q]; keys >= N -> dS = 0
            f32x4 ds[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int kb = k0 + 16 * (2 * c + t) + 4 * (lane >> 4);
                float keep[4] = {1.f, 1.f, 1.f, 1.f};
                if (drop) drop_keep4(drk, kb, dth, dsc, keep);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float v = fast_exp2(s[t][r] * c2 - lse_q) * (dp[t][r] * keep[r] - del_q) * scale;
                    ds[t][r] = kb + r < N ? v : 0.f;
                }
            }
            const bf16x8 dsf = pack_frag(ds[0], ds[1]);
            static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
                constexpr int sl = decltype(ic)::value;
#pragma unroll
                for (int hf = 0; hf < 4; hf++)
                    dq[sl][hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag_at(kimg + sl * IMG_BYTES, 32 * c, lo.t[hf]), dsf, dq[sl][hf], 0, 0, 0);
            });
        }
        mfma_fence();
    }
    uint16_t *dbase = hv.packed(a.dqkv);
    static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
        constexpr int sl = decltype(ic)::value;
        store_rows(dbase + 64 * sl, ld, q, q < N, dq[sl], 1.f, lane);
    });
}

template <int S>
int launch_fwd(const AttnPlan &p, const sfcvit_attn_args &a, hipStream_t s) {
    if (int rc = raise_lds_limit(reinterpret_cast<const void *>(&attn_wide_stream_fwd_kernel<S>), ATTN_LDS_LIMIT, "attention_wide_stream attribute")) return rc;
    hipLaunchKernelGGL(attn_wide_stream_fwd_kernel<S>, dim3(p.grid, a.H, a.B), dim3(THREADS), p.lds, s, a);
    return check_launch("attention_wide_stream_fwd");
}

template <int S>
int launch_bwd(const AttnPlan &p, const sfcvit_attn_args &a, hipStream_t s) {
    for (const void *k : {reinterpret_cast<const void *>(&attn_wide_stream_bwd_kv_kernel<S>), reinterpret_cast<const void *>(&attn_wide_stream_bwd_q_kernel<S>)})
        if (int rc = raise_lds_limit(k, ATTN_LDS_LIMIT, "attention_wide_stream attribute")) return rc;
    const dim3 grid(p.grid, a.H, a.B);
    hipLaunchKernelGGL(attn_wide_stream_bwd_kv_kernel<S>, grid, dim3(THREADS), p.lds, s, a);
    if (int rc = check_launch("attention_wide_stream_bwd kv")) return rc;
    hipLaunchKernelGGL(attn_wide_stream_bwd_q_kernel<S>, grid, dim3(THREADS), p.lds2, s, a);
    return check_launch("attention_wide_stream_bwd q");
}

}  // namespace

// The plan's streaming head-dim 128 / 192 / 256 kernels (dispatch.cpp; S = p.inst = hd / 64).
int attn_wide_stream_fwd(const AttnPlan &p, const sfcvit_attn_args &a, hipStream_t s) {
    if (p.inst == 2) return launch_fwd<2>(p, a, s);
    if (p.inst == 3) return launch_fwd<3>(p, a, s);
    return launch_fwd<4>(p, a, s);
}

int attn_wide_stream_bwd(const AttnPlan &p, const sfcvit_attn_args &a, hipStream_t s) {
    if (p.inst == 2) return launch_bwd<2>(p, a, s);
    if (p.inst == 3) return launch_bwd<3>(p, a, s);
    return launch_bwd<4>(p, a, s);
}

}  // namespace sfcvit
