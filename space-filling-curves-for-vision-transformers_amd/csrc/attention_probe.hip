// Attention maps and attention-distance statistics (sfcvit_attention_probs / sfcvit_attention_stats), any N, head dims
// 64 S (S = 1..4).
//
// Both kernels rebuild P[i, j] = exp(scale q_i . k_j - lse_i) from the packed projection and the forward's lse, streaming
// 64-key blocks of K through one LDS block of S slices (the images, fragment addressing and MFMA layouts of
// attention_wide_stream.hip's forward: a wave holds 16 queries, lane (g, i) gets S^T[key 16 kf + 4 g + r][query i]).  The
// row constant rides in the MFMA chain: the accumulators start at -lse_i / scale, so the chain leaves
// x = q_i . k_j - lse_i / scale and P = exp2(scale log2(e) x) needs no subtraction, no row maximum and no second pass;
// lse_i - s_ij, the entropy's factor, is -scale x.
//   statistics  workgroup = 64 queries of one (batch, head); loop over the key blocks; four running sums per lane, added over
//               the keys in ascending block order, then over the four 16-lane groups that share a query (group_sum); lanes
//               0..15 store.  [B, H, N] floats out, N x N is never written.
//   map         workgroup = one 64 x 64 tile of one (batch, head) map -- or, head_mean, of the batch item's mean map: the heads
//               loop runs inside the workgroup, the tile is summed in fp32 registers in head order and multiplied by 1 / H once.
// Keys >= N (zero rows of the image) are selected to P = 0; query rows >= N are computed on zero fragments and never
// stored.  No atomics: every output element belongs to one lane (group).  Inputs are only read.
// MFMA rule (device_common.h): the score chain ends in mfma_fence(); the tail masks are selects.
#include "attention_common.h"
#include "common_host.h"

namespace sfcvit {
namespace {

using namespace attn;

// x[kf][r] = q . k - lse / scale for this wave's 16 queries (fragments qf) against the 64 keys staged in kimg
template <int S>
__device__ __forceinline__ void probe_scores(f32x4 (&x)[4], const char *kimg, const bf16x8 (&qf)[S][2], float c0, const LaneOff &lo) {
#pragma unroll
    for (int kf = 0; kf < 4; kf++) x[kf] = f32x4{c0, c0, c0, c0};
    static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
        constexpr int sl = decltype(ic)::value;
#pragma unroll
        for (int kf = 0; kf < 4; kf++)
#pragma unroll
            for (int kk = 0; kk < 2; kk++)
                x[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc_frag_at(kimg + sl * IMG_BYTES, 16 * kf, lo.k[kk]), qf[sl][kk], x[kf], 0, 0, 0);
    });
    mfma_fence();
}

template <int S>
__global__ __launch_bounds__(THREADS) void attn_probe_stats_kernel(const sfcvit_attn_probe_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *kimg = smem;
    float *prow = reinterpret_cast<float *>(smem + S * IMG_BYTES), *pcol = prow + BLK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, N = a.N, hd = 64 * S, D = a.H * hd, ld = 3 * D;
    const HeadView hv = head_view(a, b, h, hd);
    const uint16_t *qp = hv.qp, *kp = hv.kp;
    const int q0 = blockIdx.x * BLK + wave * 16, q = q0 + (lane & 15);
    const size_t row = bh_row(b, a.H, h, N, 0);
    const float lse_q = q < N ? a.lse[row + q] : 0.f;
    const float c0 = -lse_q / a.scale, c2 = a.scale * LOG2E;
    const bool has_pos = a.pos != nullptr;
    const float qr = has_pos && q < N ? a.pos[2 * size_t(q)] : 0.f, qc = has_pos && q < N ? a.pos[2 * size_t(q) + 1] : 0.f;
    const LaneOff lo = lane_offsets(lane);

    bf16x8 qf[S][2];
    static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
        constexpr int sl = decltype(ic)::value;
#pragma unroll
        for (int kk = 0; kk < 2; kk++) qf[sl][kk] = global_frag(qp + 64 * sl, ld, q0, N, kk, lane);
    });
    float dist = 0.f, seq = 0.f, ent = 0.f, mass = 0.f;

    for (int k0 = 0; k0 < N; k0 += BLK) {
        __syncthreads();
        static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
            constexpr int sl = decltype(ic)::value;
            stage64<false>(kimg + sl * IMG_BYTES, kp + 64 * sl, ld, k0, N, tid);
        });
        if (tid < BLK) {                                         // positions of the block's keys (0 without pos, or past N)
            const int key = k0 + tid;
            const bool ok = has_pos && key < N;
            prow[tid] = ok ? a.pos[2 * size_t(key)] : 0.f;
            pcol[tid] = ok ? a.pos[2 * size_t(key) + 1] : 0.f;
        }
        __syncthreads();

        f32x4 x[4];
        probe_scores<S>(x, kimg, qf, c0, lo);
#pragma unroll
        for (int kf = 0; kf < 4; kf++) {
            const int kb = 16 * kf + 4 * g;
            const f32x4 kr = *reinterpret_cast<const f32x4 *>(prow + kb), kc = *reinterpret_cast<const f32x4 *>(pcol + kb);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int key = k0 + kb + r;
                const float p = key < N ? fast_exp2(x[kf][r] * c2) : 0.f;
                const float dr = qr - kr[r], dc = qc - kc[r];
                mass += p;
                ent += p * x[kf][r];
                seq += p * fabsf(float(q - key));
                dist += p * __builtin_amdgcn_sqrtf(dr * dr + dc * dc);
            }
        }
        mfma_fence();
    }
    dist = group_sum(dist);
    seq = group_sum(seq);
    ent = group_sum(ent) * -a.scale;                             // sum_j P (lse - s) = -scale sum_j P x
    mass = group_sum(mass);
    if (q < N && lane < 16) {
        if (a.dist_rows) a.dist_rows[row + q] = dist;
        if (a.seq_rows) a.seq_rows[row + q] = seq;
        if (a.ent_rows) a.ent_rows[row + q] = ent;
        if (a.mass_rows) a.mass_rows[row + q] = mass;
    }
}

// attention_common.h's store_rows for a tile whose columns may end early: acc[kf][r] = X[row = lane & 15][col 16 kf + 4 g + r]
// as bf16, two 16-byte stores per lane (the permlane16_swap pairing described there; all 64 lanes must be active), a store
// only where its 8 columns lie below `ncols` (a multiple of 8, or >= 64).
__device__ __forceinline__ void store_tile_bf16(uint16_t *__restrict__ dst, bool row_ok, int ncols, const f32x4 (&acc)[4], int lane) {
    uint32_t p[4][2];
#pragma unroll
    for (int kf = 0; kf < 4; kf++) {
        p[kf][0] = pack2bf(acc[kf][0], acc[kf][1]);
        p[kf][1] = pack2bf(acc[kf][2], acc[kf][3]);
    }
    const int g = lane >> 4;
#pragma unroll
    for (int pr = 0; pr < 2; pr++) {
        const auto lo = __builtin_amdgcn_permlane16_swap(p[2 * pr][0], p[2 * pr + 1][0], false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap(p[2 * pr][1], p[2 * pr + 1][1], false, false);
        const u32x4 o = {lo[0], hi[0], lo[1], hi[1]};
        const int col = 16 * (2 * pr + (g & 1)) + 8 * (g >> 1);
        if (row_ok && col < ncols) *reinterpret_cast<u32x4 *>(dst + col) = o;
    }
}

// grid (query block, key block, z): z = batch item (MEAN: heads 0 .. H - 1 summed here) or (batch item, head)
template <int S, bool MEAN>
__global__ __launch_bounds__(THREADS) void attn_probe_map_kernel(const sfcvit_attn_probe_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *kimg = smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int z = blockIdx.z, N = a.N, hd = 64 * S, D = a.H * hd, ld = 3 * D;
    const int b = MEAN ? z : z / a.H, h_lo = MEAN ? 0 : z % a.H, h_hi = MEAN ? a.H : h_lo + 1;
    const int q0 = blockIdx.x * BLK + wave * 16, q = q0 + (lane & 15), k0 = blockIdx.y * BLK;
    const float c2 = a.scale * LOG2E;
    const LaneOff lo = lane_offsets(lane);

    f32x4 acc[4];
#pragma unroll
    for (int kf = 0; kf < 4; kf++) acc[kf] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int h = h_lo; h < h_hi; h++) {
        const uint16_t *base = static_cast<const uint16_t *>(a.qkv) + size_t(b) * N * ld + h * hd;
        const uint16_t *qp = base, *kp = base + D;
        const float lse_q = q < N ? a.lse[bh_row(b, a.H, h, N, 0) + q] : 0.f;
        bf16x8 qf[S][2];
        static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
            constexpr int sl = decltype(ic)::value;
#pragma unroll
            for (int kk = 0; kk < 2; kk++) qf[sl][kk] = global_frag(qp + 64 * sl, ld, q0, N, kk, lane);
        });
        __syncthreads();
        static_for<0, S>([&](auto ic) __attribute__((always_inline)) {
            constexpr int sl = decltype(ic)::value;
            stage64<false>(kimg + sl * IMG_BYTES, kp + 64 * sl, ld, k0, N, tid);
        });
        __syncthreads();
        f32x4 x[4];
        probe_scores<S>(x, kimg, qf, -lse_q / a.scale, lo);
#pragma unroll
        for (int kf = 0; kf < 4; kf++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float p = k0 + 16 * kf + 4 * g + r < N ? fast_exp2(x[kf][r] * c2) : 0.f;
                acc[kf][r] = MEAN ? acc[kf][r] + p : p;
            }
        mfma_fence();
    }
    if (MEAN) {
        const float inv_h = 1.f / float(a.H);
#pragma unroll
        for (int kf = 0; kf < 4; kf++) acc[kf] *= inv_h;
    }

    // row q of map z, columns k0 .. k0 + 63 (as far as they exist)
    const bool row_ok = q < N;
    const size_t off = (size_t(z) * N + size_t(row_ok ? q : 0)) * size_t(N) + k0;
    const int ncols = N - k0;
    if (a.probs_is_bf16) {
        uint16_t *dst = static_cast<uint16_t *>(a.probs) + off;
        if (N % 8 == 0) {
            store_tile_bf16(dst, row_ok, ncols, acc, lane);
        } else {
#pragma unroll
            for (int kf = 0; kf < 4; kf++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int col = 16 * kf + 4 * g + r;
                    if (row_ok && col < ncols) dst[col] = f2bf(acc[kf][r]);
                }
        }
    } else {
        float *dst = static_cast<float *>(a.probs) + off;
        if (N % 4 == 0) {
#pragma unroll
            for (int kf = 0; kf < 4; kf++) {
                const int col = 16 * kf + 4 * g;
                if (row_ok && col < ncols) *reinterpret_cast<f32x4 *>(dst + col) = acc[kf];
            }
        } else {
#pragma unroll
            for (int kf = 0; kf < 4; kf++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int col = 16 * kf + 4 * g + r;
                    if (row_ok && col < ncols) dst[col] = acc[kf][r];
                }
        }
    }
}

template <int S>
int launch_stats(const ProbePlan &p, const sfcvit_attn_probe_args &a, hipStream_t s) {
    hipLaunchKernelGGL(attn_probe_stats_kernel<S>, dim3(p.blocks, a.H, p.grid_z), dim3(THREADS), p.lds, s, a);
    return check_launch("attention_stats");
}

template <int S>
int launch_map(const ProbePlan &p, const sfcvit_attn_probe_args &a, hipStream_t s) {
    const dim3 grid(p.blocks, p.blocks, p.grid_z);
    if (p.mean) hipLaunchKernelGGL((attn_probe_map_kernel<S, true>), grid, dim3(THREADS), p.lds, s, a);
    else hipLaunchKernelGGL((attn_probe_map_kernel<S, false>), grid, dim3(THREADS), p.lds, s, a);
    return check_launch("attention_probs");
}

int attention_probe(const sfcvit_attn_probe_args *a, void *stream, bool stats) {
    if (!a) return fail(SFCVIT_EINVAL, "%s: null pointer", stats ? "attention_stats" : "attention_probs");
    const ProbePlan p = attn_probe_plan(*a, stats);
    if (p.err) return fail(p.err, "%s", p.msg);
    note_attn_kernel(p);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (p.inst) {
    case 1: return stats ? launch_stats<1>(p, *a, s) : launch_map<1>(p, *a, s);
    case 2: return stats ? launch_stats<2>(p, *a, s) : launch_map<2>(p, *a, s);
    case 3: return stats ? launch_stats<3>(p, *a, s) : launch_map<3>(p, *a, s);
    default: return stats ? launch_stats<4>(p, *a, s) : launch_map<4>(p, *a, s);
    }
}

}  // namespace
}  // namespace sfcvit

extern "C" int sfcvit_attention_probs(const sfcvit_attn_probe_args *a, void *stream) { return sfcvit::attention_probe(a, stream, false); }
extern "C" int sfcvit_attention_stats(const sfcvit_attn_probe_args *a, void *stream) { return sfcvit::attention_probe(a, stream, true); }
