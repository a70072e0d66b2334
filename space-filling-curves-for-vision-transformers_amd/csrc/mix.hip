// Device-side MixUp / CutMix beside the gather (include/sfcvit.h, "MixUp / CutMix on the device"):
//   sfcvit_mix_images    the mixed image batch in one pass, for the tokenizers that never materialise tokens
//   sfcvit_soft_ce_pair  soft-target cross entropy on the label pair (y_a, y_b) + the lam-weighted hit count per row
// The mixing gather kernels themselves live with the gather in patch_embed.hip; mix.h is what the three share.
#include "common_host.h"
#include "mix.h"
#include "tokenizer.h"

namespace sfcvit {
namespace {

constexpr int THREADS = MIX_THREADS, WAVES = MIX_WAVES;

// out[b, c, p] = mix(x[b, c, p], x[perm[b], c, p]): a thread owns V consecutive pixels of a plane (V = 4: one 16-byte
// load of each image and one 16-byte store; V = 1 when H * W is not a multiple of 4) and walks the B * C planes with the
// stride of grid.y, so the pixel's row and column are worked out once.  CutMix reads the partner only where a vector
// touches the box.
template <int V>
__global__ __launch_bounds__(THREADS) void mix_images_kernel(const float *__restrict__ x, const int32_t *__restrict__ perm,
                                                             const uint32_t *__restrict__ rec, float *__restrict__ out, int B, int C,
                                                             int HW, int W) {
    const int p = (blockIdx.x * THREADS + threadIdx.x) * V;
    if (p >= HW) return;
    const MixRec mr = load_mix_rec(rec);
    bool inside[V];
    bool partner = mr.mode == 1u;
#pragma unroll
    for (int e = 0; e < V; e++) {
        const int row = (p + e) / W, col = (p + e) - row * W;
        inside[e] = in_box(mr, row, col);
        partner = partner || (mr.mode == 2u && inside[e]);
    }
    for (int plane = blockIdx.y; plane < B * C; plane += gridDim.y) {
        const int b = plane / C, c = plane - b * C;
        const size_t off = size_t(plane) * HW + p;
        if constexpr (V == 4) {
            f32x4 a = *reinterpret_cast<const f32x4 *>(x + off);
            if (partner) {
                const f32x4 q = *reinterpret_cast<const f32x4 *>(x + (size_t(mix_partner(perm, b, B)) * C + c) * HW + p);
#pragma unroll
                for (int e = 0; e < 4; e++) a[e] = mix_px(mr, a[e], q[e], inside[e]);
            }
            *reinterpret_cast<f32x4 *>(out + off) = a;
        } else {
            float a = x[off];
            if (partner) a = mix_px(mr, a, x[(size_t(mix_partner(perm, b, B)) * C + c) * HW + p], inside[0]);
            out[off] = a;
        }
    }
}

// One wave per row, the max / sum-of-exponentials loop of soft_ce_kernel (rowwise.hip) -- the same lse -- with the target
// sums collapsed to the two labels.  A label outside [0, C) is a label without a target: it contributes nothing to the
// loss, the gradient or the hit count, and nothing is read or written through it (checked per lane, no host sync).
__global__ __launch_bounds__(THREADS) void soft_ce_pair_kernel(const uint16_t *__restrict__ logits, const int64_t *__restrict__ y_a,
                                                               const int64_t *__restrict__ y_b, const uint32_t *__restrict__ rec,
                                                               float *__restrict__ loss_rows, uint16_t *__restrict__ dlogits,
                                                               float *__restrict__ hit_rows, int B, int C, int ld, float gscale) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (row >= B) return;
    const MixRec mr = load_mix_rec(rec);
    const float lam = mr.mode ? mr.lam : 1.f, oml = mr.mode ? mr.oml : 0.f;
    const int64_t ya64 = y_a[row], yb64 = y_b[row];
    const bool va = ya64 >= 0 && ya64 < C, vb = yb64 >= 0 && yb64 < C;
    const int ya = va ? int(ya64) : -1, yb = vb ? int(yb64) : -1;
    const uint16_t *l = logits + size_t(row) * ld;
    float mx = -INFINITY;
    int am = 0;                                           // argmax, the lowest index winning ties (torch.argmax)
    for (int c = lane; c < C; c += 64) {
        const float z = bf2f(l[c]);
        if (z > mx) { mx = z; am = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
    }
    // se as soft_ce_kernel forms it, and beside it the same sum without the term of y_a / of y_b: 1 - softmax at a target
    // column is then sa / se instead of 1 - exp(z - lse), which loses every digit when the model is sure of that label
    float se = 0.f, sa = 0.f, sb = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float e = __expf(bf2f(l[c]) - mx);
        se += e;
        sa += c == ya ? 0.f : e;
        sb += c == yb ? 0.f : e;
    }
    se = wave_sum(se);
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    const float lse = mx + __logf(se);
    // the dense row lam * onehot(y_a) + (1 - lam) * onehot(y_b) holds fadd(lam, 1 - lam) where the labels coincide
    const float both = mixup_px(lam, 1.f, oml, 1.f);
    const float ta = va ? (ya == yb ? both : lam) : 0.f;
    const float tb = (vb && ya != yb) ? oml : 0.f;
    const float st = (va && vb) ? both : (va ? lam : (vb ? oml : 0.f));
    const float za = va ? bf2f(l[ya]) : 0.f, zb = (vb && ya != yb) ? bf2f(l[yb]) : 0.f;
    if (lane == 0) {
        loss_rows[row] = lse * st - (ta * za + tb * zb);  // -sum t * (z - lse)
        if (hit_rows) hit_rows[row] = mixup_px(lam, am == ya ? 1.f : 0.f, oml, am == yb ? 1.f : 0.f);
    }
    if (dlogits) {
        uint16_t *d = dlogits + size_t(row) * ld;
        for (int c = lane; c < ld; c += 64) {
            float gr = 0.f;
            if (c < C) {
                // softmax * sum(t) - t; at a target column written as p * (the other target) - t * (1 - p)
                const float pc = __expf(bf2f(l[c]) - lse);
                if (c == ya) gr = pc * tb - ta * (sa / se);
                else if (c == yb) gr = pc * ta - tb * (sb / se);
                else gr = pc * st;
                gr *= gscale;
            }
            d[c] = f2bf(gr);
        }
    }
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_mix_images(const void *x, const int32_t *perm, const uint32_t *rec, void *out, int B, int C, int H, int W,
                                 void *stream) {
    const MixPlan p = mix_images_plan(x, perm, rec, out, B, C, H, W);
    if (p.err) return fail(p.err, "%s", p.msg);
    const dim3 grid(p.grid, p.grid_y);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.vec == 4)
        hipLaunchKernelGGL(mix_images_kernel<4>, grid, dim3(THREADS), 0, s, static_cast<const float *>(x), perm, rec,
                           static_cast<float *>(out), B, C, p.HW, W);
    else
        hipLaunchKernelGGL(mix_images_kernel<1>, grid, dim3(THREADS), 0, s, static_cast<const float *>(x), perm, rec,
                           static_cast<float *>(out), B, C, p.HW, W);
    return check_launch("mix_images");
}

extern "C" int sfcvit_soft_ce_pair(const void *logits, const int64_t *y_a, const int64_t *y_b, const uint32_t *rec, float *loss_rows,
                                   void *dlogits, float *hit_rows, int B, int C, int ld, float gscale, void *stream) {
    const MixPlan p = soft_ce_pair_plan(logits, y_a, y_b, rec, loss_rows, B, C, ld);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipLaunchKernelGGL(soft_ce_pair_kernel, dim3(p.grid), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(logits), y_a, y_b, rec, loss_rows, static_cast<uint16_t *>(dlogits), hit_rows, B,
                       C, ld, gscale);
    return check_launch("soft_ce_pair");
}
