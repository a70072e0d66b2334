// Device side of the image transforms (include/sfcvit.h, "Train / test image transforms on the device"):
//   sfcvit_augment_apply  uint8 batch + one 16-word record per image -> cropped / resized / flipped / colour-jittered /
//                         erased / normalized fp32 or bf16 batch, one launch, no allocation, no sync.
//
// Shape: ONE WORKGROUP PER IMAGE, a thread owns V consecutive output pixels of a row (V = 4: one 16-byte store per
// channel in fp32; V = 1 when S is not a multiple of 4) with the three channels of each pixel side by side in registers,
// because every jitter op after brightness couples the channels.  The contrast op blends with the mean gray of the image
// AS IT STANDS when the op runs, which depends on the ops in front of it: a record with contrast therefore takes two
// sweeps -- the first evaluates the pipeline up to the contrast op and reduces gray (lane partials in pixel order, wave
// butterfly, LDS across the waves, summed by every thread in wave order: a fixed order, so two runs give the same bits),
// the second finishes.  KEEP = the image fits the workgroup one vector per thread (CIFAR: 32 x 32 / 4 = 256 threads):
// the first sweep's pixels stay in registers; otherwise (224 x 224: 1024 threads, 13 vectors each) the second sweep
// resamples -- the uint8 source of one image is 147 KB and is still in L2.  Records without contrast skip the first sweep.
//
// Bit-exact contract of the geometry (tests compare with a numpy fp32 statement in the same operation order): v / 255.0f,
// the tap weights and the two-level blend h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11), and (x - mean) / std
// are separately rounded IEEE operations: contraction is switched off inside those functions (as mix.h: mixup_px does),
// and this file is built with -ffp-contract=fast-honor-pragmas (csrc/Makefile) -- under the library's plain
// -ffp-contract=fast the backend fuses (dst + 0.5) * scale - 0.5 and the blend whatever the pragma says.  The jitter ops
// are free to contract.
#include "common_host.h"
#include "device_common.h"

namespace sfcvit {
namespace {

struct AugParams {
    int B, C, H, W, S, out_bf16;
    float mean[3], std[3];
};

// One image's record with every field made safe: a crop box clamped into the image (no read leaves the batch whatever
// the buffer holds), an order word that is not a permutation replaced by the identity order.
struct AugRec {
    uint32_t flags, order;
    int top, left, ch, cw;
    int et, el, eh, ew;
    float fac[4];
    float sy, sx;             // crop / S per axis (fp32 division)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ AugRec load_aug_rec(const uint32_t *__restrict__ r, const AugParams &p) {
    AugRec a;
    a.flags = r[SFCVIT_AUG_FLAGS];
    a.top = clampi(int(r[SFCVIT_AUG_CROP + 0]), 0, p.H - 1);
    a.left = clampi(int(r[SFCVIT_AUG_CROP + 1]), 0, p.W - 1);
    a.ch = clampi(int(r[SFCVIT_AUG_CROP + 2]), 1, p.H - a.top);
    a.cw = clampi(int(r[SFCVIT_AUG_CROP + 3]), 1, p.W - a.left);
    a.order = r[SFCVIT_AUG_ORDER] & 0xFFu;
    const uint32_t seen = (1u << (a.order & 3)) | (1u << ((a.order >> 2) & 3)) | (1u << ((a.order >> 4) & 3)) | (1u << ((a.order >> 6) & 3));
    if (seen != 0xFu) a.order = SFCVIT_AUG_ORDER_IDENTITY;
#pragma unroll
    for (int i = 0; i < 4; i++) a.fac[i] = __uint_as_float(r[SFCVIT_AUG_FACTORS + i]);
    a.et = int(r[SFCVIT_AUG_ERASE + 0]); a.el = int(r[SFCVIT_AUG_ERASE + 1]);
    a.eh = int(r[SFCVIT_AUG_ERASE + 2]); a.ew = int(r[SFCVIT_AUG_ERASE + 3]);
    a.sy = float(a.ch) / float(p.S);
    a.sx = float(a.cw) / float(p.S);
    if (p.C != 3) a.flags &= ~(0xFu << SFCVIT_AUG_JITTER_SHIFT);      // colour ops exist for RGB only
    return a;
}

// Source coordinate of output index `dst` along one axis: tap i0, upper tap i1 (clamped to the crop edge), weight of i1.
__device__ __forceinline__ void tap(int dst, float scale, int crop, int &i0, int &i1, float &w1) {
#pragma clang fp contract(off)
    float src = (float(dst) + 0.5f) * scale;
    src = src - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = int(src);
    i0 = i0 > crop - 1 ? crop - 1 : i0;
    i1 = i0 + 1 > crop - 1 ? crop - 1 : i0 + 1;
    w1 = src - float(i0);
}

__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float wx1, float wy1) {
#pragma clang fp contract(off)
    const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    const float a0 = wx0 * v00, a1 = wx1 * v01;
    const float b0 = wx0 * v10, b1 = wx1 * v11;
    const float r0 = wy0 * (a0 + a1), r1 = wy1 * (b0 + b1);
    return r0 + r1;
}

__device__ __forceinline__ float u8_unit(uint8_t v) {
#pragma clang fp contract(off)
    return float(v) / 255.0f;
}

__device__ __forceinline__ float normalize(float x, float mean, float std) {
#pragma clang fp contract(off)
    const float d = x - mean;
    return d / std;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// torchvision's tensor adjust_hue: _rgb2hsv, h = fmod(h + hue + 1, 1), _hsv2rgb.
__device__ __forceinline__ void hue_px(float &r, float &g, float &b, float hue) {
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float div = eqc ? 1.f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    const float hr = maxc == r ? bc - gc : 0.f;
    const float hg = (maxc == g && maxc != r) ? 2.f + rc - bc : 0.f;
    const float hb = (maxc != g && maxc != r) ? 4.f + gc - rc : 0.f;
    float h = fmodf((hr + hg + hb) / 6.f + 1.f, 1.f);
    h = fmodf(h + hue + 1.f, 1.f);
    const float v = maxc;
    const float h6 = h * 6.f;
    const float fi = floorf(h6);
    const float f = h6 - fi;
    int i = int(fi) % 6;
    const float p = clamp01(v * (1.f - s));
    const float q = clamp01(v * (1.f - s * f));
    const float t = clamp01(v * (1.f - s * (1.f - f)));
    r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
    g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
    b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// Jitter ops at positions [from, to) of the record's order on one pixel; m = the gray mean for the contrast op.
__device__ __forceinline__ void jitter_px(const AugRec &a, int from, int to, float m, float &r, float &g, float &b) {
    for (int pos = from; pos < to; pos++) {
        const uint32_t op = (a.order >> (2 * pos)) & 3u;
        if (!((a.flags >> (SFCVIT_AUG_JITTER_SHIFT + op)) & 1u)) continue;
        const float f = op == 0 ? a.fac[0] : op == 1 ? a.fac[1] : op == 2 ? a.fac[2] : a.fac[3];
        if (op == 0) {
            r = clamp01(f * r); g = clamp01(f * g); b = clamp01(f * b);
        } else if (op == 1) {
            const float k = (1.f - f) * m;
            r = clamp01(f * r + k); g = clamp01(f * g + k); b = clamp01(f * b + k);
        } else if (op == 2) {
            const float k = (1.f - f) * gray_of(r, g, b);
            r = clamp01(f * r + k); g = clamp01(f * g + k); b = clamp01(f * b + k);
        } else {
            hue_px(r, g, b, f);
        }
    }
}

// The resized crop at output pixels (oy, ox0 .. ox0 + V - 1), channels 0 .. C - 1 (px[c][e]; channels >= C untouched).
template <int V>
__device__ __forceinline__ void sample(const uint8_t *__restrict__ img, const AugParams &p, const AugRec &a, int oy, int ox0,
                                       float (&px)[3][V]) {
    int y0, y1;
    float wy1;
    tap(oy, a.sy, a.ch, y0, y1, wy1);
    const uint8_t *row0 = img + size_t(a.top + y0) * p.W + a.left;
    const uint8_t *row1 = img + size_t(a.top + y1) * p.W + a.left;
    const size_t plane = size_t(p.H) * p.W;
#pragma unroll
    for (int e = 0; e < V; e++) {
        const int ox = (a.flags & SFCVIT_AUG_FLIP_BIT) ? p.S - 1 - (ox0 + e) : ox0 + e;
        int x0, x1;
        float wx1;
        tap(ox, a.sx, a.cw, x0, x1, wx1);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (c < p.C) {
                const uint8_t *r0 = row0 + c * plane, *r1 = row1 + c * plane;
                px[c][e] = bilerp(u8_unit(r0[x0]), u8_unit(r0[x1]), u8_unit(r1[x0]), u8_unit(r1[x1]), wx1, wy1);
            }
        }
    }
}

template <int THREADS>
__device__ __forceinline__ float block_sum_fixed(float v, float *lds) {
    constexpr int WAVES = THREADS / 64;
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; w++) s += lds[w];
    return s;
}

template <int V>
__device__ __forceinline__ void finish_store(const AugParams &p, const AugRec &a, void *__restrict__ out, int b, int oy, int ox0,
                                             float (&px)[3][V]) {
    const bool erase_row = (a.flags & SFCVIT_AUG_ERASE_BIT) && oy >= a.et && oy < a.et + a.eh;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (c < p.C) {
            float o[V];
#pragma unroll
            for (int e = 0; e < V; e++) {
                const bool erased = erase_row && ox0 + e >= a.el && ox0 + e < a.el + a.ew;
                o[e] = normalize(erased ? 0.f : px[c][e], p.mean[c], p.std[c]);
            }
            const size_t off = ((size_t(b) * p.C + c) * p.S + oy) * p.S + ox0;
            if constexpr (V == 4) {
                if (p.out_bf16)
                    __builtin_nontemporal_store(u32x2{pack2bf(o[0], o[1]), pack2bf(o[2], o[3])},
                                                reinterpret_cast<u32x2 *>(static_cast<uint16_t *>(out) + off));
                else
                    __builtin_nontemporal_store(f32x4{o[0], o[1], o[2], o[3]}, reinterpret_cast<f32x4 *>(static_cast<float *>(out) + off));
            } else {
                if (p.out_bf16) static_cast<uint16_t *>(out)[off] = f2bf(o[0]);
                else static_cast<float *>(out)[off] = o[0];
            }
        }
    }
}

template <int THREADS, int V, bool KEEP>
__global__ __launch_bounds__(THREADS) void augment_kernel(const uint8_t *__restrict__ x, const uint32_t *__restrict__ rec,
                                                          void *__restrict__ out, AugParams p) {
    __shared__ float lds[THREADS / 64];
    const int b = blockIdx.x;
    const AugRec a = load_aug_rec(rec + size_t(b) * SFCVIT_AUG_WORDS, p);
    const uint8_t *img = x + size_t(b) * p.C * p.H * p.W;
    const int per_row = p.S / V, nvec = p.S * per_row;
    const bool color = (a.flags & (0xFu << SFCVIT_AUG_JITTER_SHIFT)) != 0;
    const bool contrast = (a.flags >> (SFCVIT_AUG_JITTER_SHIFT + 1)) & 1u;
    int cpos = 0;                                   // position of the contrast op in the order
#pragma unroll
    for (int i = 0; i < 4; i++) cpos = ((a.order >> (2 * i)) & 3u) == 1u ? i : cpos;

    float keep[3][V] = {};
    float m = 0.f;
    if (contrast) {                                 // block-uniform: every thread reaches the barrier inside
        float part = 0.f;
        for (int q = threadIdx.x; q < nvec; q += THREADS) {
            const int oy = q / per_row, ox0 = (q - oy * per_row) * V;
            float px[3][V];
            sample<V>(img, p, a, oy, ox0, px);
#pragma unroll
            for (int e = 0; e < V; e++) {
                jitter_px(a, 0, cpos, 0.f, px[0][e], px[1][e], px[2][e]);
                part += gray_of(px[0][e], px[1][e], px[2][e]);
                if constexpr (KEEP) { keep[0][e] = px[0][e]; keep[1][e] = px[1][e]; keep[2][e] = px[2][e]; }
            }
        }
        m = block_sum_fixed<THREADS>(part, lds) / float(p.S * p.S);
    }
    for (int q = threadIdx.x; q < nvec; q += THREADS) {
        const int oy = q / per_row, ox0 = (q - oy * per_row) * V;
        float px[3][V];
        if (KEEP && contrast) {
#pragma unroll
            for (int e = 0; e < V; e++) {
                px[0][e] = keep[0][e]; px[1][e] = keep[1][e]; px[2][e] = keep[2][e];
                jitter_px(a, cpos, 4, m, px[0][e], px[1][e], px[2][e]);
            }
        } else {
            sample<V>(img, p, a, oy, ox0, px);
            if (color) {
#pragma unroll
                for (int e = 0; e < V; e++) jitter_px(a, 0, 4, m, px[0][e], px[1][e], px[2][e]);
            }
        }
        finish_store<V>(p, a, out, b, oy, ox0, px);
    }
}

template <int THREADS, int V, bool KEEP>
void launch(const uint8_t *x, const uint32_t *rec, void *out, const AugParams &p, hipStream_t s) {
    hipLaunchKernelGGL((augment_kernel<THREADS, V, KEEP>), dim3(unsigned(p.B)), dim3(THREADS), 0, s, x, rec, out, p);
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_augment_apply(const uint8_t *x, const uint32_t *rec_dev, void *out, int B, int C, int H, int W,
                                    const sfcvit_augment_cfg *cfg, void *stream) {
    if (!x || !rec_dev || !out || !cfg) return fail(SFCVIT_EINVAL, "augment_apply: null pointer");
    const int S = cfg->S;
    if (B <= 0 || C < 1 || C > 3 || H <= 0 || W <= 0 || S <= 0 || S > 32768)
        return fail(SFCVIT_EINVAL, "augment_apply: B=%d C=%d (1..3) H=%d W=%d S=%d", B, C, H, W, S);
    if (S < H || S < W)
        return fail(SFCVIT_EINVAL, "augment_apply: S=%d is smaller than the source %d x %d (downsampling needs antialiasing, "
                                   "which this kernel does not do)", S, H, W);
    if (C != 3 && (cfg->brightness > 0 || cfg->contrast > 0 || cfg->saturation > 0 || cfg->hue > 0))
        return fail(SFCVIT_EINVAL, "augment_apply: colour ops need C == 3, got C=%d", C);
    for (int c = 0; c < 3; c++)
        if (!(cfg->std[c] != 0.f) || !(cfg->mean[c] == cfg->mean[c]))
            return fail(SFCVIT_EINVAL, "augment_apply: std[%d]=%g must be nonzero (mean %g)", c, double(cfg->std[c]), double(cfg->mean[c]));
    if (!aligned16(rec_dev) || !aligned16(out)) return fail(SFCVIT_EINVAL, "augment_apply: rec and out must be 16-byte aligned");
    AugParams p;
    p.B = B; p.C = C; p.H = H; p.W = W; p.S = S; p.out_bf16 = cfg->out_is_bf16 ? 1 : 0;
    for (int c = 0; c < 3; c++) { p.mean[c] = cfg->mean[c]; p.std[c] = cfg->std[c]; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (S % 4 == 0) {
        if (S * (S / 4) <= 256) launch<256, 4, true>(x, rec_dev, out, p, s);
        else launch<1024, 4, false>(x, rec_dev, out, p, s);
    } else {
        if (S * S <= 256) launch<256, 1, true>(x, rec_dev, out, p, s);
        else launch<1024, 1, false>(x, rec_dev, out, p, s);
    }
    return check_launch("augment_apply");
}
