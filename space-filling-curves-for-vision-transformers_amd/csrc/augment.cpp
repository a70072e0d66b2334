// Host side of the device image transforms (include/sfcvit.h, "Train / test image transforms on the device"): the
// per-sample parameter draw.  No HIP calls; plain C++ so that it is tested without a GPU and joins the sanitizer build.
//
// The stream.  Every uniform is a pure function of (seed, step, sample, draw index):
//     key  = mix32(lo(seed) + 0x9E3779B1); then for w in hi(seed), lo(step), hi(step), lo(sample), hi(sample):
//            key = mix32(key ^ w)
//     h(i) = mix32(key ^ (i * 0x9E3779B1 + 0x7FEB352D))            mix32 = the finaliser of device_common.h
//     U(i) = (h(i) >> 8) * 2^-24 in [0, 1);  U(a, b) = a + (b - a) * U;  randint(0, n) = floor(U * n)
// Draw indices are fixed slots, so no draw depends on how many tries another one took:
//     crop try t (0..9): 4t area, 4t + 1 aspect, 4t + 2 top, 4t + 3 left;  40 flip;  41 order;
//     42..45 brightness, contrast, saturation, hue;  46 erase decision;
//     erase try t (0..9): 48 + 4t area, + 1 aspect, + 2 top, + 3 left.
// The rules are torchvision v2's get_params (RandomResizedCrop, ColorJitter, RandomErasing), arithmetic in double with
// the C library's log / exp / sqrt, int(round(x)) as nearbyint (round half to even, the default rounding mode).
#include "common_host.h"

#include <cmath>
#include <cstring>

// the draw is specified operation by operation (tests restate it in Python): no fused multiply-adds
#pragma clang fp contract(off)

namespace {

inline uint32_t mix32(uint32_t x) {          // device_common.h: mix32, restated for the host
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

struct Stream {
    uint32_t key;
    Stream(uint64_t seed, uint64_t step, uint64_t sample) {
        key = mix32(uint32_t(seed) + 0x9E3779B1u);
        const uint32_t words[5] = {uint32_t(seed >> 32), uint32_t(step), uint32_t(step >> 32), uint32_t(sample), uint32_t(sample >> 32)};
        for (uint32_t w : words) key = mix32(key ^ w);
    }
    double u(uint32_t i) const { return double(mix32(key ^ (i * 0x9E3779B1u + 0x7FEB352Du)) >> 8) * (1.0 / 16777216.0); }
    double u(uint32_t i, double a, double b) const { return a + (b - a) * u(i); }
    int randint(uint32_t i, int n) const { return int(std::floor(u(i) * double(n))); }   // [0, n)
};

inline int iround(double x) { return int(std::nearbyint(x)); }

inline uint32_t f32_bits(double v) {
    const float f = float(v);
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

// The k-th of the 24 orders of (0, 1, 2, 3) in lexicographic order, packed as four 2-bit fields (field i = i-th op).
uint32_t order_word(int k) {
    int items[4] = {0, 1, 2, 3}, left = 4;
    uint32_t word = 0;
    const int fact[4] = {6, 2, 1, 1};
    for (int i = 0; i < 4; i++) {
        const int j = k / fact[i];
        k %= fact[i];
        word |= uint32_t(items[j]) << (2 * i);
        for (int m = j; m + 1 < left; m++) items[m] = items[m + 1];
        left--;
    }
    return word;
}

}  // namespace

using sfcvit::fail;

extern "C" int sfcvit_augment_draw(uint32_t *rec_host, int B, int H, int W, const sfcvit_augment_cfg *cfg, uint64_t seed,
                                   uint64_t step, int64_t sample_base) {
    if (!rec_host || !cfg) return fail(SFCVIT_EINVAL, "augment_draw: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || H > 32768 || W > 32768 || cfg->S <= 0 || cfg->S > 32768)
        return fail(SFCVIT_EINVAL, "augment_draw: B=%d H=%d W=%d S=%d", B, H, W, cfg->S);
    if (cfg->crop && !(cfg->scale[0] > 0 && cfg->scale[0] <= cfg->scale[1] && cfg->ratio[0] > 0 && cfg->ratio[0] <= cfg->ratio[1]))
        return fail(SFCVIT_EINVAL, "augment_draw: scale (%g, %g) / ratio (%g, %g) must be positive, ascending ranges", cfg->scale[0],
                    cfg->scale[1], cfg->ratio[0], cfg->ratio[1]);
    if (!(cfg->brightness >= 0 && cfg->contrast >= 0 && cfg->saturation >= 0 && cfg->hue >= 0 && cfg->hue <= 0.5 &&
          cfg->erase_p >= 0 && cfg->erase_p <= 1))
        return fail(SFCVIT_EINVAL, "augment_draw: jitter ranges must be >= 0 (hue <= 0.5) and erase_p in [0, 1]");
    const int S = cfg->S;
    const double jit[4] = {cfg->brightness, cfg->contrast, cfg->saturation, cfg->hue};
    for (int b = 0; b < B; b++) {
        const Stream st(seed, step, uint64_t(sample_base + b));
        uint32_t *r = rec_host + size_t(b) * SFCVIT_AUG_WORDS;
        std::memset(r, 0, SFCVIT_AUG_WORDS * 4);
        uint32_t flags = 0;
        // ---- RandomResizedCrop.get_params
        int top = 0, left = 0, h = H, w = W;
        if (cfg->crop) {
            const double l0 = std::log(cfg->ratio[0]), l1 = std::log(cfg->ratio[1]);
            bool found = false;
            for (uint32_t t = 0; t < 10 && !found; t++) {
                const double area = double(H) * double(W) * st.u(4 * t, cfg->scale[0], cfg->scale[1]);
                const double aspect = std::exp(st.u(4 * t + 1, l0, l1));
                const int cw = iround(std::sqrt(area * aspect)), ch = iround(std::sqrt(area / aspect));
                if (cw > 0 && cw <= W && ch > 0 && ch <= H) {
                    w = cw; h = ch;
                    top = st.randint(4 * t + 2, H - h + 1);
                    left = st.randint(4 * t + 3, W - w + 1);
                    found = true;
                }
            }
            if (!found) {                                  // central crop clipped to the ratio range
                const double in_ratio = double(W) / double(H);
                if (in_ratio < cfg->ratio[0]) { w = W; h = iround(w / cfg->ratio[0]); }
                else if (in_ratio > cfg->ratio[1]) { h = H; w = iround(h * cfg->ratio[1]); }
                else { w = W; h = H; }
                h = h < 1 ? 1 : (h > H ? H : h);
                w = w < 1 ? 1 : (w > W ? W : w);
                top = (H - h) / 2;
                left = (W - w) / 2;
            }
        }
        r[SFCVIT_AUG_CROP + 0] = uint32_t(top); r[SFCVIT_AUG_CROP + 1] = uint32_t(left);
        r[SFCVIT_AUG_CROP + 2] = uint32_t(h);   r[SFCVIT_AUG_CROP + 3] = uint32_t(w);
        // ---- RandomHorizontalFlip
        if (cfg->flip && st.u(40) < 0.5) flags |= SFCVIT_AUG_FLIP_BIT;
        // ---- ColorJitter.get_params
        const bool any_jitter = jit[0] > 0 || jit[1] > 0 || jit[2] > 0 || jit[3] > 0;
        r[SFCVIT_AUG_ORDER] = any_jitter ? order_word(st.randint(41, 24)) : SFCVIT_AUG_ORDER_IDENTITY;
        for (int op = 0; op < 4; op++) {
            double f = op == 3 ? 0.0 : 1.0;
            if (jit[op] > 0) {
                flags |= 1u << (SFCVIT_AUG_JITTER_SHIFT + op);
                f = op == 3 ? st.u(42 + op, -jit[op], jit[op]) : st.u(42 + op, std::fmax(0.0, 1.0 - jit[op]), 1.0 + jit[op]);
            }
            r[SFCVIT_AUG_FACTORS + op] = f32_bits(f);
        }
        // ---- RandomErasing.get_params on the S x S output
        if (cfg->erase_p > 0 && st.u(46) < cfg->erase_p) {
            const double l0 = std::log(0.3), l1 = std::log(3.3);
            for (uint32_t t = 0; t < 10; t++) {
                const double area = double(S) * double(S) * st.u(48 + 4 * t, 0.02, 0.33);
                const double aspect = std::exp(st.u(49 + 4 * t, l0, l1));
                const int eh = iround(std::sqrt(area * aspect)), ew = iround(std::sqrt(area / aspect));
                if (eh < S && ew < S) {
                    flags |= SFCVIT_AUG_ERASE_BIT;
                    r[SFCVIT_AUG_ERASE + 0] = uint32_t(st.randint(50 + 4 * t, S - eh + 1));
                    r[SFCVIT_AUG_ERASE + 1] = uint32_t(st.randint(51 + 4 * t, S - ew + 1));
                    r[SFCVIT_AUG_ERASE + 2] = uint32_t(eh);
                    r[SFCVIT_AUG_ERASE + 3] = uint32_t(ew);
                    break;
                }
            }
        }
        r[SFCVIT_AUG_FLAGS] = flags;
    }
    return SFCVIT_OK;
}
