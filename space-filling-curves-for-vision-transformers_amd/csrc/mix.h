// Device side of the batch mix record (include/sfcvit.h, "MixUp / CutMix on the device"): shared by the gather kernels
// (patch_embed.hip), the one-pass image mixer and the label-pair loss (mix.hip).
#pragma once
#include "device_common.h"

namespace sfcvit {

struct MixRec {
    uint32_t mode;            // 0 none, 1 MixUp, 2 CutMix
    int r0, r1, c0, c1;       // CutMix box [r0, r1) x [c0, c1) on tensor dims 2 and 3, as it is applied
    float lam, oml;           // lam and 1 - lam, each rounded once on the host
};

// All eight words through uniform addresses: once per wave, not per pixel.
__device__ __forceinline__ MixRec load_mix_rec(const uint32_t *__restrict__ rec) {
    MixRec m;
    m.mode = rec[0];
    m.r0 = int(rec[1]); m.r1 = int(rec[2]); m.c0 = int(rec[3]); m.c1 = int(rec[4]);
    m.lam = __uint_as_float(rec[5]); m.oml = __uint_as_float(rec[6]);
    return m;
}

// Partner image of image b.  A value outside [0, B) (a record that was never filled in) falls back to b itself: no read
// leaves the batch whatever the buffer holds.
__device__ __forceinline__ int mix_partner(const int32_t *__restrict__ perm, int b, int B) {
    const int q = perm[b];
    return unsigned(q) < unsigned(B) ? q : b;
}

// lam * a + (1 - lam) * b as torch evaluates it: two products and a sum, each rounded to fp32.  The library is built
// with -ffp-contract=fast and a fused multiply-add gives other bits, so contraction is switched off for these three.
__device__ __forceinline__ float mixup_px(float lam, float a, float oml, float b) {
#pragma clang fp contract(off)
    const float pa = lam * a;
    const float pb = oml * b;
    return pa + pb;
}

__device__ __forceinline__ bool in_box(const MixRec &m, int row, int col) {
    return row >= m.r0 && row < m.r1 && col >= m.c0 && col < m.c1;
}

// Does pixel (row, col) need the partner image at all?
__device__ __forceinline__ bool mix_needs_partner(const MixRec &m, int row, int col) {
    return m.mode == 1u || (m.mode == 2u && in_box(m, row, col));
}

// One pixel, branch-free: a = x[b], bq = x[perm[b]] (any value where mix_needs_partner said no), inside = the pixel is in
// the CutMix box.  Mode 0 gives a.
__device__ __forceinline__ float mix_px(const MixRec &m, float a, float bq, bool inside) {
    const float mu = mixup_px(m.lam, a, m.oml, bq);
    const float cm = (m.mode == 2u && inside) ? bq : a;
    return m.mode == 1u ? mu : cm;
}

}  // namespace sfcvit
