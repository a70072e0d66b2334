// The optimizer step for gfx950: sum of squares (gradient norm), the fused clip + AdamW step, the same with the model EMA in
// it, gradient accumulation, and the device-resident step state.  HBM-bound: every global access is a 16-byte vector (8 bf16
// or 4 fp32; the four-per-lane kernels pair an 8-byte bf16 access with it).  The launchers run what the plans of rowwise.h /
// model_ema.h / grad_accum.h say.
#include "common_host.h"
#include "grad_accum.h"
#include "model_ema.h"
#include "rowwise_device.h"

namespace sfcvit {
namespace {

constexpr int THREADS = ROW_THREADS;
constexpr int WAVES = ROW_WAVES;
static_assert(ADAMW_THREADS == THREADS, "model_ema.h plans the grids for this file's workgroup size");

// ---------------------------------------------------------------------------
// Sum of squares (gradient norm) and fused clip + AdamW
// ---------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(THREADS) void sumsq_kernel(const void *__restrict__ g, int64_t n, float *__restrict__ out) {
    __shared__ float red[WAVES];
    float s = 0.f;
    const int64_t nvec = n >> 3;
    for (int64_t i = blockIdx.x * int64_t(THREADS) + threadIdx.x; i < nvec; i += int64_t(gridDim.x) * THREADS) {
        float v[8];
        if (F32) {
            const f32x4 a = reinterpret_cast<const f32x4 *>(g)[2 * i], b = reinterpret_cast<const f32x4 *>(g)[2 * i + 1];
            v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
        } else {
            unpack8(reinterpret_cast<const u32x4 *>(g)[i], v);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) s += v[j] * v[j];
    }
    if (blockIdx.x == 0 && threadIdx.x < int(n & 7)) {   // tail (< 8 elements)
        const int64_t i = (nvec << 3) + threadIdx.x;
        const float v = F32 ? static_cast<const float *>(g)[i] : bf2f(static_cast<const uint16_t *>(g)[i]);
        s += v * v;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; w++) t += red[w];
        out[blockIdx.x] = t;                           // partial[block]
    }
}

// *out += sum of the block partials in a fixed order (lane-strided, then the wave butterfly)
__global__ __launch_bounds__(64) void sumsq_reduce_kernel(const float *__restrict__ part, int nparts, float *__restrict__ out) {
    float t = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 64) t += part[i];
    t = wave_sum(t);
    if (threadIdx.x == 0) *out += t;
}

// 8 elements per thread-iteration: bf16 param / grad as one 16-byte vector, fp32 master / m / v
// as two each.  n_vec = n / 8; the (< 8 element) tail is handled by the first threads.
__device__ __forceinline__ void adamw_one(float &w, float &m, float &v, float gr, const sfcvit_adamw_args &a, float bc1,
                                          float rbc2) {
    w *= 1.f - a.lr * a.weight_decay;
    m = a.beta1 * m + (1.f - a.beta1) * gr;
    v = a.beta2 * v + (1.f - a.beta2) * gr * gr;
    const float denom = sqrtf(v) * rbc2 + a.eps;
    w -= (a.lr / bc1) * (m / denom);
}

template <int NT>      // bit 0: non-temporal loads, bit 1: non-temporal stores of the fp32 state
__global__ __launch_bounds__(THREADS) void adamw_kernel(sfcvit_adamw_args a, float bc1, float rbc2) {
    if (a.dev_state) {            // learning rate and bias corrections of THIS step from the device (sfcvit_step_advance)
        a.lr = a.dev_state[2];
        bc1 = a.dev_state[3];
        rbc2 = a.dev_state[4];
    }
    float gmul = a.grad_scale;
    if (a.sumsq) {
        const float norm = sqrtf(*a.sumsq) * a.grad_scale;
        gmul *= fminf(1.f, a.max_norm / (norm + 1e-6f));
    }
    uint16_t *p = static_cast<uint16_t *>(a.param);
    const uint16_t *g = static_cast<const uint16_t *>(a.grad);
    // A lane owns groups of FOUR parameters: one 8-byte load of the bf16 gradient and one 16-byte load of each fp32 buffer,
    // so that every wave instruction covers one contiguous 512-byte / 1-KiB span (with eight parameters per lane the fp32
    // loads were two 16-byte halves at a 32-byte lane stride: half-used lines per instruction, 4.0 TB/s; tools/bench_adamw.py).
    // Two groups per iteration keep 2 x 56 bytes per lane in flight.
    const int64_t nq = a.n >> 2, step = int64_t(gridDim.x) * THREADS;
    auto load = [&](int64_t i, u32x2 &gq, f32x4 &wv, f32x4 &mv, f32x4 &vv) __attribute__((always_inline)) {
        if (NT & 1) {                                               // every byte is touched once per step
            gq = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(g) + i);
            wv = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(a.master) + i);
            mv = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(a.m) + i);
            vv = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(a.v) + i);
        } else {
            gq = reinterpret_cast<const u32x2 *>(g)[i];
            wv = reinterpret_cast<const f32x4 *>(a.master)[i];
            mv = reinterpret_cast<const f32x4 *>(a.m)[i];
            vv = reinterpret_cast<const f32x4 *>(a.v)[i];
        }
    };
    auto update = [&](int64_t i, const u32x2 &gq, f32x4 wv, f32x4 mv, f32x4 vv) __attribute__((always_inline)) {
        const float gr[4] = {bf2f(uint16_t(gq[0])), bf2f(uint16_t(gq[0] >> 16)), bf2f(uint16_t(gq[1])), bf2f(uint16_t(gq[1] >> 16))};
        float w[4], m[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            w[j] = wv[j];
            m[j] = mv[j];
            v[j] = vv[j];
            adamw_one(w[j], m[j], v[j], gr[j] * gmul, a, bc1, rbc2);
        }
        if (NT & 2) {
            __builtin_nontemporal_store(f32x4{w[0], w[1], w[2], w[3]}, reinterpret_cast<f32x4 *>(a.master) + i);
            __builtin_nontemporal_store(f32x4{m[0], m[1], m[2], m[3]}, reinterpret_cast<f32x4 *>(a.m) + i);
            __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4 *>(a.v) + i);
        } else {
            reinterpret_cast<f32x4 *>(a.master)[i] = f32x4{w[0], w[1], w[2], w[3]};
            reinterpret_cast<f32x4 *>(a.m)[i] = f32x4{m[0], m[1], m[2], m[3]};
            reinterpret_cast<f32x4 *>(a.v)[i] = f32x4{v[0], v[1], v[2], v[3]};
        }
        reinterpret_cast<u32x2 *>(p)[i] = u32x2{pack2bf(w[0], w[1]), pack2bf(w[2], w[3])};   // (the next forward reads these)
    };
    int64_t i = blockIdx.x * int64_t(THREADS) + threadIdx.x;
    for (; i + step < nq; i += 2 * step) {
        u32x2 g0, g1;
        f32x4 w0, m0, v0, w1, m1, v1;
        load(i, g0, w0, m0, v0);
        load(i + step, g1, w1, m1, v1);
        update(i, g0, w0, m0, v0);
        update(i + step, g1, w1, m1, v1);
    }
    if (i < nq) {
        u32x2 g0;
        f32x4 w0, m0, v0;
        load(i, g0, w0, m0, v0);
        update(i, g0, w0, m0, v0);
    }
    if (blockIdx.x == 0 && threadIdx.x < int(a.n & 3)) {
        const int64_t t = (nq << 2) + threadIdx.x;
        float w = a.master[t], m = a.m[t], v = a.v[t];
        adamw_one(w, m, v, bf2f(g[t]) * gmul, a, bc1, rbc2);
        a.master[t] = w;
        a.m[t] = m;
        a.v[t] = v;
        p[t] = f2bf(w);
    }
}

// adamw_kernel plus an exponential moving average of the fp32 master weights (model_ema.h): after adamw_one has produced the
// new w, e <- e + (1 - d_t) * (w - e) with e fp32, one more 16-byte stream in and out per lane (36 bytes per parameter instead
// of 28, no second pass over master).  d_t = decay, or with `warmup` min(decay, (1 + t) / (10 + t)), t the 1-based step of
// this update: a.step, or the device counter when dev_state is set, read when the kernel runs -- so a captured step replays
// with the right decay.  A kernel of its own: param, master, m and v get adamw_kernel's bits, and adamw_kernel keeps its
// text (a shared templated body changes the existing instantiations, profiles/drop_path/isa_identity.txt).
template <int NT>      // as adamw_kernel
__global__ __launch_bounds__(THREADS) void adamw_ema_kernel(sfcvit_adamw_args a, float bc1, float rbc2, float *__restrict__ ema,
                                                            float decay, int warmup, int t) {
    if (a.dev_state) {            // t arrives as a.step in an argument of its own: a value, not a second address to load from
        a.lr = a.dev_state[2];
        bc1 = a.dev_state[3];
        rbc2 = a.dev_state[4];
        t = reinterpret_cast<const int32_t *>(a.dev_state)[1];
    }
    const float d = warmup ? fminf(decay, float(1 + t) / float(10 + t)) : decay;      // a true (correctly rounded) division
    const float omd = 1.f - d;                                                         // exact for d >= 0.5 (Sterbenz)
    float gmul = a.grad_scale;
    if (a.sumsq) {
        const float norm = sqrtf(*a.sumsq) * a.grad_scale;
        gmul *= fminf(1.f, a.max_norm / (norm + 1e-6f));
    }
    uint16_t *p = static_cast<uint16_t *>(a.param);
    const uint16_t *g = static_cast<const uint16_t *>(a.grad);
    // adamw_kernel's layout: four parameters per lane and group, two groups in flight (2 x 72 bytes per lane here)
    const int64_t nq = a.n >> 2, step = int64_t(gridDim.x) * THREADS;
    auto load = [&](int64_t i, u32x2 &gq, f32x4 &wv, f32x4 &mv, f32x4 &vv, f32x4 &ev) __attribute__((always_inline)) {
        if (NT & 1) {
            gq = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(g) + i);
            wv = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(a.master) + i);
            mv = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(a.m) + i);
            vv = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(a.v) + i);
            ev = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(ema) + i);
        } else {
            gq = reinterpret_cast<const u32x2 *>(g)[i];
            wv = reinterpret_cast<const f32x4 *>(a.master)[i];
            mv = reinterpret_cast<const f32x4 *>(a.m)[i];
            vv = reinterpret_cast<const f32x4 *>(a.v)[i];
            ev = reinterpret_cast<const f32x4 *>(ema)[i];
        }
    };
    auto update = [&](int64_t i, const u32x2 &gq, f32x4 wv, f32x4 mv, f32x4 vv, f32x4 ev) __attribute__((always_inline)) {
        const float gr[4] = {bf2f(uint16_t(gq[0])), bf2f(uint16_t(gq[0] >> 16)), bf2f(uint16_t(gq[1])), bf2f(uint16_t(gq[1] >> 16))};
        float w[4], m[4], v[4], e[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            w[j] = wv[j];
            m[j] = mv[j];
            v[j] = vv[j];
            adamw_one(w[j], m[j], v[j], gr[j] * gmul, a, bc1, rbc2);
            e[j] = ev[j] + omd * (w[j] - ev[j]);
        }
        if (NT & 2) {
            __builtin_nontemporal_store(f32x4{w[0], w[1], w[2], w[3]}, reinterpret_cast<f32x4 *>(a.master) + i);
            __builtin_nontemporal_store(f32x4{m[0], m[1], m[2], m[3]}, reinterpret_cast<f32x4 *>(a.m) + i);
            __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4 *>(a.v) + i);
            __builtin_nontemporal_store(f32x4{e[0], e[1], e[2], e[3]}, reinterpret_cast<f32x4 *>(ema) + i);
        } else {
            reinterpret_cast<f32x4 *>(a.master)[i] = f32x4{w[0], w[1], w[2], w[3]};
            reinterpret_cast<f32x4 *>(a.m)[i] = f32x4{m[0], m[1], m[2], m[3]};
            reinterpret_cast<f32x4 *>(a.v)[i] = f32x4{v[0], v[1], v[2], v[3]};
            reinterpret_cast<f32x4 *>(ema)[i] = f32x4{e[0], e[1], e[2], e[3]};
        }
        reinterpret_cast<u32x2 *>(p)[i] = u32x2{pack2bf(w[0], w[1]), pack2bf(w[2], w[3])};
    };
    int64_t i = blockIdx.x * int64_t(THREADS) + threadIdx.x;
    for (; i + step < nq; i += 2 * step) {
        u32x2 g0, g1;
        f32x4 w0, m0, v0, e0, w1, m1, v1, e1;
        load(i, g0, w0, m0, v0, e0);
        load(i + step, g1, w1, m1, v1, e1);
        update(i, g0, w0, m0, v0, e0);
        update(i + step, g1, w1, m1, v1, e1);
    }
    if (i < nq) {
        u32x2 g0;
        f32x4 w0, m0, v0, e0;
        load(i, g0, w0, m0, v0, e0);
        update(i, g0, w0, m0, v0, e0);
    }
    if (blockIdx.x == 0 && threadIdx.x < int(a.n & 3)) {
        const int64_t k = (nq << 2) + threadIdx.x;
        float w = a.master[k], m = a.m[k], v = a.v[k];
        const float e = ema[k];
        adamw_one(w, m, v, bf2f(g[k]) * gmul, a, bc1, rbc2);
        a.master[k] = w;
        a.m[k] = m;
        a.v[k] = v;
        ema[k] = e + omd * (w - e);
        p[k] = f2bf(w);
    }
}

// ---------------------------------------------------------------------------
// Gradient accumulation (grad_accum.h): fp32 running sum of the micro-batch gradients, and on the last micro-batch the
// average formed in place with the clip's sum of squares in the same pass.  adamw_kernel's layout: four parameters per lane
// and group (an 8-byte bf16 access, a 16-byte fp32 one), two groups in flight, a remainder group and the under-4 tail.
// Kernels of their own: sumsq_kernel and adamw_kernel keep their text (profiles/grad_accum/isa_identity.txt).
// ---------------------------------------------------------------------------
// acc = float(g) (FIRST: acc is not read) or acc + float(g): one fp32 add per element.  6 / 10 bytes per parameter, every
// byte touched once: NT as adamw_kernel (bit 0 loads, bit 1 the store of acc, which nothing reads before the next pass).
template <bool FIRST, int NT>
__global__ __launch_bounds__(THREADS) void grad_accum_kernel(const uint16_t *__restrict__ g, float *__restrict__ acc, int64_t n) {
    const int64_t nq = n >> 2, step = int64_t(gridDim.x) * THREADS;
    auto load = [&](int64_t i, u32x2 &gq, f32x4 &av) __attribute__((always_inline)) {
        if (NT & 1) {
            gq = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(g) + i);
            if (!FIRST) av = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(acc) + i);
        } else {
            gq = reinterpret_cast<const u32x2 *>(g)[i];
            if (!FIRST) av = reinterpret_cast<const f32x4 *>(acc)[i];
        }
    };
    auto update = [&](int64_t i, const u32x2 &gq, const f32x4 &av) __attribute__((always_inline)) {
        const float gr[4] = {bf2f(uint16_t(gq[0])), bf2f(uint16_t(gq[0] >> 16)), bf2f(uint16_t(gq[1])), bf2f(uint16_t(gq[1] >> 16))};
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; j++) r[j] = FIRST ? gr[j] : av[j] + gr[j];
        if (NT & 2) __builtin_nontemporal_store(r, reinterpret_cast<f32x4 *>(acc) + i);
        else reinterpret_cast<f32x4 *>(acc)[i] = r;
    };
    int64_t i = blockIdx.x * int64_t(THREADS) + threadIdx.x;
    for (; i + step < nq; i += 2 * step) {
        u32x2 g0, g1;
        f32x4 a0 = {}, a1 = {};
        load(i, g0, a0);
        load(i + step, g1, a1);
        update(i, g0, a0);
        update(i + step, g1, a1);
    }
    if (i < nq) {
        u32x2 g0;
        f32x4 a0 = {};
        load(i, g0, a0);
        update(i, g0, a0);
    }
    if (blockIdx.x == 0 && threadIdx.x < int(n & 3)) {
        const int64_t t = (nq << 2) + threadIdx.x;
        acc[t] = FIRST ? bf2f(g[t]) : acc[t] + bf2f(g[t]);
    }
}

// g = bf16((acc + float(g)) * scale) in place: one add, one multiply, one rounding (an add feeding a multiply cannot contract).
// SUMSQ: part[block] = sum of the squares of the STORED bf16 values, the per-workgroup partials of sumsq_kernel, which
// sumsq_reduce_kernel adds into *sumsq in a fixed order.  8 bytes per parameter: acc is read once (NT bit 0); g is stored
// plainly, the AdamW kernel reads it next.
template <bool SUMSQ, int NT>
__global__ __launch_bounds__(THREADS) void grad_accum_finish_kernel(uint16_t *__restrict__ g, const float *__restrict__ acc, int64_t n,
                                                                    float scale, float *__restrict__ part) {
    __shared__ float red[WAVES];
    float s = 0.f;
    const int64_t nq = n >> 2, step = int64_t(gridDim.x) * THREADS;
    auto load = [&](int64_t i, u32x2 &gq, f32x4 &av) __attribute__((always_inline)) {
        gq = reinterpret_cast<const u32x2 *>(g)[i];
        if (NT & 1) av = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(acc) + i);
        else av = reinterpret_cast<const f32x4 *>(acc)[i];
    };
    auto update = [&](int64_t i, const u32x2 &gq, const f32x4 &av) __attribute__((always_inline)) {
        const float gr[4] = {bf2f(uint16_t(gq[0])), bf2f(uint16_t(gq[0] >> 16)), bf2f(uint16_t(gq[1])), bf2f(uint16_t(gq[1] >> 16))};
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; j++) r[j] = (av[j] + gr[j]) * scale;
        const u32x2 o = {pack2bf(r[0], r[1]), pack2bf(r[2], r[3])};
        reinterpret_cast<u32x2 *>(g)[i] = o;
        if (SUMSQ) {
            const float q[4] = {bf2f(uint16_t(o[0])), bf2f(uint16_t(o[0] >> 16)), bf2f(uint16_t(o[1])), bf2f(uint16_t(o[1] >> 16))};
#pragma unroll
            for (int j = 0; j < 4; j++) s += q[j] * q[j];
        }
    };
    int64_t i = blockIdx.x * int64_t(THREADS) + threadIdx.x;
    for (; i + step < nq; i += 2 * step) {
        u32x2 g0, g1;
        f32x4 a0, a1;
        load(i, g0, a0);
        load(i + step, g1, a1);
        update(i, g0, a0);
        update(i + step, g1, a1);
    }
    if (i < nq) {
        u32x2 g0;
        f32x4 a0;
        load(i, g0, a0);
        update(i, g0, a0);
    }
    if (blockIdx.x == 0 && threadIdx.x < int(n & 3)) {
        const int64_t t = (nq << 2) + threadIdx.x;
        const uint16_t o = f2bf((acc[t] + bf2f(g[t])) * scale);
        g[t] = o;
        if (SUMSQ) s += bf2f(o) * bf2f(o);
    }
    if (SUMSQ) {
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; w++) t += red[w];
            part[blockIdx.x] = t;                          // partial[block]
        }
    }
}

// ---------------------------------------------------------------------------
// Device-resident step state: [0] dropout seed offset (uint32)  [1] step count (int32)  [2] learning rate (float,
// written by the host, read by adamw)  [3] 1 - beta1^step  [4] 1 / sqrt(1 - beta2^step).  One thread advances it once
// per training step -- as the first node of a captured step graph, so that every replay draws new dropout masks and
// applies the right Adam bias correction without any by-value kernel argument changing.
// ---------------------------------------------------------------------------
__global__ void step_advance_kernel(uint32_t *state, float beta1, float beta2, uint32_t seed_base) {
    if (threadIdx.x || blockIdx.x) return;
    const int step = int(state[1]) + 1;
    state[1] = uint32_t(step);
    state[0] = mix32(seed_base ^ (uint32_t(step) * 0x9E3779B1u));
    float *f = reinterpret_cast<float *>(state);
    f[3] = 1.f - powf(beta1, float(step));
    f[4] = 1.f / sqrtf(1.f - powf(beta2, float(step)));
}

// One launch path for sfcvit_adamw_step and, with `e`, sfcvit_adamw_ema_step (model_ema.h).
int launch_adamw(const AdamwPlan &p, const sfcvit_adamw_args *a, const sfcvit_ema_args *e, void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float bc1 = 1.f - powf(a->beta1, float(a->step));
    const float bc2 = 1.f - powf(a->beta2, float(a->step));
    if (e) g_rowwise.set("adamw_ema_kernel<%d>", p.nt);
#define ADAMW(NT) do { \
        if (e) hipLaunchKernelGGL(adamw_ema_kernel<NT>, dim3(p.grid), dim3(THREADS), 0, s, *a, bc1, 1.f / sqrtf(bc2), e->ema, e->decay, int(e->warmup), int(a->step)); \
        else hipLaunchKernelGGL(adamw_kernel<NT>, dim3(p.grid), dim3(THREADS), 0, s, *a, bc1, 1.f / sqrtf(bc2)); } while (0)
    if (p.nt == 3) ADAMW(3); else if (p.nt == 2) ADAMW(2); else if (p.nt == 1) ADAMW(1); else ADAMW(0);
#undef ADAMW
    return check_launch(e ? "adamw_ema" : "adamw");
}

}  // namespace
}  // namespace sfcvit

using namespace sfcvit;

extern "C" int sfcvit_sumsq_accum(const void *g, int64_t n, int is_f32, float *out, void *workspace, void *stream) {
    const RowGridPlan p = sumsq_plan(g, n, out, workspace);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(workspace);
    if (is_f32) hipLaunchKernelGGL(sumsq_kernel<true>, dim3(p.grid), dim3(THREADS), 0, s, g, n, part);
    else hipLaunchKernelGGL(sumsq_kernel<false>, dim3(p.grid), dim3(THREADS), 0, s, g, n, part);
    if (int rc = check_launch("sumsq")) return rc;
    hipLaunchKernelGGL(sumsq_reduce_kernel, dim3(1), dim3(64), 0, s, part, p.grid, out);
    return check_launch("sumsq reduce");
}

extern "C" int sfcvit_adamw_step(const sfcvit_adamw_args *a, void *stream) {
    const AdamwPlan p = adamw_plan(a, read_rowwise_knobs());
    if (p.err) return fail(p.err, "%s", p.msg);
    return launch_adamw(p, a, nullptr, stream);
}

extern "C" int sfcvit_adamw_ema_step(const sfcvit_adamw_args *a, const sfcvit_ema_args *e, void *stream) {
    const AdamwEmaPlan p = adamw_ema_plan(a, e, read_rowwise_knobs());
    if (p.err) return fail(p.err, "%s", p.msg);
    return launch_adamw(p, a, e, stream);
}

extern "C" int sfcvit_grad_accum(const void *grad, float *acc, int64_t n, int first, void *stream) {
    const GradAccumPlan p = grad_accum_plan(grad, acc, n, read_rowwise_knobs());
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint16_t *g = static_cast<const uint16_t *>(grad);
#define ACCUM(NT) do { \
        if (first) hipLaunchKernelGGL((grad_accum_kernel<true, NT>), dim3(p.grid), dim3(THREADS), 0, s, g, acc, n); \
        else hipLaunchKernelGGL((grad_accum_kernel<false, NT>), dim3(p.grid), dim3(THREADS), 0, s, g, acc, n); } while (0)
    if (p.nt == 3) ACCUM(3); else if (p.nt == 2) ACCUM(2); else if (p.nt == 1) ACCUM(1); else ACCUM(0);
#undef ACCUM
    return check_launch("grad_accum");
}

extern "C" int sfcvit_grad_accum_finish(void *grad, const float *acc, int64_t n, float scale, float *sumsq, void *workspace, void *stream) {
    const GradAccumPlan p = grad_accum_finish_plan(grad, acc, n, scale, sumsq, workspace, read_rowwise_knobs());
    if (p.err) return fail(p.err, "%s", p.msg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint16_t *g = static_cast<uint16_t *>(grad);
    float *part = static_cast<float *>(workspace);
    const bool nt = p.nt & 1;                              // the one stream of this kernel that is read once: acc
    if (!sumsq) {
        if (nt) hipLaunchKernelGGL((grad_accum_finish_kernel<false, 1>), dim3(p.grid), dim3(THREADS), 0, s, g, acc, n, scale, nullptr);
        else hipLaunchKernelGGL((grad_accum_finish_kernel<false, 0>), dim3(p.grid), dim3(THREADS), 0, s, g, acc, n, scale, nullptr);
        return check_launch("grad_accum_finish");
    }
    if (nt) hipLaunchKernelGGL((grad_accum_finish_kernel<true, 1>), dim3(p.grid), dim3(THREADS), 0, s, g, acc, n, scale, part);
    else hipLaunchKernelGGL((grad_accum_finish_kernel<true, 0>), dim3(p.grid), dim3(THREADS), 0, s, g, acc, n, scale, part);
    if (int rc = check_launch("grad_accum_finish")) return rc;
    hipLaunchKernelGGL(sumsq_reduce_kernel, dim3(1), dim3(64), 0, s, part, p.grid, sumsq);
    return check_launch("grad_accum_finish reduce");
}

extern "C" int sfcvit_step_advance(void *state, float beta1, float beta2, uint32_t seed_base, void *stream) {
    const RowGridPlan p = step_advance_plan(state);
    if (p.err) return fail(p.err, "%s", p.msg);
    hipLaunchKernelGGL(step_advance_kernel, dim3(p.grid), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<uint32_t *>(state), beta1,
                       beta2, seed_base);
    return check_launch("step_advance");
}
