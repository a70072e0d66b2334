#include "common_host.h"
#include "rowwise.h"
#include "tokenizer.h"

#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdlib>
#include <mutex>

namespace sfcvit {
namespace {
thread_local char g_err[512] = "";
thread_local GemmPlan g_gemm;
thread_local bool g_gemm_noted = false;
}
thread_local KernelNote g_attn, g_rowwise;

int env_int(const char *name, int def) {
    const char *e = getenv(name);
    return e ? atoi(e) : def;
}

char env_first(const char *name) {
    const char *e = getenv(name);
    return e ? e[0] : 0;
}

int env_pair(const char *name, int *a, int *b) {
    const char *e = getenv(name);
    const int n = e ? sscanf(e, "%d,%d", a, b) : 0;
    return n > 0 ? n : 0;
}

Knobs read_knobs(KnobScope scope) {
    static const Knobs once = [] {
        Knobs k;
        k.gemm_walk = env_int("SFCVIT_GEMM_WALK", -1);
        k.attn_bwd_queue = !env_off("SFCVIT_ATTN_BWD_QUEUE");
        k.attn_nt = env_int("SFCVIT_ATTN_NT", 0);
        return k;
    }();
    Knobs k = once;
    if (scope == KNOBS_GEMM) {
        k.gemm_2phase = !env_off("SFCVIT_GEMM_2PHASE");
        env_pair("SFCVIT_GEMM_STAGGER", &k.gemm_stagger_slots, &k.gemm_stagger_ticks);
        k.reserve_cus = env_int("SFCVIT_RESERVE_CUS", 0);
        return k;
    }
    k.attn_long = !env_off("SFCVIT_ATTN_LONG");
    k.attn_wide_stream = env_int("SFCVIT_ATTN_WIDE_STREAM", 0) != 0;
    if (scope == KNOBS_ATTN_BWD) {
        k.attn_bwd_fused = !env_off("SFCVIT_ATTN_BWD_FUSED");
        k.attn_dq_in_kernel = env_first("SFCVIT_ATTN_DQSUM") != 'p';
        k.attn_bwd_persist = !env_off("SFCVIT_ATTN_BWD_PERSIST");
        int slots = 0;
        if (env_pair("SFCVIT_ATTN_STAGGER_BWD", &slots, &k.attn_stagger_ticks)) k.attn_stagger_slots = slots < 1 ? 1 : slots;
    }
    return k;
}

const RowwiseKnobs &read_rowwise_knobs() {
    static const RowwiseKnobs once = [] {
        RowwiseKnobs k;
        k.ln_cols = !env_off("SFCVIT_LN_COLS");
        k.ln_blocks = env_int("SFCVIT_LN_BLOCKS", k.ln_blocks);
        k.ln_fwd_two_rows = env_int("SFCVIT_LN_FWD_TWO_ROWS", k.ln_fwd_two_rows);
        k.adamw_nt = env_int("SFCVIT_ADAMW_NT", k.adamw_nt);
        return k;
    }();
    return once;
}

const TokenizerKnobs &read_tokenizer_knobs() {
    static const TokenizerKnobs once = [] {
        TokenizerKnobs k;
        k.gather_u = env_int("SFCVIT_GATHER_U", k.gather_u);
        k.gather_nt = env_int("SFCVIT_GATHER_NT", k.gather_nt);
        return k;
    }();
    return once;
}

// ---- the scaffold of plan.h ----
void refuse(PlanStatus &p, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.msg, sizeof(p.msg), fmt, ap);
    va_end(ap);
    p.err = code;
}

void KernelNote::set(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof(name), fmt, ap);
    va_end(ap);
}

int KernelNote::read(char *buf, int n) const {
    if (!buf || n <= 0) return SFCVIT_EINVAL;
    snprintf(buf, size_t(n), "%s", name);
    return SFCVIT_OK;
}

void note_attn_kernel(const AttnPlan &p) { kernel_name(p, g_attn.name, sizeof(g_attn.name)); }
void note_attn_kernel(const ProbePlan &p) { kernel_name(p, g_attn.name, sizeof(g_attn.name)); }

// The GEMM note stays a copy of the plan (about 100 launches per training step): the name is formatted when it is asked for.
void note_gemm_kernel(const GemmPlan &p) {
    g_gemm = p;
    g_gemm_noted = true;
}

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

void clear_error() { g_err[0] = 0; }

// hipFuncSetAttribute applies to the kernel on the CURRENT device only: one flag per (kernel, device).
int raise_lds_limit(const void *kernel, int bytes, const char *what) {
    struct Entry { const void *fn; uint64_t devs; };
    static Entry table[128];
    static int used = 0;
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fail(SFCVIT_ENODEV, "%s: no current HIP device", what);
    std::lock_guard<std::mutex> lock(mu);
    Entry *e = nullptr;
    for (int i = 0; i < used && !e; i++)
        if (table[i].fn == kernel) e = &table[i];
    if (e && (e->devs >> dev & 1)) return SFCVIT_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return check_launch(what);
    if (!e && used < 128) { e = &table[used++]; e->fn = kernel; e->devs = 0; }
    if (e) e->devs |= uint64_t(1) << dev;          // a full table only costs the repeated (idempotent) call
    return SFCVIT_OK;
}

// Compute units of the current device (cached per device; threads that race on the first call store the same value); 0 if
// it cannot be told.
int device_cu_count() {
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (!n) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        n = prop.multiProcessorCount;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SFCVIT_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return SFCVIT_OK;
}

}  // namespace sfcvit

extern "C" int sfcvit_abi_version(void) { return SFCVIT_ABI_VERSION; }

extern "C" const char *sfcvit_last_error(void) { return sfcvit::g_err; }

extern "C" int sfcvit_last_gemm_kernel(char *buf, int n) {
    sfcvit::KernelNote note;                                     // "none" until a GEMM has run
    if (sfcvit::g_gemm_noted) sfcvit::kernel_name(sfcvit::g_gemm, note.name, sizeof(note.name));
    return note.read(buf, n);
}

extern "C" int sfcvit_last_attn_kernel(char *buf, int n) { return sfcvit::g_attn.read(buf, n); }

extern "C" int sfcvit_last_rowwise_kernel(char *buf, int n) { return sfcvit::g_rowwise.read(buf, n); }

extern "C" int sfcvit_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return -int(e);
    return n;
}
