// Argument checks and launch geometry of sfcvit_dwconv1d_fwd / _bwd (token_agg.h), on the scaffold of plan.h.  Plain host
// code: no HIP call, no allocation, so every refusal is testable on a machine without a GPU.
#include "token_agg.h"

#include "common_host.h"

namespace sfcvit {

thread_local KernelNote g_dwconv;

DwconvPlan dwconv_plan(const char *what, int B, int N, int D, int k, int s) {
    DwconvPlan p;
    if (k < 1 || k > DWC_MAX_K) REFUSE(SFCVIT_EINVAL, "%s: kernel size k=%d not supported (1..%d)", what, k, DWC_MAX_K);
    if (s < 1 || s > DWC_MAX_S) REFUSE(SFCVIT_EINVAL, "%s: stride s=%d not supported (1..%d)", what, s, DWC_MAX_S);
    if (D <= 0 || D % 8) REFUSE(SFCVIT_EINVAL, "%s: D=%d must be a positive multiple of 8", what, D);
    if (B <= 0 || N <= 0 || B > 65535) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d (1 <= B <= 65535, N >= 1)", what, B, N);
    if (int64_t(N) + 2 * DWC_MAX_K > INT32_MAX / 2) REFUSE(SFCVIT_EINVAL, "%s: N=%d too long", what, N);
    p.pad = k / 2;
    p.Nout = (N + 2 * p.pad - k) / s + 1;       // >= 1: N + 2 (k / 2) >= k for every N >= 1
    p.spec = k == 3 && s == 1;
    p.slabs = int(ceil_div(D, DWC_CV * 8));
    const int rows = p.Nout > N ? p.Nout : N;
    p.groups = int(ceil_div(rows, DWC_RL * DWC_MAX_RUN));
    if (p.groups > 65535 || int64_t(B) * p.groups > INT32_MAX) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d beyond the launch grid", what, B, N);
    p.run_out = int(ceil_div(p.Nout, p.groups * DWC_RL));
    p.run_in = int(ceil_div(N, p.groups * DWC_RL));
    if (int64_t(D) * (k + 1) > INT32_MAX) REFUSE(SFCVIT_EINVAL, "%s: D=%d too wide", what, D);
    p.ld = D * (k + 1);
    const int64_t parts = int64_t(B) * p.groups;                // < 2^31 partial rows of < 2^31 floats
    if (parts > (INT64_MAX / 4) / p.ld) REFUSE(SFCVIT_EINVAL, "%s: B=%d N=%d D=%d: the byte counts leave int64", what, B, N, D);
    p.ws_bytes = parts * p.ld * int64_t(sizeof(float));
    return p;
}

int dwconv_check_fwd(const DwconvPlan &p, const void *x, const void *w, const void *u) {
    if (p.err) return fail(p.err, "%s", p.msg);
    if (!x || !w || !u) return fail(SFCVIT_EINVAL, "dwconv1d_fwd: null pointer (x / w / u)");
    if (!aligned16(x) || !aligned16(u)) return fail(SFCVIT_EINVAL, "dwconv1d_fwd: x and u must be 16-byte aligned");
    return SFCVIT_OK;
}

int dwconv_check_bwd(const DwconvPlan &p, const void *du, const void *x, const void *w, const void *dx, const void *dw, const void *db,
                     const void *workspace, int64_t workspace_bytes) {
    if (p.err) return fail(p.err, "%s", p.msg);
    if (!du) return fail(SFCVIT_EINVAL, "dwconv1d_bwd: null pointer (du)");
    if (!dx && !dw && !db) return fail(SFCVIT_EINVAL, "dwconv1d_bwd: every output is NULL: nothing to compute");
    if (dx && !w) return fail(SFCVIT_EINVAL, "dwconv1d_bwd: null pointer (w, needed for dx)");
    if (dw && !x) return fail(SFCVIT_EINVAL, "dwconv1d_bwd: null pointer (x, needed for dw)");
    if (!aligned16(du) || !aligned16(x) || !aligned16(dx) || !aligned16(workspace))
        return fail(SFCVIT_EINVAL, "dwconv1d_bwd: du, x, dx and the workspace must be 16-byte aligned");
    if ((dw || db) && (!workspace || workspace_bytes < p.ws_bytes))
        return fail(SFCVIT_EINVAL, "dwconv1d_bwd: workspace of %lld bytes needed", (long long)p.ws_bytes);
    return SFCVIT_OK;
}

}  // namespace sfcvit

extern "C" int sfcvit_dwconv1d_out_len(int N, int k, int s) {
    const sfcvit::DwconvPlan p = sfcvit::dwconv_plan("dwconv1d_out_len", 1, N, 8, k, s);
    if (p.err) {
        sfcvit::fail(p.err, "%s", p.msg);
        return -1;
    }
    return p.Nout;
}

extern "C" int64_t sfcvit_dwconv1d_bwd_workspace(int B, int N, int D, int k, int s) {
    const sfcvit::DwconvPlan p = sfcvit::dwconv_plan("dwconv1d_bwd_workspace", B, N, D, k, s);
    return p.err ? 0 : p.ws_bytes;
}

extern "C" int sfcvit_last_dwconv_kernel(char *buf, int n) { return sfcvit::g_dwconv.read(buf, n); }
