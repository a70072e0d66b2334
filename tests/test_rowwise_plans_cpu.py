"""The row-wise family's host layer without a GPU: every entry point that used to check its arguments inline still refuses
before any HIP call, sfcvit_layernorm_bwd_ws is the plan's workspace, and the sanitizer program pins the plans themselves
(csrc/rowwise.cpp, check_rowwise in csrc/hostcheck/host_check.cpp)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd")
EINVAL, ELAUNCH = 1, 2


def test_old_entry_points_refuse_before_any_launch():
    """Every refusal is SFCVIT_EINVAL with a message that starts with the entry point's name, decided before any HIP call: this
    machine has no GPU, so a launch attempt would come back as a launch error (status 2), not as status 1."""
    from sfcvit import _lib
    lib = _lib.lib
    raw = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(raw) + 15) // 16 * 16                # 16-byte aligned host addresses: never dereferenced
    a, b, c, d, e, f, g, h, w = (p + (i << 12) for i in range(9))
    nan = float("nan")

    def refused(rc, prefix, word=""):
        msg = lib.sfcvit_last_error().decode()
        print(rc, msg)
        assert rc != ELAUNCH, msg
        assert rc == EINVAL and msg.startswith(prefix + ":") and word in msg, (rc, prefix, word, msg)

    def ln_fwd(x=a, gamma=b, beta=c, y=d, mean=e, rstd=f, M=8, D=16):
        return lib.sfcvit_layernorm_fwd(x, gamma, beta, y, mean, rstd, M, D, 1e-5, None)
    for n in ("x", "gamma", "beta", "y", "mean", "rstd"):
        refused(ln_fwd(**{n: None}), "layernorm_fwd", "null")
    for kw in (dict(M=0), dict(D=0), dict(D=12), dict(D=4104)):
        refused(ln_fwd(**kw), "layernorm_fwd", "D=%d" % kw.get("D", 16))
    for n, addr in dict(x=a, gamma=b, beta=c, y=d).items():
        refused(ln_fwd(**{n: addr + 8}), "layernorm_fwd", "alignment")

    def ln_bwd(dy=a, x=b, mean=e, rstd=f, gamma=c, dx_add=None, dx=d, dx_drop=None, p=0.0, dgamma=g, dbeta=h, M=8, D=16, ws=w):
        return lib.sfcvit_layernorm_bwd_drop(dy, x, mean, rstd, gamma, dx_add, dx, dx_drop, p, 7, None, dgamma, dbeta, None, 0, M, D, ws, None)
    for n in ("dy", "x", "mean", "rstd", "gamma", "dx", "dgamma", "dbeta", "ws"):
        refused(ln_bwd(**{n: None}), "layernorm_bwd", "null")
    for kw in (dict(M=0), dict(M=-2), dict(D=0), dict(D=12), dict(D=2056)):
        refused(ln_bwd(**kw), "layernorm_bwd", "D=%d" % kw.get("D", 16))
    for n, addr in dict(dy=a, x=b, gamma=c, dx=d, dx_add=a, dx_drop=a).items():
        refused(ln_bwd(**{n: addr + 8}), "layernorm_bwd", "alignment")
    for bad in (1.0, -0.1, nan):
        refused(ln_bwd(dx_drop=a + 2048, p=bad), "layernorm_bwd", "dropout p=")
    refused(lib.sfcvit_layernorm_bwd(None, b, e, f, c, None, d, g, h, 8, 16, w, None), "layernorm_bwd", "null")

    def colsum(x=a, M=8, N=16, ld=16, out=b, ws=c, ws_bytes=1 << 12):
        return lib.sfcvit_colsum(x, M, N, ld, out, 0, ws, ws_bytes, None)
    refused(colsum(x=None), "colsum", "null")
    refused(colsum(out=None), "colsum", "null")
    for kw in (dict(M=0), dict(N=0), dict(N=12), dict(ld=20), dict(ld=8)):
        refused(colsum(**kw), "colsum", "M=%d N=%d ld=%d" % (kw.get("M", 8), kw.get("N", 16), kw.get("ld", 16)))
    refused(colsum(x=a + 8), "colsum", "alignment")
    need = lib.sfcvit_colsum_workspace(8, 16)
    assert need == 1 * 16 * 4
    refused(colsum(ws=None), "colsum", "workspace")
    refused(colsum(ws_bytes=need - 1), "colsum", "workspace of %d bytes" % need)

    def transpose(src=a, R=8, C=16, lds=16, dst=b, ldd=8):
        return lib.sfcvit_transpose(src, R, C, lds, dst, ldd, None)
    refused(transpose(src=None), "transpose", "null")
    refused(transpose(dst=None), "transpose", "null")
    for kw in (dict(R=0), dict(C=0), dict(R=12), dict(C=12), dict(lds=20), dict(ldd=12), dict(lds=8), dict(R=16)):
        refused(transpose(**kw), "transpose", "multiples of 8")
    refused(transpose(src=a + 8), "transpose", "alignment")
    refused(transpose(dst=b + 2), "transpose", "alignment")
    refused(lib.sfcvit_transpose_batched(None, b, c, 1, None), "transpose_batched", "null")
    refused(lib.sfcvit_transpose_batched(a, None, c, 1, None), "transpose_batched", "null")
    refused(lib.sfcvit_transpose_batched(a, b, None, 1, None), "transpose_batched", "null")
    refused(lib.sfcvit_transpose_batched(a, b, c, 0, None), "transpose_batched", "no tiles")
    refused(lib.sfcvit_transpose_batched(a + 8, b, c, 1, None), "transpose_batched", "alignment")
    refused(lib.sfcvit_transpose_batched(a, b + 4, c, 1, None), "transpose_batched", "alignment")

    refused(lib.sfcvit_gelu_fwd(None, b, 16, None), "gelu_fwd")
    refused(lib.sfcvit_gelu_fwd(a, None, 16, None), "gelu_fwd")
    for n in (0, -8, 12):
        refused(lib.sfcvit_gelu_fwd(a, b, n, None), "gelu_fwd", "n=%d" % n)
        refused(lib.sfcvit_gelu_bwd(a, b, c, n, None), "gelu_bwd", "n=%d" % n)
    for args in ((None, b, c), (a, None, c), (a, b, None)):
        refused(lib.sfcvit_gelu_bwd(*args, 16, None), "gelu_bwd")

    def gd_fwd(x=a, y=b, rows=8, cols=16, p=0.1):
        return lib.sfcvit_gelu_drop_fwd(x, y, rows, cols, p, 7, None, None)

    def gd_bwd(dy=c, x=a, dx=b, rows=8, cols=16, p=0.1):
        return lib.sfcvit_gelu_drop_bwd(dy, x, dx, rows, cols, p, 7, None, None)
    refused(gd_bwd(dy=None), "gelu_drop_bwd", "null")
    for fn, name, outs in ((gd_fwd, "gelu_drop_fwd", ("x", "y")), (gd_bwd, "gelu_drop_bwd", ("x", "dx"))):
        for n in outs:
            refused(fn(**{n: None}), name, "rows=8 cols=16")
        for kw in (dict(rows=0), dict(cols=0), dict(cols=12)):
            refused(fn(**kw), name, "rows=%d cols=%d" % (kw.get("rows", 8), kw.get("cols", 16)))
        for bad in (1.0, -0.5, nan):
            refused(fn(p=bad), name, "dropout p=")

    refused(lib.sfcvit_dropout_mask(None, 8, 16, 0.1, 7, None), "dropout_mask")
    refused(lib.sfcvit_dropout_mask(a, 0, 16, 0.1, 7, None), "dropout_mask")
    refused(lib.sfcvit_dropout_mask(a, 8, 0, 0.1, 7, None), "dropout_mask")
    for bad in (1.0, -0.5, nan):
        refused(lib.sfcvit_dropout_mask(a, 8, 16, bad, 7, None), "dropout_mask")

    def soft_ce(logits=a, targets=b, loss=c, B=4, C=10, ld=16):
        return lib.sfcvit_soft_ce(logits, targets, loss, None, B, C, ld, 1.0, None)
    for n in ("logits", "targets", "loss"):
        refused(soft_ce(**{n: None}), "soft_ce", "null")
    for kw in (dict(B=0), dict(C=0), dict(ld=8)):
        refused(soft_ce(**kw), "soft_ce", "B=%d C=%d ld=%d" % (kw.get("B", 4), kw.get("C", 10), kw.get("ld", 16)))

    def sumsq(g_=a, n=64, out=b, ws=c):
        return lib.sfcvit_sumsq_accum(g_, n, 0, out, ws, None)
    for kw in (dict(g_=None), dict(out=None), dict(ws=None), dict(n=0), dict(n=-1)):
        refused(sumsq(**kw), "sumsq")
    refused(sumsq(g_=a + 8), "sumsq", "alignment")

    def adamw(n=64, **over):
        args = _lib.AdamWArgs()
        args.param, args.grad, args.master, args.m, args.v = a, b, c, d, e
        args.n, args.lr, args.beta1, args.beta2, args.eps, args.weight_decay, args.max_norm, args.grad_scale, args.step = (
            n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 1)
        for k_, v_ in over.items():
            setattr(args, k_, v_)
        return lib.sfcvit_adamw_step(ctypes.byref(args), None)
    refused(lib.sfcvit_adamw_step(None, None), "adamw", "null")
    for n in ("param", "grad", "master", "m", "v"):
        refused(adamw(**{n: None}), "adamw", "null")
        refused(adamw(**{n: a + (1 << 13) + 8}), "adamw", "aligned")
    refused(adamw(n=0), "adamw", "n=0")
    refused(adamw(n=-4), "adamw", "n=-4")
    refused(adamw(step=0), "adamw", "step=0")

    refused(lib.sfcvit_step_advance(None, 0.9, 0.999, 1, None), "step_advance", "16-byte aligned")
    refused(lib.sfcvit_step_advance(a + 8, 0.9, 0.999, 1, None), "step_advance", "16-byte aligned")

    buf = ctypes.create_string_buffer(96)
    assert lib.sfcvit_last_rowwise_kernel(buf, 96) == 0 and buf.value == b"none"      # nothing was launched


@pytest.mark.parametrize("M,D,blocks", [(50176, 768, 768), (36864, 1024, 512), (50176, 512, 512), (50176, 2048, 512), (10, 16, 3),
                                        (4, 8, 1), (2052, 768, 513)])
def test_layernorm_bwd_ws_is_the_plans(M, D, blocks):
    """[blocks][3][D] fp32 partials, blocks as check_rowwise pins them for ln_bwd_plan (the default switches)."""
    from sfcvit._lib import lib
    for name in ("SFCVIT_LN_COLS", "SFCVIT_LN_BLOCKS"):
        assert name not in os.environ
    got = lib.sfcvit_layernorm_bwd_ws(M, D)
    print(M, D, got)
    assert got == blocks * 3 * D * 4
    assert lib.sfcvit_layernorm_bwd_ws(0, D) == 0 and lib.sfcvit_layernorm_bwd_ws(M, 0) == 0 and lib.sfcvit_layernorm_bwd_ws(-1, D) == 0


def test_sanitizer_program_drives_the_rowwise_plans():
    """`make asan` builds and runs csrc/hostcheck/host_check.cpp with rowwise.cpp compiled in under
    -fsanitize=address,undefined; check_rowwise is part of it."""
    csrc = os.path.join(PKG, "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^ASAN_SRCS :=.*\browwise\.cpp\b", mk, re.M)
    assert "check_rowwise();" in open(os.path.join(csrc, "hostcheck", "host_check.cpp")).read()
    out = subprocess.run(["make", "-s", "-C", csrc, "asan"], capture_output=True, text=True, timeout=900)
    print(out.stdout[-500:], out.stderr[-2000:])
    assert out.returncode == 0 and "host_check ok" in out.stdout


def test_no_environment_read_outside_the_plans():
    """The launchers pick nothing themselves: the switches reach the kernels through RowwiseKnobs alone."""
    for name in ("rowwise.hip", "layernorm.hip", "optim.hip", "rowwise.cpp"):
        text = open(os.path.join(PKG, "csrc", name)).read()
        assert not re.search(r"\b(getenv|env_int|env_off|env_first|env_pair)\b", text), name
