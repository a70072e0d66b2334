"""Thin, allocation-only wrappers over the C ABI (include/sfcvit.h).

Every function here takes torch CUDA tensors, checks dtype / contiguity, allocates
outputs with torch's caching allocator and launches the HIP kernels on torch's
current stream.  There is no CPU path: a CPU tensor raises.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import lib, check

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
_BF16 = torch.bfloat16


class KernelTimer:
    """Optional per-launch timing with HIP events on the launching stream (bench.py's roofline
    leg).  Set `ops.TIMER = KernelTimer()`; every wrapper below then brackets its launch."""

    def __init__(self, only_prefix=None):
        self.records = {}
        self.only_prefix = only_prefix      # time only keys with this prefix (an event pair costs ~1 us of stream time)
        self.active = True                  # bench.py switches it per step: every launch of every 4th timed step is timed

    def launch(self, key, work, fn):
        if not self.active or (self.only_prefix and not key.startswith(self.only_prefix)):
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        if key.startswith("gemm "):         # key GEMM timings by the kernel symbol the library chose (as rocprofv3 names it)
            key = "gemm " + last_gemm_kernel()
        self.records.setdefault(key, []).append((e0, e1, work))
        return out

    def summary(self):
        """key -> dict(launches, ms_total, ms_avg, work_total); synchronises."""
        torch.cuda.synchronize()
        out = {}
        for key, recs in self.records.items():
            ms = sum(a.elapsed_time(b) for a, b, _ in recs)
            out[key] = {"launches": len(recs), "ms_total": ms, "ms_avg": ms / len(recs),
                        "work_total": float(sum(w for _, _, w in recs))}
        return out


TIMER = None
KERNEL_LOG = None     # tests: set to a list and every GEMM / attention launch appends the kernel symbol the library chose


def _last_kernel(fn):
    """What one of the library's sfcvit_last_*_kernel readers says: the kernel symbol as rocprofv3 names it, "none" before any."""
    buf = ctypes.create_string_buffer(96)
    fn(buf, 96)
    return buf.value.decode()


def last_gemm_kernel():
    return _last_kernel(lib.sfcvit_last_gemm_kernel)


def last_attn_kernel():
    return _last_kernel(lib.sfcvit_last_attn_kernel)


def last_rowwise_kernel():
    return _last_kernel(lib.sfcvit_last_rowwise_kernel)


def _launch(key, work, fn):
    out = fn() if TIMER is None else TIMER.launch(key, work, fn)
    if KERNEL_LOG is not None:
        if key.startswith("gemm "):
            KERNEL_LOG.append(last_gemm_kernel())
        elif key.startswith("attn"):
            KERNEL_LOG.append(last_attn_kernel())
    return out


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cur_dev(t, name):
    """One process per GPU: kernels are launched on the CURRENT device's current stream, and the library keeps
    per-(device, stream) state (tile-queue counters).  A tensor of another device would be dereferenced through the
    wrong context, so it is refused here rather than faulting there."""
    if t.device.index != torch.cuda.current_device():
        raise _lib.SfcvitError(f"{name}: tensor lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                               "wrap the call in torch.cuda.device(tensor.device) (one process per GPU is the supported layout)")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _need(t, dtype, name, dims=None):
    if not t.is_cuda:
        raise _lib.SfcvitError(f"{name}: the HIP path needs a CUDA (ROCm) tensor, got device {t.device}; "
                               "there is no CPU fallback")
    _cur_dev(t, name)
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{name}: expected {dims}-D, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _rows2d(t, dtype, name):
    """2-D, unit inner stride, arbitrary row stride (views of packed buffers are fine)."""
    if not t.is_cuda:
        raise _lib.SfcvitError(f"{name}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
    _cur_dev(t, name)
    if t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected 2-D {dtype} with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    return t


def _grad_outs(what, out, shapes, wanted, device, expected, name="out"):
    """The parameter gradients of a backward wrapper, one per entry of `shapes`: fp32, or -- with `out`, one tensor or a
    tuple with an entry per shape, e.g. views of a flat gradient buffer (None entries are allocated) -- bf16 written in
    place.  -> (the tensors, None where not wanted; whether they are bf16: the C calls' grad_bf16 flag)."""
    given = (None,) * len(shapes) if out is None else (out,) if torch.is_tensor(out) else out
    for t, shape in zip(given, shapes):
        if t is not None and (t.dtype != _BF16 or t.numel() != math.prod(shape) or not t.is_contiguous()):
            raise ValueError(f"{what} {name}: {expected} expected")
    gdt = torch.float32 if out is None else _BF16
    grads = [None if not want else t if t is not None else torch.empty(tuple(shape), device=device, dtype=gdt)
             for t, shape, want in zip(given, shapes, wanted)]
    return grads, out is not None


# ----------------------------------------------------------------------------
# GEMM
# ----------------------------------------------------------------------------
def auto_splitk(M, N, K):
    """Split K when the output has too few 128 x 128 tiles to fill 256 CUs at 2 workgroups each
    (weight-gradient shapes: 36-144 tiles, K = batch * tokens).  The split is chosen so that
    tiles * splits fills whole rounds of the 512 workgroup slots (864 workgroups = 1.69 rounds cost
    15 % against 1008 = 1.97), each k-range keeps >= 896 deep, and -- for outputs under 64 tiles,
    where sfcvit_gemm gives every XCD its own k-ranges -- is a multiple of 8."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if K < 2048:
        return 1
    if M % 256 == 0 and N % 256 == 0 and (M // 256) * (N // 256) <= 128:      # any K: the last K % 128 rows are one more slab
        # weight-gradient form of the 8-phase kernel: one workgroup per CU, tiles256 x splits <= 256
        s = min(64, 256 // ((M // 256) * (N // 256)))
        if s >= 2 and K // s >= 512:
            return s
    if tiles >= 256:
        return 1
    step = 8 if tiles < 64 else 1
    best, best_eff = 1, tiles / 512.0 if tiles < 512 else 1.0
    for s in range(max(2, step), 65, step):
        if K // s < 896:
            break
        wgs = tiles * s
        eff = wgs / (-(-wgs // 512) * 512)
        if eff > best_eff + 0.02:
            best, best_eff = s, eff
        if best_eff >= 0.93:
            break
    return best


# Device-resident step state (include/sfcvit.h, sfcvit_step_advance): None = seeds and Adam's step count live on the host
# (the default, as in the reference); a CUDA int32[8] tensor = every dropout site adds the device seed offset and AdamW
# reads lr / bias corrections from the device, so a whole training step can replay from one hipGraph
# (sfcvit.training.GraphedTrainStep).
STEP_STATE = None


def _seed_off():
    return ctypes.c_void_p(STEP_STATE.data_ptr()) if STEP_STATE is not None else None


_site = 0     # device-state mode: dropout sites of the current step drawn so far


def step_advance(state, beta1, beta2, seed_base):
    global _site
    _site = 0
    check(lib.sfcvit_step_advance(_p(state), beta1, beta2, seed_base & 0xFFFFFFFF, _stream()), "sfcvit_step_advance")


# Deferred reductions (include/sfcvit.h: sfcvit_reduce_defer / _flush).  Bias, LayerNorm-parameter and similar gradients are
# a main kernel + a 5-us fixed-order reduction over its partial rows; inside a backward pass nobody reads them before the pass
# ends when they are written into gradient slots (functional._slot marks those views), so their reductions are queued and
# run as ONE launch from an autograd end-of-pass callback (66 launches per ViT-B step become one).  A reducer that ships
# gradients mid-pass calls flush_deferred(end=False) first.  SFCVIT_DEFER_REDUCE=0 switches it off (A/B, tests).
import os as _os
DEFER_REDUCES = _os.environ.get("SFCVIT_DEFER_REDUCE", "1") != "0"
_defer = {"task": -1, "keep": []}
# autograd's id of the running backward pass (-1 outside one); a torch without it simply never defers / batches
graph_task_id = getattr(torch._C, "_current_graph_task_id", lambda: -1)


def flush_deferred(end=True):
    """Launch every queued reduction on the current stream (end=False: the backward pass goes on deferring)."""
    if lib.sfcvit_reduce_pending():
        check(lib.sfcvit_reduce_flush(_stream()), "sfcvit_reduce_flush")
    _defer["keep"].clear()
    if end:
        _defer["task"] = -1


class _Deferring:
    """with _Deferring(outputs, workspaces): the C calls inside queue their final reductions iff every output is a
    gradient slot and a backward pass is running; the workspaces then stay alive until the flush."""

    def __init__(self, outs, keep):
        self.on, self.keep = False, keep
        if DEFER_REDUCES and outs and all(getattr(t, "_sfcvit_deferrable", False) for t in outs):
            task = graph_task_id()
            if task >= 0:
                if _defer["task"] != task:
                    if lib.sfcvit_reduce_pending():      # a pass that died with reductions queued
                        lib.sfcvit_reduce_discard()
                    _defer["keep"].clear()
                    _defer["task"] = task
                    torch.autograd.Variable._execution_engine.queue_callback(flush_deferred)
                self.on = True

    def __enter__(self):
        if self.on:
            lib.sfcvit_reduce_defer(1)
        return self

    def __exit__(self, *exc):
        if self.on:
            lib.sfcvit_reduce_defer(0)
            _defer["keep"].extend(self.keep)
        return False


def next_seed():
    """32-bit dropout seed drawn on the host from torch's default CPU generator: reproducible under
    torch.manual_seed, no device synchronisation (kernels receive it as a plain argument)."""
    global _site
    if STEP_STATE is not None:
        # device-state mode: the by-value seed only tells the sites of one step apart (it is frozen into a captured graph);
        # what changes from step to step is the device offset the kernels add to it
        _site += 1
        return ((_site * 0x9E3779B1) & 0x7FFFFFFF) | 1
    return int(torch.randint(0, 0x7FFFFFFF, (), dtype=torch.int64)) * 2 + 1


def gemm(a, b, *, a_kmajor=False, b_kmajor=False, bias=None, act=ACT_NONE, residual=None,
         aux_in=None, dact=ACT_NONE, want_aux=False, out_f32=False, splitk=None, force_generic=False,
         dropout_p=0.0, dropout_seed=0, dact_scale=1.0, out=None, row_offset=0, colsum=None, actmask=None):
    """C[M,N] = epilogue(sum_k A(m,k) B(n,k)).  a: [M,K] (or [K,M] if a_kmajor),
    b: [N,K] (or [K,N] if b_kmajor), bf16.  Returns C (and the pre-activation if want_aux; and the column sums of C
    if `colsum` is True (fp32 [N]) or a bf16 [N] tensor to write them into, e.g. a bias-gradient slot).
    actmask: uint8 [M, N/8] bit matrix (bit n & 7 of byte n >> 3 <-> C[m, n] > 0): written with act = RELU, optionally
    read in place of aux_in with dact = RELU (sfcvit_gemm_args.actmask)."""
    _rows2d(a, _BF16, "gemm a")
    _rows2d(b, _BF16, "gemm b")
    M, K = (a.shape[1], a.shape[0]) if a_kmajor else (a.shape[0], a.shape[1])
    N, Kb = (b.shape[1], b.shape[0]) if b_kmajor else (b.shape[0], b.shape[1])
    if K != Kb:
        raise ValueError(f"gemm: contraction mismatch {K} vs {Kb}")
    if out is not None:
        c = _rows2d(out, torch.float32 if out_f32 else _BF16, "gemm out")
        if c.shape != (M, N):
            raise ValueError(f"gemm out: expected {(M, N)}, got {tuple(c.shape)}")
    else:
        c = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else _BF16)
    aux = torch.empty((M, N), device=a.device, dtype=_BF16) if want_aux else None
    args = _lib.GemmArgs()
    args.a, args.b, args.c = a.data_ptr(), b.data_ptr(), c.data_ptr()
    args.bias = _need(bias, _BF16, "gemm bias", 1).data_ptr() if bias is not None else None
    args.M, args.N, args.K = M, N, K
    args.lda, args.ldb, args.ldc = a.stride(0), b.stride(0), c.stride(0)
    if residual is not None:
        _rows2d(residual, _BF16, "gemm residual")
        args.residual, args.ldr = residual.data_ptr(), residual.stride(0)
    ldaux = N
    if aux_in is not None:
        _rows2d(aux_in, _BF16, "gemm aux_in")
        args.aux_in, ldaux = aux_in.data_ptr(), aux_in.stride(0)
    if aux is not None:
        args.aux_out = aux.data_ptr()
    args.ldaux = ldaux
    args.a_kmajor, args.b_kmajor = int(a_kmajor), int(b_kmajor)
    args.act, args.dact, args.c_is_f32 = act, dact, int(out_f32)
    args.dropout_p, args.dropout_seed, args.dact_scale = dropout_p, dropout_seed, dact_scale
    if dropout_p > 0.0 and STEP_STATE is not None:
        args.seed_off = STEP_STATE.data_ptr()
    args.row_offset = row_offset
    if actmask is not None:
        if actmask.dtype != torch.uint8 or actmask.dim() != 2 or actmask.shape[0] != M or actmask.shape[1] * 8 < N \
                or actmask.stride(1) != 1 or actmask.device != a.device:
            raise ValueError(f"gemm actmask: expected uint8 [{M}, >= {N // 8}] on {a.device}, got {actmask.dtype} {tuple(actmask.shape)}")
        args.actmask, args.ld_actmask = actmask.data_ptr(), actmask.stride(0)
    plain = (bias is None and residual is None and aux_in is None and not want_aux and act == 0 and dact == 0
             and dropout_p == 0.0)
    if splitk is None:
        splitk = auto_splitk(M, N, K) if plain else 1
    ws = None
    if splitk > 1:
        nbytes = lib.sfcvit_gemm_workspace(M, N, splitk)
        ws = torch.empty(nbytes, device=a.device, dtype=torch.uint8)
        args.workspace, args.workspace_bytes = ws.data_ptr(), nbytes
    args.splitk = splitk
    args.force_generic = int(force_generic)
    cs = None
    if colsum is not None and colsum is not False:
        cs = torch.empty(N, device=a.device, dtype=torch.float32) if colsum is True else colsum
        if cs.numel() != N or not cs.is_contiguous() or cs.dtype not in (torch.float32, _BF16):
            raise ValueError("gemm colsum: contiguous fp32 or bf16 [N] expected")
        nbytes = lib.sfcvit_gemm_colsum_workspace(M, N)
        ws = torch.empty(nbytes, device=a.device, dtype=torch.uint8)
        args.workspace, args.workspace_bytes = ws.data_ptr(), nbytes
        args.colsum_out, args.colsum_bf16 = cs.data_ptr(), int(cs.dtype == _BF16)
    key = "gemm %s" % {(False, False): "y=x.W^T (k-contig, k-contig)", (False, True): "dx=dy.W (k-contig, k-major)",
                       (True, True): "dW=dy^T.x (k-major, k-major)", (True, False): "(k-major, k-contig)"}[(a_kmajor, b_kmajor)]
    with _Deferring([colsum] if cs is not None and colsum is not True else [], [ws] if cs is not None else []):
        check(_launch(key, 2.0 * M * N * K, lambda: lib.sfcvit_gemm(ctypes.byref(args), _stream())), "sfcvit_gemm")
    if cs is not None:
        return (c, aux, cs) if want_aux else (c, cs)
    return (c, aux) if want_aux else c


def transpose(x):
    """[R, C] bf16 -> contiguous [C, R]."""
    _rows2d(x, _BF16, "transpose x")
    R, C = x.shape
    out = torch.empty((C, R), device=x.device, dtype=_BF16)
    check(lib.sfcvit_transpose(_p(x), R, C, x.stride(0), _p(out), R, _stream()), "sfcvit_transpose")
    return out


def transpose_batched(src_flat, dst_flat, tiles, n_tiles):
    """Every matrix of a flat bf16 buffer transposed in one launch; `tiles` = device uint8 tensor holding n_tiles
    sfcvit_transpose_tile records (FlatGradBuffer.transposed)."""
    _need(src_flat, _BF16, "transpose_batched src", 1)
    _need(dst_flat, _BF16, "transpose_batched dst", 1)
    if tiles.dtype != torch.uint8 or not tiles.is_cuda or tiles.numel() != 32 * n_tiles:
        raise ValueError("transpose_batched tiles: device uint8 tensor of 32 bytes per tile expected")
    check(lib.sfcvit_transpose_batched(_p(src_flat), _p(dst_flat), _p(tiles), n_tiles, _stream()), "sfcvit_transpose_batched")


def gemm_dx(dy, w, **kw):
    """dX[M, in] = dY[M, out] . W[out, in] (+ epilogue).  When the shape is eligible for the LDS-DMA
    kernel, W is transposed once (a few MB) so that both operands are k-contiguous; otherwise W is
    read k-major in place by the generic kernel."""
    M, K = dy.shape
    N = w.shape[1]
    # the persistent 8-phase kernel takes any M >= 192 (a last row tile that overlaps its predecessor); the LDS-DMA
    # ring kernel before it needs whole 256-row tiles
    if N % 128 == 0 and K % 32 == 0 and (M % 256 == 0 or (M >= 192 and N % 256 == 0 and K % 128 == 0 and K >= 256)):
        slot = getattr(w, "_sfcvit_slot", None)          # a parameter of a flat buffer: W^T from this backward pass's batch
        wt = slot[0].transposed(w) if slot is not None else None
        return gemm(dy, wt if wt is not None else transpose(w), **kw)
    return gemm(dy, w, b_kmajor=True, **kw)


def colsum(x, out=None):
    """Column sums [N]: fp32 (new tensor), or written as bf16 into `out` (e.g. a view of a flat gradient buffer)."""
    _rows2d(x, _BF16, "colsum x")
    if out is None:
        out = torch.empty(x.shape[1], device=x.device, dtype=torch.float32)
    elif out.dtype != _BF16 or out.numel() != x.shape[1] or not out.is_contiguous():
        raise ValueError("colsum out: contiguous bf16 [N] expected")
    nbytes = lib.sfcvit_colsum_workspace(x.shape[0], x.shape[1])
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    with _Deferring([out], [ws]):
        check(lib.sfcvit_colsum(_p(x), x.shape[0], x.shape[1], x.stride(0), _p(out), int(out.dtype == _BF16), _p(ws), nbytes,
                                _stream()), "sfcvit_colsum")
    return out


# ----------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps=1e-5):
    _need(x, _BF16, "layernorm x", 2)
    M, D = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    check(lib.sfcvit_layernorm_fwd(_p(x), _p(_need(gamma, _BF16, "gamma", 1)), _p(_need(beta, _BF16, "beta", 1)),
                                   _p(y), _p(mean), _p(rstd), M, D, eps, _stream()), "sfcvit_layernorm_fwd")
    return y, mean, rstd


def _layernorm_bwd(path, dy, x, mean, rstd, gamma, dx_add, drop_p, drop_seed, want_colsum, grad_out, scale=None):
    """layernorm_bwd (path = None), layernorm_bwd_path (path = (rows_per_image, path_rate, path_seed)) and layernorm_bwd_scale
    (path and scale = (branch, lam)): the checks, the buffers, the workspace of the plan the C call uses, the call -> dx, dgamma,
    dbeta, dx_drop (None if not written), dcol (None if not wanted) [, dlam with scale]."""
    what = "layernorm_bwd" if path is None else "layernorm_bwd_path" if scale is None else "layernorm_bwd_scale"
    _need(dy, _BF16, "layernorm dy", 2)
    _need(x, _BF16, "layernorm x", 2)
    if scale is not None:
        branch, lam = scale
        _need(branch, _BF16, "layernorm_bwd_scale branch", 2)
    M, D = x.shape
    if path is not None and (path[0] <= 0 or M % path[0]):
        raise ValueError(f"{what}: {M} rows are not whole images of {path[0]}")
    if scale is not None and (branch.shape != x.shape or dy.shape != x.shape or _need(lam, _BF16, "lam", 1).numel() != D):
        raise ValueError(f"{what}: dy, x and branch must be equal [M, D] and lam [D], got {tuple(dy.shape)} {tuple(x.shape)} "
                         f"{tuple(branch.shape)} {tuple(lam.shape)}")
    dx = torch.empty_like(x)
    dx_drop = torch.empty_like(x) if path is not None or drop_p > 0 else None
    if scale is None:
        (dg, db, dcol), bf16 = _grad_outs(what, grad_out, ((D,), (D,), (D,)), (True, True, want_colsum), x.device,
                                          "contiguous bf16 [D] tensors", name="out" if path is not None else "grad_out")   # the words each had
        dl = ()
    else:
        if grad_out is not None and len(grad_out) == 4:
            grad_out = (grad_out[0], grad_out[1], grad_out[3], grad_out[2])      # the optional entry last, as _grad_outs' callers have it
        (dg, db, *dl, dcol), bf16 = _grad_outs(what, grad_out, ((D,), (D,), (D,), (D,)), (True, True, True, want_colsum), x.device,
                                               "contiguous bf16 [D] tensors (dgamma, dbeta, colsum or None, dlam)")
    ws_bytes = lib.sfcvit_layernorm_bwd_ws if scale is None else lib.sfcvit_layernorm_bwd_scale_ws
    ws = torch.empty(ws_bytes(M, D), device=x.device, dtype=torch.uint8)
    if dx_add is not None:
        _need(dx_add, _BF16, "layernorm dx_add", 2)
    # (the scale form draws no flag at rate 0; the path form passes the offset whatever the rate)
    seed_off = _seed_off() if drop_p > 0 or (path is not None and (scale is None or path[1] > 0)) else None
    with _Deferring([dg, db, *dl] + ([dcol] if dcol is not None else []), [ws]):
        if path is None:
            rc = lib.sfcvit_layernorm_bwd_drop(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx_add), _p(dx), _p(dx_drop), drop_p,
                                               drop_seed, seed_off, _p(dg), _p(db), _p(dcol), int(bf16), M, D, _p(ws), _stream())
        elif scale is None:
            rc = lib.sfcvit_layernorm_bwd_path(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx_add), _p(dx), _p(dx_drop), drop_p,
                                               drop_seed, seed_off, _p(dg), _p(db), _p(dcol), int(bf16), M // path[0], path[0], D,
                                               _p(ws), path[1], path[2], _stream())
        else:
            rc = lib.sfcvit_layernorm_bwd_scale(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx_add), _p(branch), _p(lam), _p(dx),
                                                _p(dx_drop), drop_p, drop_seed, seed_off, _p(dg), _p(db), _p(dcol), _p(dl[0]), int(bf16),
                                                M // path[0], path[0], D, _p(ws), path[1], path[2], _stream())
        check(rc, "sfcvit_" + what)
    if KERNEL_LOG is not None:
        KERNEL_LOG.append(last_rowwise_kernel())
    return (dx, dg, db, dx_drop, dcol, *dl)


def layernorm_bwd(dy, x, mean, rstd, gamma, dx_add=None, drop_p=0.0, drop_seed=0, want_colsum=False, grad_out=None):
    """-> dx, dgamma, dbeta [, dx_drop when drop_p > 0] [, colsum of the outgoing gradient (dx_drop if
    drop_p > 0 else dx) when want_colsum].  dgamma / dbeta / colsum are fp32 [D], or -- with
    grad_out = (dgamma, dbeta, colsum-or-None) bf16 [D] tensors, e.g. views of a flat gradient buffer (None entries
    are allocated) -- written as bf16 in place."""
    dx, dg, db, dx_drop, dcol = _layernorm_bwd(None, dy, x, mean, rstd, gamma, dx_add, drop_p, drop_seed, want_colsum, grad_out)
    return (dx, dg, db) + ((dx_drop,) if drop_p > 0 else ()) + ((dcol,) if want_colsum else ())


# ----------------------------------------------------------------------------
# Stochastic depth (DropPath) on a residual site: one keep flag per image, a function of (seed, image index)
# ----------------------------------------------------------------------------
def drop_path_keep(B, rate, seed, device="cuda"):
    """bool [B]: which images a site with `seed` keeps at `rate` -- column 0 of the dropout mask of that seed, which is what
    the kernels regenerate (without STEP_STATE's device offset: tests and debugging)."""
    return dropout_mask(B, 8, rate, seed, device)[:, 0] > 0


def _add_layernorm_fwd(what, branch, x, lam, gamma, beta, B, rate, seed, eps):
    """add_layernorm_path_fwd and add_layernorm_scale_fwd (what = "add_layernorm_scale", with lam): the checks, the buffers, the
    call -> (s, y, mean, rstd)."""
    scaled = what == "add_layernorm_scale"
    _need(branch, _BF16, f"{what} branch", 2)
    _need(x, _BF16, f"{what} x", 2)
    M, D = x.shape
    if branch.shape != x.shape or B <= 0 or M % B:
        raise ValueError(f"{what}: branch {tuple(branch.shape)} and x {tuple(x.shape)} must be equal [B * N, D] with B = {B}")
    if scaled and _need(lam, _BF16, "lam", 1).numel() != D:
        raise ValueError(f"{what}: lam must be [D] = [{D}], got {tuple(lam.shape)}")
    s, y = torch.empty_like(x), torch.empty_like(x)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    head = (_p(branch), _p(x)) + ((_p(lam),) if scaled else ())
    tail = (_p(_need(gamma, _BF16, "gamma", 1)), _p(_need(beta, _BF16, "beta", 1)), _p(s), _p(y), _p(mean), _p(rstd), B, M // B, D, eps,
            rate, seed)
    if scaled:                                  # no flag is drawn at rate 0: the device seed offset only with one
        rc = lib.sfcvit_add_layernorm_scale_fwd(*head, *tail, _seed_off() if rate > 0 else None, _stream())
    else:
        rc = lib.sfcvit_add_layernorm_path_fwd(*head, *tail, _seed_off(), _stream())
    check(rc, f"sfcvit_{what}_fwd")
    if KERNEL_LOG is not None:
        KERNEL_LOG.append(last_rowwise_kernel())
    return s, y, mean, rstd


def add_layernorm_path_fwd(branch, x, gamma, beta, B, rate, seed, eps=1e-5):
    """s = bf16(x + c[b] * branch), LayerNorm(s) -> (s, y, mean, rstd); c[b] = keep(b) / (1 - rate) per image b = row // (M / B).
    branch, x: bf16 [M, D], M = B * tokens.  A dropped image's rows of s are the bits of x."""
    return _add_layernorm_fwd("add_layernorm_path", branch, x, None, gamma, beta, B, rate, seed, eps)


def layernorm_bwd_path(dy, x, mean, rstd, gamma, rows_per_image, path_rate, path_seed, dx_add=None, drop_p=0.0, drop_seed=0,
                       want_colsum=False, grad_out=None):
    """layernorm_bwd for a residual site with stochastic depth -> dx, dgamma, dbeta, dx_drop [, colsum of dx_drop].  dx_drop, the
    gradient entering the sub-layer, is always returned (also at drop_p = 0): image b = row // rows_per_image gets
    dx * dropout mask / ((1 - drop_p)(1 - path_rate)) when the site of `path_seed` kept it, zeros otherwise.  dx (the residual
    path), dgamma and dbeta are those of layernorm_bwd; grad_out as there."""
    dx, dg, db, dx_drop, dcol = _layernorm_bwd((rows_per_image, path_rate, path_seed), dy, x, mean, rstd, gamma, dx_add, drop_p,
                                               drop_seed, want_colsum, grad_out)
    return (dx, dg, db, dx_drop) + ((dcol,) if want_colsum else ())


# ----------------------------------------------------------------------------
# LayerScale residual site (pre-norm layers): the site above with a per-channel scale on the branch
# ----------------------------------------------------------------------------
def add_layernorm_scale_fwd(branch, x, lam, gamma, beta, B, rate=0.0, seed=0, eps=1e-5):
    """s = bf16(x + (c[b] * lam[d]) * branch), LayerNorm(s) -> (s, y, mean, rstd); lam bf16 [D]; c[b] = keep(b) / (1 - rate) per
    image b = row // (M / B), 1 at rate = 0 (no flag is drawn).  branch, x: bf16 [M, D], M = B * tokens.  A dropped image's rows
    of s are the bits of x."""
    return _add_layernorm_fwd("add_layernorm_scale", branch, x, lam, gamma, beta, B, rate, seed, eps)


def layernorm_bwd_scale(dy, x, mean, rstd, gamma, branch, lam, rows_per_image, path_rate=0.0, path_seed=0, dx_add=None, drop_p=0.0,
                        drop_seed=0, want_colsum=False, grad_out=None):
    """layernorm_bwd_path with the channel scale of a LayerScale site -> dx, dgamma, dbeta, dx_drop, dlam [, colsum of dx_drop].
    dx is the gradient of s (and of the residual input); dx_drop = dx * lam * dropout mask / ((1 - drop_p)(1 - path_rate)) for
    kept images, zeros for dropped ones, is the gradient entering the sub-layer; dlam[d] = sum over rows of the stored dx * c[b]
    * branch.  grad_out = (dgamma, dbeta, colsum-or-None, dlam) bf16 [D] tensors (None entries are allocated): written in place
    as bf16, e.g. views of a flat gradient buffer -- dlam may be a row of a [2, D] parameter's slot."""
    dx, dg, db, dx_drop, dcol, dl = _layernorm_bwd((rows_per_image, path_rate, path_seed), dy, x, mean, rstd, gamma, dx_add, drop_p,
                                                   drop_seed, want_colsum, grad_out, scale=(branch, lam))
    return (dx, dg, db, dx_drop, dl) + ((dcol,) if want_colsum else ())


# ----------------------------------------------------------------------------
# QK-norm: LayerNorm over the head dim on the q and k thirds of a packed projection, in place
# ----------------------------------------------------------------------------
def qk_norm_plan(M, n_heads, hp):
    """The launch geometry of both QK-norm kernels for M rows: dict(rows_per_wg, slot_groups, blocks, vpl).  No GPU call."""
    out = (ctypes.c_int32 * 4)()
    check(lib.sfcvit_qk_norm_plan(M, n_heads, hp, out), "sfcvit_qk_norm_plan")
    return dict(rows_per_wg=out[0], slot_groups=out[1], blocks=out[2], vpl=out[3])


def _qk_norm_args(what, qkv, params, n_heads, head_dim):
    """-> (M, hp) of a packed buffer [.., 3 * H * hp] and its parameters [4, head_dim], checked."""
    if qkv.dim() not in (2, 3):
        raise ValueError(f"{what}: [M, 3 * H * hp] or [B, N, 3 * H * hp] expected, got shape {tuple(qkv.shape)}")
    _need(qkv, _BF16, f"{what} qkv")
    _need(params, _BF16, f"{what} params", 2)
    D3 = qkv.shape[-1]
    if n_heads <= 0 or D3 % (3 * n_heads):
        raise ValueError(f"{what}: packed width {D3} is not 3 * n_heads * head_dim for n_heads = {n_heads}")
    hp = D3 // (3 * n_heads)
    if tuple(params.shape) != (4, head_dim):
        raise ValueError(f"{what}: params must be [4, head_dim] = [4, {head_dim}] (q_weight, q_bias, k_weight, k_bias), got "
                         f"{tuple(params.shape)}")
    return qkv.numel() // D3, hp


def qk_norm_fwd(qkv, params, n_heads, head_dim, eps=1e-6):
    """LayerNorm over the head_dim real columns of every query and key head row of qkv [.., 3 * H * hp] bf16, IN PLACE (columns
    head_dim .. hp - 1, the zero padding of a head dim the kernels do not have, become +0; v is untouched) -> raw [M, 2 * H * hp]:
    the bits of q | k as they were, which qk_norm_bwd needs.  params: bf16 [4, head_dim], rows q_weight, q_bias, k_weight,
    k_bias, shared by all heads."""
    M, hp = _qk_norm_args("qk_norm_fwd", qkv, params, n_heads, head_dim)
    raw = torch.empty((M, 2 * n_heads * hp), device=qkv.device, dtype=_BF16)
    check(lib.sfcvit_qk_norm_fwd(_p(qkv), _p(raw), _p(params), M, n_heads, head_dim, hp, eps, _stream()), "sfcvit_qk_norm_fwd")
    if KERNEL_LOG is not None:
        KERNEL_LOG.append(last_rowwise_kernel())
    return raw


def qk_norm_bwd(dqkv, raw, params, n_heads, head_dim, eps=1e-6, colsum=None, grad_out=None, vsum=None):
    """The backward of qk_norm_fwd, IN PLACE on the q and k thirds of dqkv as the attention backward left them (v untouched,
    padded columns +0) -> (dqkv, dparams, colsum or None).  dparams [4, head_dim]: fp32 (new), or -- with grad_out, a bf16
    [4, head_dim] tensor such as a gradient slot -- written there.  colsum: None; True -> fp32 [2 * H * hp] (new), the column
    sums of the new dq | dk; or a contiguous fp32 / bf16 tensor to write into.  With vsum (fp32 [H * hp], the v third of
    attention_bwd's colsum) the colsum tensor is [3 * H * hp] and its last third receives vsum: the whole in_proj bias gradient
    in one place.  The reductions run now, in a fixed order (never queued: the slot they end in is complete when this returns
    to the stream)."""
    M, hp = _qk_norm_args("qk_norm_bwd", dqkv, params, n_heads, head_dim)
    Da = n_heads * hp
    _need(raw, _BF16, "qk_norm_bwd raw", 2)
    if tuple(raw.shape) != (M, 2 * Da):
        raise ValueError(f"qk_norm_bwd: raw must be [M, 2 * H * hp] = {(M, 2 * Da)}, got {tuple(raw.shape)}")
    (dP,), dp_bf16 = _grad_outs("qk_norm_bwd", grad_out, ((4, head_dim),), (True,), dqkv.device, "a contiguous bf16 [4, head_dim] tensor",
                                name="grad_out")
    width = 3 * Da if vsum is not None else 2 * Da
    if vsum is not None:
        _need(vsum, torch.float32, "qk_norm_bwd vsum", 1)
        if vsum.numel() != Da or colsum is None or colsum is False:
            raise ValueError(f"qk_norm_bwd: vsum must be fp32 [H * hp] = [{Da}] and needs colsum")
    cs = None
    if colsum is not None and colsum is not False:
        cs = torch.empty(width, device=dqkv.device, dtype=torch.float32) if colsum is True else colsum
        if not cs.is_cuda or cs.numel() != width or not cs.is_contiguous() or cs.dtype not in (torch.float32, _BF16):
            raise ValueError(f"qk_norm_bwd colsum: contiguous fp32 or bf16 [{width}] expected")
    ws = torch.empty(lib.sfcvit_qk_norm_bwd_ws(M, n_heads, hp), device=dqkv.device, dtype=torch.uint8)
    check(lib.sfcvit_qk_norm_bwd(_p(dqkv), _p(raw), _p(params), _p(dP), int(dp_bf16), _p(cs), int(cs is not None and cs.dtype == _BF16),
                                 _p(vsum), _p(ws), M, n_heads, head_dim, hp, eps, _stream()), "sfcvit_qk_norm_bwd")
    if KERNEL_LOG is not None:
        KERNEL_LOG.append(last_rowwise_kernel())
    return dqkv, dP, cs


# ----------------------------------------------------------------------------
# RoPE: rotary position embedding on the q and k thirds of a packed projection, in place
# ----------------------------------------------------------------------------
class RopeTable:
    """The (cos, sin) table of a rotary position embedding: fp32 [N, head_dim / 2, 2] (CPU; row n, pair p holds (c, s);
    sfcvit.rope builds them), shared by the heads, the batch, and q and k.  Validated once on the host -- shape, dtype, every
    entry finite -- and uploaded once per device, where the copy stays put (graph capture replays it).  Not a parameter: it
    receives no gradient and enters no state_dict."""

    def __init__(self, table):
        if not isinstance(table, torch.Tensor) or table.is_cuda or table.dtype != torch.float32 or table.dim() != 3 \
                or table.shape[2] != 2 or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError("RopeTable: a CPU fp32 [N, head_dim / 2, 2] tensor of (cos, sin) pairs is expected "
                             "(sfcvit.rope builds them)")
        if not bool(torch.isfinite(table).all()):
            raise ValueError("RopeTable: the table holds a non-finite entry")
        self.table = table.detach().contiguous().clone()
        self.n_tokens, self.head_dim = int(table.shape[0]), 2 * int(table.shape[1])
        self._dev = {}

    def on(self, device):
        """The table on `device`, uploaded at the first request."""
        key = torch.device(device)
        if key.type == "cuda" and key.index is None:
            key = torch.device("cuda", torch.cuda.current_device())
        if key not in self._dev:
            self._dev[key] = self.table.to(key)
        return self._dev[key]

    def __repr__(self):
        return f"RopeTable(N={self.n_tokens}, head_dim={self.head_dim})"


def rope_plan(B, N, n_heads, hp):
    """The launch geometry of both RoPE kernels for B images of N tokens: dict(tokens_per_wg, batch_per_wg, rows_per_wg,
    slot_groups, blocks, vpl).  No GPU call."""
    out = (ctypes.c_int32 * 5)()
    check(lib.sfcvit_rope_plan(B, N, n_heads, hp, out), "sfcvit_rope_plan")
    return dict(tokens_per_wg=out[0], batch_per_wg=out[1], rows_per_wg=out[0] * out[1], slot_groups=out[2], blocks=out[3], vpl=out[4])


def _rope_args(what, qkv, table, n_heads):
    """-> (device table, B, N, hd, hp) of a packed buffer [M, 3 * H * hp] or [B, N, 3 * H * hp] and a RopeTable, checked."""
    if qkv.dim() not in (2, 3):
        raise ValueError(f"{what}: [M, 3 * H * hp] or [B, N, 3 * H * hp] expected, got shape {tuple(qkv.shape)}")
    _need(qkv, _BF16, f"{what} qkv")
    if not isinstance(table, RopeTable):
        raise ValueError(f"{what}: table must be an ops.RopeTable")
    D3 = qkv.shape[-1]
    if n_heads <= 0 or D3 % (3 * n_heads):
        raise ValueError(f"{what}: packed width {D3} is not 3 * n_heads * head_dim for n_heads = {n_heads}")
    hp, M, N = D3 // (3 * n_heads), qkv.numel() // D3, table.n_tokens
    if qkv.dim() == 3 and qkv.shape[1] != N:
        raise ValueError(f"{what}: table for {N} tokens on a sequence of {qkv.shape[1]}")
    if M % N:
        raise ValueError(f"{what}: {M} rows are no whole number of sequences of the table's {N} tokens")
    if table.head_dim > hp:
        raise ValueError(f"{what}: table for head dim {table.head_dim} on a packed head width of {hp}")
    return table.on(qkv.device), M // N, N, table.head_dim, hp


def rope_fwd(qkv, table, n_heads):
    """Rotates the channel pairs (2 p, 2 p + 1) of every query and key head row of qkv [.., 3 * H * hp] bf16 IN PLACE by the
    table's (c, s) of the row's token, y0 = x0 c - x1 s, y1 = x0 s + x1 c (columns head_dim .. hp - 1, the zero padding of a head
    dim the kernels do not have, become +0; v is untouched) -> qkv.  table: an ops.RopeTable for N tokens; row m uses its row
    m mod N.  Nothing is kept for the backward."""
    t, B, N, hd, hp = _rope_args("rope_fwd", qkv, table, n_heads)
    check(lib.sfcvit_rope_fwd(_p(qkv), _p(t), B, N, n_heads, hd, hp, _stream()), "sfcvit_rope_fwd")
    if KERNEL_LOG is not None:
        KERNEL_LOG.append(last_rowwise_kernel())
    return qkv


def rope_bwd(dqkv, table, n_heads, colsum=None, vsum=None):
    """The backward of rope_fwd, the transposed rotation, IN PLACE on the q and k thirds of dqkv as the attention backward left
    them (v untouched, padded columns +0) -> (dqkv, colsum or None).  colsum: None -- one launch, no workspace; True -> fp32
    [2 * H * hp] (new), the column sums of the new dq | dk; or a contiguous fp32 / bf16 tensor to write into.  With vsum (fp32
    [H * hp], the v third of attention_bwd's colsum) the colsum tensor is [3 * H * hp] and its last third receives vsum: the
    whole in_proj bias gradient in one place.  The reduction runs now, in a fixed order (never queued)."""
    t, B, N, hd, hp = _rope_args("rope_bwd", dqkv, table, n_heads)
    Da = n_heads * hp
    width = 3 * Da if vsum is not None else 2 * Da
    if vsum is not None:
        _need(vsum, torch.float32, "rope_bwd vsum", 1)
        if vsum.numel() != Da or colsum is None or colsum is False:
            raise ValueError(f"rope_bwd: vsum must be fp32 [H * hp] = [{Da}] and needs colsum")
    cs = ws = None
    if colsum is not None and colsum is not False:
        cs = torch.empty(width, device=dqkv.device, dtype=torch.float32) if colsum is True else colsum
        if not cs.is_cuda or cs.numel() != width or not cs.is_contiguous() or cs.dtype not in (torch.float32, _BF16):
            raise ValueError(f"rope_bwd colsum: contiguous fp32 or bf16 [{width}] expected")
        ws = torch.empty(lib.sfcvit_rope_bwd_ws(B, N, n_heads, hp), device=dqkv.device, dtype=torch.uint8)
    check(lib.sfcvit_rope_bwd(_p(dqkv), _p(t), _p(cs), int(cs is not None and cs.dtype == _BF16), _p(vsum), _p(ws), B, N, n_heads,
                              hd, hp, _stream()), "sfcvit_rope_bwd")
    if KERNEL_LOG is not None:
        KERNEL_LOG.append(last_rowwise_kernel())
    return dqkv, cs


# ----------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------
SUPPORTED_HEAD_DIMS = (64, 128, 192, 256)


def _attn_dims(D3, n_heads):
    """(D, head dim) of a packed q|k|v projection; the kernels exist for head dims 64 (any N) and 128 / 192 / 256 (any N
    with any_length=True: whole-sequence kernels up to N = 256 / 192 / 160, streaming kernels beyond; without it those
    limits are refusals)."""
    if D3 % 3 or (D3 // 3) % n_heads:
        raise ValueError(f"attention: packed width {D3} is not 3 * n_heads * head_dim for n_heads = {n_heads}")
    D = D3 // 3
    hd = D // n_heads
    if hd not in SUPPORTED_HEAD_DIMS:
        raise ValueError(f"attention: head dim {hd} (= {D} / {n_heads}) is not supported; supported: {SUPPORTED_HEAD_DIMS}")
    return D, hd


def padded_head_dim(hd):
    """The kernel head dim a model head dim runs on: itself when supported, else the next supported one (zero-padded
    q / k / v columns change neither q k^T nor p v; the softmax scale stays 1 / sqrt(hd)); None above the largest."""
    for s in sorted(SUPPORTED_HEAD_DIMS):
        if hd <= s:
            return s
    return None


def attention_fwd(qkv, n_heads, dropout_p=0.0, dropout_seed=0, scale=None, any_length=False):
    """qkv [B, N, 3*D] bf16 -> out [B, N, D] bf16, lse [B, H, N] fp32.  scale: softmax scale, default 1 / sqrt(head dim).
    any_length: head dims 128 / 192 / 256 at any N (sfcvit_attention_fwd_any); otherwise the whole-sequence limits hold."""
    _need(qkv, _BF16, "attention qkv", 3)
    B, N, D3 = qkv.shape
    D, hd = _attn_dims(D3, n_heads)
    out = torch.empty((B, N, D), device=qkv.device, dtype=_BF16)
    lse = torch.empty((B, n_heads, N), device=qkv.device, dtype=torch.float32)
    a = _lib.AttnArgs()
    a.qkv, a.out, a.lse = qkv.data_ptr(), out.data_ptr(), lse.data_ptr()
    a.B, a.N, a.H, a.hd, a.scale = B, N, n_heads, hd, (1.0 / math.sqrt(hd) if scale is None else float(scale))
    a.dropout_p, a.dropout_seed = dropout_p, dropout_seed
    if dropout_p > 0.0 and STEP_STATE is not None:
        a.seed_off = STEP_STATE.data_ptr()
    fn = lib.sfcvit_attention_fwd_any if any_length else lib.sfcvit_attention_fwd
    check(_launch("attn_fwd_kernel", 4.0 * B * n_heads * N * N * hd,
                  lambda: fn(ctypes.byref(a), _stream())), "sfcvit_attention_fwd" + ("_any" if any_length else ""))
    return out, lse


def attention_bwd(qkv, out, lse, dout, n_heads, dropout_p=0.0, dropout_seed=0, colsum=None, scale=None, any_length=False):
    """-> dqkv [, column sums of dqkv over all B * N rows = the in_proj bias gradient: colsum=True -> fp32 [3D] (new
    tensor), or a bf16 [3D] tensor to write into (e.g. a slot of the flat gradient buffer)].  any_length: as in
    attention_fwd (sfcvit_attention_bwd_any)."""
    _need(dout, _BF16, "attention dout", 3)
    B, N, D3 = qkv.shape
    D, hd = _attn_dims(D3, n_heads)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, n_heads, N), device=qkv.device, dtype=torch.float32)
    a = _lib.AttnArgs()
    a.qkv, a.out, a.lse, a.dout = qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr()
    a.dqkv, a.delta = dqkv.data_ptr(), delta.data_ptr()
    a.B, a.N, a.H, a.hd, a.scale = B, N, n_heads, hd, (1.0 / math.sqrt(hd) if scale is None else float(scale))
    a.dropout_p, a.dropout_seed = dropout_p, dropout_seed
    if dropout_p > 0.0 and STEP_STATE is not None:
        a.seed_off = STEP_STATE.data_ptr()
    cs = None
    if colsum is not None and colsum is not False:
        cs = torch.empty(D3, device=qkv.device, dtype=torch.float32) if colsum is True else colsum
        if cs.numel() != D3 or not cs.is_contiguous() or cs.dtype not in (torch.float32, _BF16):
            raise ValueError("attention_bwd colsum: contiguous fp32 or bf16 [3D] expected")
        nbytes = lib.sfcvit_attention_colsum_workspace(B, N, n_heads, hd)
        ws = torch.empty(nbytes, device=qkv.device, dtype=torch.uint8)
        a.colsum_part, a.colsum_part_bytes = ws.data_ptr(), nbytes
        a.colsum_out, a.colsum_bf16 = cs.data_ptr(), int(cs.dtype == _BF16)
    with _Deferring([colsum] if cs is not None and colsum is not True else [], [ws] if cs is not None else []):
        fn = lib.sfcvit_attention_bwd_any if any_length else lib.sfcvit_attention_bwd
        check(_launch("attn_bwd", 10.0 * B * n_heads * N * N * hd,
                      lambda: fn(ctypes.byref(a), _stream())), "sfcvit_attention_bwd" + ("_any" if any_length else ""))
    return dqkv if cs is None else (dqkv, cs)


class AttentionMask:
    """An additive attention mask [N, N] (fp32, CPU; entries finite or -inf, shared by all batches and heads) validated by
    sfcvit_attention_mask_blocks, with its block map (one byte per 64 x 64 block: 0 skip, 1 mixed, 2 all zero).  Built once
    on the host; the device copies of mask and map are made once per device and stay put (graph capture replays them).
    ValueError, with the library's message, for NaN, +inf, a row that hides every key, N < 1 or N > 4096."""

    def __init__(self, mask):
        if not isinstance(mask, torch.Tensor) or mask.is_cuda or mask.dtype != torch.float32 or mask.dim() != 2 or mask.shape[0] != mask.shape[1]:
            raise ValueError("AttentionMask: a CPU fp32 [N, N] tensor is expected (sfcvit.masks builds them)")
        self.mask = mask.contiguous()
        self.n_tokens = N = int(mask.shape[0])
        nb = (max(N, 1) + 63) // 64
        self.block_map = torch.zeros((nb, nb), dtype=torch.uint8)
        rc = lib.sfcvit_attention_mask_blocks(ctypes.c_void_p(self.mask.data_ptr()), N, ctypes.c_void_p(self.block_map.data_ptr()))
        if rc != 0:
            raise ValueError(lib.sfcvit_last_error().decode(errors="replace"))
        self.total_blocks = nb * nb
        self.visited_blocks = int((self.block_map != 0).sum())
        self._dev = {}

    def on(self, device):
        """(mask, block map) on `device`, uploaded at the first request."""
        key = torch.device(device)
        if key.type == "cuda" and key.index is None:
            key = torch.device("cuda", torch.cuda.current_device())
        if key not in self._dev:
            self._dev[key] = (self.mask.to(key), self.block_map.to(key))
        return self._dev[key]

    def __repr__(self):
        return f"AttentionMask(N={self.n_tokens}, blocks {self.visited_blocks}/{self.total_blocks})"


def as_attention_mask(mask, n_tokens=None):
    """None, or the AttentionMask of an attention mask in any of nn.TransformerEncoder.forward's forms: an AttentionMask as
    it is, a float additive [N, N] tensor (finite or -inf), or a bool tensor with True = may NOT attend (validated and
    uploaded now: callers that run more than once convert once).  ValueError for a size other than n_tokens."""
    if mask is None:
        return None
    if not isinstance(mask, AttentionMask):
        from . import masks
        mask = torch.as_tensor(mask)
        mask = AttentionMask(masks.from_bool(mask) if mask.dtype == torch.bool else mask.detach().to("cpu", torch.float32))
    if n_tokens is not None and mask.n_tokens != n_tokens:
        raise ValueError(f"attention mask for {mask.n_tokens} tokens on a sequence of {n_tokens}")
    return mask


def _masked_args(qkv, n_heads, mask, block_map, dropout_p, dropout_seed, scale, what):
    _need(qkv, _BF16, f"{what} qkv", 3)
    B, N, D3 = qkv.shape
    if D3 % 3 or (D3 // 3) % n_heads:
        raise ValueError(f"{what}: packed width {D3} is not 3 * n_heads * head_dim for n_heads = {n_heads}")
    hd = D3 // 3 // n_heads
    nb = (N + 63) // 64
    if tuple(_need(mask, torch.float32, f"{what} mask", 2).shape) != (N, N):
        raise ValueError(f"{what}: mask must be [N, N] = {(N, N)}, got {tuple(mask.shape)}")
    if tuple(_need(block_map, torch.uint8, f"{what} block_map", 2).shape) != (nb, nb):
        raise ValueError(f"{what}: block_map must be {(nb, nb)}, got {tuple(block_map.shape)}")
    a = _lib.AttnMaskArgs()
    a.qkv, a.mask, a.block_map = qkv.data_ptr(), mask.data_ptr(), block_map.data_ptr()
    a.B, a.N, a.H, a.hd, a.scale = B, N, n_heads, hd, (1.0 / math.sqrt(hd) if scale is None else float(scale))
    a.dropout_p, a.dropout_seed = dropout_p, dropout_seed
    if dropout_p > 0.0 and STEP_STATE is not None:
        a.seed_off = STEP_STATE.data_ptr()
    return a, B, N, D3 // 3, hd


def attention_masked_fwd(qkv, n_heads, mask, block_map, dropout_p=0.0, dropout_seed=0, scale=None):
    """attention_fwd with an additive mask: scores scale * q k^T + mask.  mask [N, N] fp32 and block_map [nb, nb] uint8 are
    the device tensors of an AttentionMask (AttentionMask.on(device)).  Head dim 64 only, 1 <= N <= 4096.  The lse
    includes the mask."""
    a, B, N, D, hd = _masked_args(qkv, n_heads, mask, block_map, dropout_p, dropout_seed, scale, "attention_masked_fwd")
    out = torch.empty((B, N, D), device=qkv.device, dtype=_BF16)
    lse = torch.empty((B, n_heads, N), device=qkv.device, dtype=torch.float32)
    a.out, a.lse = out.data_ptr(), lse.data_ptr()
    check(_launch("attn_masked_fwd", 4.0 * B * n_heads * N * N * hd,
                  lambda: lib.sfcvit_attention_masked_fwd(ctypes.byref(a), _stream())), "sfcvit_attention_masked_fwd")
    return out, lse


def attention_masked_bwd(qkv, out, lse, dout, n_heads, mask, block_map, dropout_p=0.0, dropout_seed=0, colsum=None, scale=None):
    """-> dqkv [, column sums of dqkv as in attention_bwd]."""
    a, B, N, D, hd = _masked_args(qkv, n_heads, mask, block_map, dropout_p, dropout_seed, scale, "attention_masked_bwd")
    _need(dout, _BF16, "attention_masked_bwd dout", 3)
    _need(out, _BF16, "attention_masked_bwd out", 3)
    _need(lse, torch.float32, "attention_masked_bwd lse", 3)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, n_heads, N), device=qkv.device, dtype=torch.float32)
    a.out, a.lse, a.dout, a.dqkv, a.delta = out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), delta.data_ptr()
    cs = None
    if colsum is not None and colsum is not False:
        cs = torch.empty(3 * D, device=qkv.device, dtype=torch.float32) if colsum is True else colsum
        if cs.numel() != 3 * D or not cs.is_contiguous() or cs.dtype not in (torch.float32, _BF16):
            raise ValueError("attention_masked_bwd colsum: contiguous fp32 or bf16 [3D] expected")
        nbytes = lib.sfcvit_attention_colsum_workspace(B, N, n_heads, hd)
        ws = torch.empty(nbytes, device=qkv.device, dtype=torch.uint8)
        a.colsum_part, a.colsum_part_bytes = ws.data_ptr(), nbytes
        a.colsum_out, a.colsum_bf16 = cs.data_ptr(), int(cs.dtype == _BF16)
    with _Deferring([colsum] if cs is not None and colsum is not True else [], [ws] if cs is not None else []):
        check(_launch("attn_masked_bwd", 10.0 * B * n_heads * N * N * hd,
                      lambda: lib.sfcvit_attention_masked_bwd(ctypes.byref(a), _stream())), "sfcvit_attention_masked_bwd")
    return dqkv if cs is None else (dqkv, cs)


class AttentionBiasIndex:
    """The static half of a relative position bias: an int32 [N, N] bucket index (CPU; values in [-1, n_buckets), -1 = the
    pair is hidden, shared by all batches and heads; sfcvit.relpos builds them) validated by sfcvit_attention_bias_blocks,
    with its block map (one byte per 64 x 64 block: 0 skip, 1 visited) and its inverted index (CSR: offsets [T + 1],
    positions = i * N + j ascending per bucket) for the table gradient.  Built once on the host; the device copies are made
    once per device and stay put (graph capture replays them).  ValueError, with the library's message, for an entry outside
    [-1, n_buckets), a row that hides every key, N outside 1 .. 1024 or n_buckets outside 1 .. 4096."""

    def __init__(self, index, n_buckets):
        if not isinstance(index, torch.Tensor) or index.is_cuda or index.dtype != torch.int32 or index.dim() != 2 \
                or index.shape[0] != index.shape[1]:
            raise ValueError("AttentionBiasIndex: a CPU int32 [N, N] tensor is expected (sfcvit.relpos builds them)")
        self.index = index.contiguous()
        self.n_tokens = N = int(index.shape[0])
        self.n_buckets = T = int(n_buckets)
        nb = (max(N, 1) + 63) // 64
        self.block_map = torch.zeros((nb, nb), dtype=torch.uint8)
        self.offsets = torch.zeros(max(T, 0) + 1, dtype=torch.int32)
        positions = torch.zeros(max(N * N, 1), dtype=torch.int32)
        rc = lib.sfcvit_attention_bias_blocks(ctypes.c_void_p(self.index.data_ptr()), N, T, ctypes.c_void_p(self.block_map.data_ptr()),
                                              ctypes.c_void_p(self.offsets.data_ptr()), ctypes.c_void_p(positions.data_ptr()))
        if rc != 0:
            raise ValueError(lib.sfcvit_last_error().decode(errors="replace"))
        self.positions = positions[:int(self.offsets[-1])].clone()
        self.total_blocks = nb * nb
        self.visited_blocks = int((self.block_map != 0).sum())
        self._dev = {}

    def on(self, device):
        """(index, block map, offsets, positions) on `device`, uploaded at the first request."""
        key = torch.device(device)
        if key.type == "cuda" and key.index is None:
            key = torch.device("cuda", torch.cuda.current_device())
        if key not in self._dev:
            self._dev[key] = tuple(t.to(key) for t in (self.index, self.block_map, self.offsets, self.positions))
        return self._dev[key]

    def __repr__(self):
        return (f"AttentionBiasIndex(N={self.n_tokens}, buckets={self.n_buckets}, "
                f"blocks {self.visited_blocks}/{self.total_blocks})")


def _bias_args(qkv, n_heads, table, bias_index, dropout_p, dropout_seed, scale, what):
    _need(qkv, _BF16, f"{what} qkv", 3)
    if not isinstance(bias_index, AttentionBiasIndex):
        raise ValueError(f"{what}: bias_index must be an ops.AttentionBiasIndex")
    B, N, D3 = qkv.shape
    if D3 % 3 or (D3 // 3) % n_heads:
        raise ValueError(f"{what}: packed width {D3} is not 3 * n_heads * head_dim for n_heads = {n_heads}")
    hd = D3 // 3 // n_heads
    if bias_index.n_tokens != N:
        raise ValueError(f"{what}: bias index for {bias_index.n_tokens} tokens on a sequence of {N}")
    if tuple(_need(table, torch.float32, f"{what} table", 2).shape) != (n_heads, bias_index.n_buckets):
        raise ValueError(f"{what}: table must be [H, T] = {(n_heads, bias_index.n_buckets)}, got {tuple(table.shape)}")
    index, block_map, offsets, positions = bias_index.on(qkv.device)
    a = _lib.AttnBiasArgs()
    a.qkv, a.index, a.table, a.block_map = qkv.data_ptr(), index.data_ptr(), table.data_ptr(), block_map.data_ptr()
    a.offsets, a.positions = offsets.data_ptr(), positions.data_ptr()
    a.T, a.visited_blocks = bias_index.n_buckets, bias_index.visited_blocks
    a.B, a.N, a.H, a.hd, a.scale = B, N, n_heads, hd, (1.0 / math.sqrt(hd) if scale is None else float(scale))
    a.dropout_p, a.dropout_seed = dropout_p, dropout_seed
    if dropout_p > 0.0 and STEP_STATE is not None:
        a.seed_off = STEP_STATE.data_ptr()
    return a, B, N, D3 // 3, hd


def attention_bias_fwd(qkv, n_heads, table, bias_index, dropout_p=0.0, dropout_seed=0, scale=None):
    """attention_fwd with a relative position bias per head: scores scale * q k^T + table[h, index[i, j]], hidden where the
    index is -1.  table: fp32 [H, T] on the device; bias_index: an AttentionBiasIndex for N tokens and T buckets.  Head dim
    64 only, 1 <= N <= 1024, T <= 4096.  -> out [B, N, D] bf16, lse [B, H, N] fp32 (the lse includes the bias)."""
    a, B, N, D, hd = _bias_args(qkv, n_heads, table, bias_index, dropout_p, dropout_seed, scale, "attention_bias_fwd")
    out = torch.empty((B, N, D), device=qkv.device, dtype=_BF16)
    lse = torch.empty((B, n_heads, N), device=qkv.device, dtype=torch.float32)
    a.out, a.lse = out.data_ptr(), lse.data_ptr()
    check(_launch("attn_bias_fwd", 4.0 * B * n_heads * N * N * hd,
                  lambda: lib.sfcvit_attention_bias_fwd(ctypes.byref(a), _stream())), "sfcvit_attention_bias_fwd")
    return out, lse


def attention_bias_bwd(qkv, out, lse, dout, n_heads, table, bias_index, dropout_p=0.0, dropout_seed=0, colsum=None, scale=None,
                       table_grad=True):
    """-> dqkv, dtable [H, T] fp32 [, column sums of dqkv as in attention_bwd].  table_grad=False (a frozen table): the
    table-gradient kernels are not launched and dtable is None."""
    a, B, N, D, hd = _bias_args(qkv, n_heads, table, bias_index, dropout_p, dropout_seed, scale, "attention_bias_bwd")
    _need(dout, _BF16, "attention_bias_bwd dout", 3)
    _need(out, _BF16, "attention_bias_bwd out", 3)
    _need(lse, torch.float32, "attention_bias_bwd lse", 3)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, n_heads, N), device=qkv.device, dtype=torch.float32)
    a.out, a.lse, a.dout, a.dqkv, a.delta = out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), delta.data_ptr()
    dtable = None
    if table_grad:
        dtable = torch.empty((n_heads, bias_index.n_buckets), device=qkv.device, dtype=torch.float32)
        nws = lib.sfcvit_attention_bias_workspace(B, N, n_heads, bias_index.visited_blocks)
        workspace = torch.empty(nws, device=qkv.device, dtype=torch.uint8)
        a.dtable, a.workspace, a.workspace_bytes = dtable.data_ptr(), workspace.data_ptr(), nws
    cs = None
    if colsum is not None and colsum is not False:
        cs = torch.empty(3 * D, device=qkv.device, dtype=torch.float32) if colsum is True else colsum
        if cs.numel() != 3 * D or not cs.is_contiguous() or cs.dtype not in (torch.float32, _BF16):
            raise ValueError("attention_bias_bwd colsum: contiguous fp32 or bf16 [3D] expected")
        nbytes = lib.sfcvit_attention_colsum_workspace(B, N, n_heads, hd)
        ws = torch.empty(nbytes, device=qkv.device, dtype=torch.uint8)
        a.colsum_part, a.colsum_part_bytes = ws.data_ptr(), nbytes
        a.colsum_out, a.colsum_bf16 = cs.data_ptr(), int(cs.dtype == _BF16)
    with _Deferring([colsum] if cs is not None and colsum is not True else [], [ws] if cs is not None else []):
        # S and dP of every visited block are recomputed for the table gradient: 4 of the backward's 10 N^2 hd flops again
        check(_launch("attn_bias_bwd", (14.0 if table_grad else 10.0) * B * n_heads * N * N * hd,
                      lambda: lib.sfcvit_attention_bias_bwd(ctypes.byref(a), _stream())), "sfcvit_attention_bias_bwd")
    return (dqkv, dtable) if cs is None else (dqkv, dtable, cs)


def _probe_args(qkv, lse, n_heads, scale, what):
    _need(qkv, _BF16, f"{what} qkv", 3)
    _need(lse, torch.float32, f"{what} lse", 3)
    B, N, D3 = qkv.shape
    D, hd = _attn_dims(D3, n_heads)
    if tuple(lse.shape) != (B, n_heads, N):
        raise ValueError(f"{what}: lse must be [B, H, N] = {(B, n_heads, N)}, got {tuple(lse.shape)}")
    a = _lib.AttnProbeArgs()
    a.qkv, a.lse = qkv.data_ptr(), lse.data_ptr()
    a.B, a.N, a.H, a.hd, a.scale = B, N, n_heads, hd, (1.0 / math.sqrt(hd) if scale is None else float(scale))
    return a, B, N, hd


def attention_probs(qkv, lse, n_heads, scale=None, head_mean=False, dtype=torch.float32, out=None):
    """The attention map softmax(scale q k^T) rebuilt from the packed projection and the lse attention_fwd returned for it
    (same scale): [B, H, N, N], or with head_mean the mean over heads [B, N, N] (nn.MultiheadAttention's
    average_attn_weights=True).  dtype: torch.float32 or torch.bfloat16.  out: a contiguous tensor of that shape and dtype
    to write into."""
    a, B, N, hd = _probe_args(qkv, lse, n_heads, scale, "attention_probs")
    if dtype not in (torch.float32, _BF16):
        raise TypeError(f"attention_probs: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
    shape = (B, N, N) if head_mean else (B, n_heads, N, N)
    if out is None:
        out = torch.empty(shape, device=qkv.device, dtype=dtype)
    elif tuple(_need(out, dtype, "attention_probs out").shape) != shape:
        raise ValueError(f"attention_probs out: expected shape {shape}, got {tuple(out.shape)}")
    a.probs, a.probs_is_bf16, a.head_mean = out.data_ptr(), int(dtype == _BF16), int(bool(head_mean))
    check(_launch("attn_probe_map", 2.0 * B * n_heads * N * N * hd,
                  lambda: lib.sfcvit_attention_probs(ctypes.byref(a), _stream())), "sfcvit_attention_probs")
    return out


ATTENTION_STATS = ("distance", "sequence_distance", "entropy", "mass")


def attention_stats(qkv, lse, n_heads, pos=None, scale=None, out=None):
    """Per query row, without forming the N x N map: a dict of [B, H, N] fp32 tensors
         "distance"           sum_j P_ij ||pos_i - pos_j||   (only with pos: [N, 2] fp32 token centres, analysis.token_positions)
         "sequence_distance"  sum_j P_ij |i - j|
         "entropy"            -sum_j P_ij ln P_ij            (nats)
         "mass"               sum_j P_ij                     (~1: these scores against the forward's lse)
    out: dict name -> contiguous fp32 [B, H, N] tensor to write into (missing names are allocated)."""
    a, B, N, hd = _probe_args(qkv, lse, n_heads, scale, "attention_stats")
    if pos is not None:
        if tuple(_need(pos, torch.float32, "attention_stats pos", 2).shape) != (N, 2):
            raise ValueError(f"attention_stats: pos must be [N, 2] = {(N, 2)}, got {tuple(pos.shape)}")
        a.pos = pos.data_ptr()
    res = {}
    for name, field in zip(ATTENTION_STATS, ("dist_rows", "seq_rows", "ent_rows", "mass_rows")):
        if name == "distance" and pos is None:
            continue
        t = (out or {}).get(name)
        if t is None:
            t = torch.empty((B, n_heads, N), device=qkv.device, dtype=torch.float32)
        elif tuple(_need(t, torch.float32, f"attention_stats out[{name}]").shape) != (B, n_heads, N):
            raise ValueError(f"attention_stats out[{name}]: expected shape {(B, n_heads, N)}, got {tuple(t.shape)}")
        setattr(a, field, t.data_ptr())
        res[name] = t
    check(_launch("attn_probe_stats", 2.0 * B * n_heads * N * N * hd,
                  lambda: lib.sfcvit_attention_stats(ctypes.byref(a), _stream())), "sfcvit_attention_stats")
    return res


# ----------------------------------------------------------------------------
# tokenizer
# ----------------------------------------------------------------------------
def last_tokenizer_kernel():
    """Name of the tokenizer kernel this thread launched last (sfcvit_last_tokenizer_kernel), "none" before any."""
    return _last_kernel(lib.sfcvit_last_tokenizer_kernel)


class TileDesc:
    """Device copy + host facts of a tile descriptor (sfcvit_tile_descriptors): the tokenizer's pixel table turned out
    to be 16 x 16 pixel tiles (or 256-pixel strips), so the coalesced kernels of csrc/patch_embed_tiled.hip apply."""

    def __init__(self, desc_host, device):
        self.mode, self.ncls = int(desc_host[0]), int(desc_host[1])
        self.cnt = [int(desc_host[6 + c + 1] - desc_host[6 + c]) for c in range(self.ncls)]
        self.dev = torch.from_numpy(desc_host.copy()).to(device)


def tile_descriptor(pix_host, img_w, device):
    """pix_host: numpy int32 [N, P] (the host pixel table) -> TileDesc, or None when the tokens are not tiles / strips."""
    import numpy as np
    N, P = pix_host.shape
    pix_host = np.ascontiguousarray(pix_host, dtype=np.int32)
    cap = 16 + 2 * N + 2 * 8 * 256
    out = np.zeros(cap, dtype=np.int32)
    n = lib.sfcvit_tile_descriptors(ctypes.c_void_p(pix_host.ctypes.data), N, P, int(img_w), ctypes.c_void_p(out.ctypes.data), cap)
    if n < 0:
        check(n, "sfcvit_tile_descriptors")
    return TileDesc(out[:n], device) if n > 0 else None


def _pe_desc(a, desc):
    if desc is not None:
        a.desc, a.desc_ncls = desc.dev.data_ptr(), desc.ncls
        for c, n in enumerate(desc.cnt):
            a.desc_cnt[c] = n


def _pe_args(x, pix, n_tokens, P, D):
    if not x.is_cuda:
        raise _lib.SfcvitError("patch_embed: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
    _cur_dev(x, "patch_embed x")
    if x.dtype not in (torch.float32, _BF16) or x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"patch_embed x: expected contiguous [B,C,H,W] fp32/bf16, got {x.dtype} {tuple(x.shape)}")
    _need(pix, torch.int32, "patch_embed pix", 2)
    B, C, H, W = x.shape
    a = _lib.PatchEmbedArgs()
    a.x, a.pix = x.data_ptr(), pix.data_ptr()
    a.B, a.C, a.HW, a.N, a.P, a.D = B, C, H * W, n_tokens, P, D
    a.x_is_bf16 = int(x.dtype == _BF16)
    return a


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def hier_resample_concat(levels):
    """levels: list of [B, N_l, D] bf16 (first = the target length) -> [B, N_0, L * D] bf16: torch's linear interpolation
    (align_corners=False) of every other level to N_0 tokens + the concatenation, one kernel (multi_hilbert.py:33-38)."""
    for t in levels:
        _need(t, _BF16, "hier_resample_concat level", 3)
    B, N0, D = levels[0].shape
    if any(t.shape[0] != B or t.shape[2] != D for t in levels):
        raise ValueError("hier_resample_concat: levels must share batch and width")
    L = len(levels)
    out = torch.empty((B, N0, L * D), device=levels[0].device, dtype=_BF16)
    n = (ctypes.c_int32 * L)(*[t.shape[1] for t in levels])
    check(_launch("hier_resample", 0.0, lambda: lib.sfcvit_hier_resample_concat(_ptr_array(levels), n, L, B, N0, D, _p(out), _stream())),
          "sfcvit_hier_resample_concat")
    return out


def hier_resample_concat_bwd(dout, n_tokens, D):
    """dout [B, N_0, L * D] bf16 -> list of d y_l [B, N_l, D] bf16."""
    _need(dout, _BF16, "hier_resample_concat dout", 3)
    B, N0, LD = dout.shape
    L = len(n_tokens)
    if LD != L * D or n_tokens[0] != N0:
        raise ValueError("hier_resample_concat_bwd: shape mismatch")
    grads = [torch.empty((B, nl, D), device=dout.device, dtype=_BF16) for nl in n_tokens]
    n = (ctypes.c_int32 * L)(*n_tokens)
    check(_launch("hier_resample_bwd", 0.0, lambda: lib.sfcvit_hier_resample_concat_bwd(_p(dout), n, L, B, N0, D, _ptr_array(grads), _stream())),
          "sfcvit_hier_resample_concat_bwd")
    return grads


GATHER_TILES = _os.environ.get("SFCVIT_GATHER_TILES", "1") != "0"     # 0: the per-pixel gather kernel for tile tables too (A/B)


def gather_order(pix_host):
    """Tokens sorted by their lowest pixel offset (numpy int32 [N]): the order in which the gather kernels pair tokens, so
    that horizontally adjacent 16 x 16 tiles -- whose rows share 128-byte lines -- go to one workgroup.  A property of the
    pixel table: the tokenizer computes it once, with the table (a performance hint only, see sfcvit_tokens_gather)."""
    import numpy as np
    return np.argsort(pix_host.min(axis=1), kind="stable").astype(np.int32)


def _mix_ptrs(mix, x, name):
    """(perm, rec) pointers of a batch mix (sfcvit.training.BatchMix, or anything with int32 `perm` [B] and `rec` [8] on
    x's device) after checking them against the image batch."""
    if x.dtype != torch.float32:
        raise TypeError(f"{name}: a mix needs an fp32 image batch (what a loader delivers), got {x.dtype}; "
                        "mixing a bf16 batch is not supported")
    perm = _need(mix.perm, torch.int32, f"{name} mix.perm", 1)
    rec = _need(mix.rec, torch.int32, f"{name} mix.rec", 1)
    if perm.numel() != x.shape[0] or rec.numel() != 8:
        raise ValueError(f"{name}: mix is for a batch of {perm.numel()} images (rec of {rec.numel()} words), "
                         f"the batch has {x.shape[0]}")
    return _p(perm), _p(rec)


def gather_tokens(x, pix, desc=None, order=None, mix=None):
    """x [B,C,H,W] fp32/bf16, pix [N,P] int32 (device) -> tokens [B*N, P*C (rounded up to 8)] bf16 in the reference's
    feature order kk * C + c: the A operand of the projection GEMM and of its weight gradient.
    desc: TileDesc of the table or None; order: device int32 [N] from gather_order() or None (tokens paired as numbered).
    16 x 16 tiles of an fp32 image go to sfcvit_tokens_gather_tiles, everything else to sfcvit_tokens_gather.
    mix: a batch mix (sfcvit.training.BatchMix) applied on the way to bf16 (sfcvit_tokens_gather_mix: MixUp / CutMix of
    image b with image mix.perm[b], fp32 images only); None = the plain gather."""
    N, P = pix.shape
    a = _pe_args(x, pix, N, P, 8)
    ld = (P * a.C + 7) // 8 * 8
    if order is not None:
        _need(order, torch.int32, "gather order", 1)
    tiles = GATHER_TILES and desc is not None and desc.mode == 1 and P == 256 and a.C <= 4 and x.dtype == torch.float32
    origin = desc.dev[16 + N:16 + 2 * N] if tiles else None
    if mix is not None:
        perm, rec = _mix_ptrs(mix, x, "gather_tokens")
        tokens = torch.empty((a.B * N, ld), device=x.device, dtype=_BF16)
        check(_launch("tokens_gather", 0.0, lambda: lib.sfcvit_tokens_gather_mix(_p(x), _p(pix), _p(order), _p(origin), perm, rec, a.B, a.C,
                                                                               x.shape[2], x.shape[3], N, P, _p(tokens), ld, _stream())),
              "sfcvit_tokens_gather_mix")
        return tokens
    tokens = torch.empty((a.B * N, ld), device=x.device, dtype=_BF16)
    if tiles:
        check(_launch("tokens_gather", 0.0, lambda: lib.sfcvit_tokens_gather_tiles(_p(x), _p(pix), _p(order), _p(origin), a.B, a.C, x.shape[2],
                                                                                 x.shape[3], N, _p(tokens), ld, _stream())),
              "sfcvit_tokens_gather_tiles")
        return tokens
    check(_launch("tokens_gather", 0.0, lambda: lib.sfcvit_tokens_gather(_p(x), a.x_is_bf16, _p(pix), _p(order), a.B, a.C, a.HW, N, P,
                                                                       _p(tokens), ld, _stream())), "sfcvit_tokens_gather")
    return tokens


def mix_images(x, mix):
    """x [B,C,H,W] fp32 -> the mixed batch (new tensor, fp32): MixUp / CutMix of image b with image mix.perm[b] as
    mix.rec says, one pass (sfcvit_mix_images).  For the tokenizers that do not go through gather_tokens."""
    if not x.is_cuda:
        raise _lib.SfcvitError(f"mix_images: the HIP path needs a CUDA (ROCm) tensor, got device {x.device}; there is no CPU fallback")
    if x.dim() != 4:
        raise ValueError(f"mix_images x: expected [B,C,H,W], got shape {tuple(x.shape)}")
    perm, rec = _mix_ptrs(mix, x, "mix_images")
    x = _need(x if x.is_contiguous() else x.contiguous(), torch.float32, "mix_images x", 4)
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    check(_launch("mix_images", 0.0, lambda: lib.sfcvit_mix_images(_p(x), perm, rec, _p(out), B, C, H, W, _stream())), "sfcvit_mix_images")
    return out


def patch_embed_is_tiled(desc, P, D):
    """Whether patch_embed_fwd / _bwd run the tiled kernels (csrc/tokenizer.cpp: patch_embed_plan) for a tile descriptor
    `desc` (or None), P pixels per token and D output columns."""
    return desc is not None and P == 256 and D % 256 == 0


def patch_embed_fwd(x, pix, w, bias, desc=None):
    """x [B,C,H,W] fp32/bf16, pix [N,P] int32 (device), w [D, P*C] bf16 -> [B, N, D] bf16.
    desc: TileDesc (tile_descriptor) or None; with it the tiled kernel runs where patch_embed_is_tiled says so."""
    N, P = pix.shape
    D = w.shape[0]
    _need(w, _BF16, "patch_embed w", 2)
    a = _pe_args(x, pix, N, P, D)
    y = torch.empty((x.shape[0], N, D), device=x.device, dtype=_BF16)
    nbytes = lib.sfcvit_patch_embed_workspace(a.B, a.C, N, P, D, 0)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    a.w, a.y, a.workspace, a.workspace_bytes = w.data_ptr(), y.data_ptr(), ws.data_ptr(), nbytes
    a.bias = _need(bias, _BF16, "patch_embed bias", 1).data_ptr() if bias is not None else None
    _pe_desc(a, desc)
    check(_launch("pe_fwd_kernel", 2.0 * a.B * N * P * a.C * D,
                  lambda: lib.sfcvit_patch_embed_fwd(ctypes.byref(a), _stream())), "sfcvit_patch_embed_fwd")
    return y


def patch_embed_bwd(x, pix, dy, D, want_bias=True, desc=None):
    """-> dW fp32 [D, P*C], dbias fp32 [D]."""
    N, P = pix.shape
    _need(dy, _BF16, "patch_embed dy", 3)
    a = _pe_args(x, pix, N, P, D)
    dw = torch.empty((D, P * a.C), device=x.device, dtype=torch.float32)
    db = torch.empty(D, device=x.device, dtype=torch.float32) if want_bias else None
    nbytes = lib.sfcvit_patch_embed_workspace(a.B, a.C, N, P, D, 1)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    a.y, a.dw, a.dbias = dy.data_ptr(), dw.data_ptr(), (db.data_ptr() if want_bias else None)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    _pe_desc(a, desc)
    check(_launch("pe_bwd_kernel", 2.0 * a.B * N * P * a.C * D,
                  lambda: lib.sfcvit_patch_embed_bwd(ctypes.byref(a), _stream())), "sfcvit_patch_embed_bwd")
    return dw, db


def hier_tokenizer_supported(n_levels, D, C, pixels_per_token):
    """Is (levels, level width, channels, pixels per token of each level) inside the fused hierarchical kernel's
    envelope (sfcvit_hier_tokenizer_supported)?  Host arithmetic only."""
    if not 1 <= n_levels <= 4 or len(pixels_per_token) != n_levels:
        return False
    P = (ctypes.c_int32 * 4)(*pixels_per_token)
    return bool(lib.sfcvit_hier_tokenizer_supported(n_levels, D, C, P))


def hier_tokenizer_fwd(x, pix_list, w_list, b_list, wf, bf):
    """Fused hierarchical tokenizer (csrc/hier_tokenizer.hip): x [B,C,H,W] fp32/bf16; per level pix [N,P_l] int32,
    w [D,P_l*C] bf16, b [D] bf16 or None; wf [L*D,L*D], bf [L*D] or None -> (y [B,N,L*D] bf16, h [B,N,L*D] bf16).
    wf = None: gather + level projections + concatenation only -> (None, h); the caller applies the fusion Linear."""
    L = len(pix_list)
    if not x.is_cuda:
        raise _lib.SfcvitError("hier_tokenizer: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
    _cur_dev(x, "hier_tokenizer x")
    if x.dtype not in (torch.float32, _BF16) or x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"hier_tokenizer x: expected contiguous [B,C,H,W] fp32/bf16, got {x.dtype} {tuple(x.shape)}")
    B, C, H, W = x.shape
    N = pix_list[0].shape[0]
    D = w_list[0].shape[0]
    E = L * D
    a = _lib.HierArgs()
    a.x, a.x_is_bf16 = x.data_ptr(), int(x.dtype == _BF16)
    flops = 2.0 * B * N * E * E if wf is not None else 0.0
    for l in range(L):
        pix = _need(pix_list[l], torch.int32, "hier_tokenizer pix", 2)
        if pix.shape[0] != N:
            raise ValueError("hier_tokenizer: every level must have the same token count")
        w = _need(w_list[l], _BF16, "hier_tokenizer w", 2)
        if tuple(w.shape) != (D, pix.shape[1] * C):
            raise ValueError(f"hier_tokenizer: level {l} weight {tuple(w.shape)}, expected {(D, pix.shape[1] * C)}")
        a.pix[l], a.w[l], a.P[l] = pix.data_ptr(), w.data_ptr(), pix.shape[1]
        a.b[l] = _need(b_list[l], _BF16, "hier_tokenizer b", 1).data_ptr() if b_list[l] is not None else None
        flops += 2.0 * B * N * pix.shape[1] * C * D
    y = None
    if wf is not None:
        _need(wf, _BF16, "hier_tokenizer wf", 2)
        if tuple(wf.shape) != (E, E):
            raise ValueError(f"hier_tokenizer: fusion weight {tuple(wf.shape)}, expected {(E, E)}")
        a.wf = wf.data_ptr()
        a.bf = _need(bf, _BF16, "hier_tokenizer bf", 1).data_ptr() if bf is not None else None
        y = torch.empty((B, N, E), device=x.device, dtype=_BF16)
        a.y = y.data_ptr()
    h = torch.empty((B, N, E), device=x.device, dtype=_BF16)
    a.h = h.data_ptr()
    a.B, a.C, a.HW, a.N, a.L, a.D = B, C, H * W, N, L, D
    check(_launch("hier_fwd_kernel", flops, lambda: lib.sfcvit_hier_tokenizer_fwd(ctypes.byref(a), _stream())),
          "sfcvit_hier_tokenizer_fwd")
    return y, h


# ----------------------------------------------------------------------------
# depth-wise conv1d along the token sequence (TokenAggregator.dw)
# ----------------------------------------------------------------------------
def last_dwconv_kernel():
    return _last_kernel(lib.sfcvit_last_dwconv_kernel)


def dwconv1d_out_len(N, k, stride=1):
    n = lib.sfcvit_dwconv1d_out_len(N, k, stride)
    if n < 0:
        check(1, "sfcvit_dwconv1d_out_len")
    return n


def _dw_weight(w, D):
    """[D, k] or nn.Conv1d's [D, 1, k], contiguous bf16 -> k."""
    if w.dim() not in (2, 3) or w.shape[0] != D or (w.dim() == 3 and w.shape[1] != 1):
        raise ValueError(f"dwconv1d weight: [{D}, k] or [{D}, 1, k] expected, got {tuple(w.shape)}")
    _need(w, _BF16, "dwconv1d weight")
    return w.shape[-1]


def dwconv1d_fwd(x, w, bias=None, stride=1):
    """u[b, n, d] = bias[d] + sum_t w[d, t] x[b, n * stride + t - k // 2, d] on x [B, N, D] bf16 -> [B, Nout, D] bf16."""
    _need(x, _BF16, "dwconv1d x", 3)
    B, N, D = x.shape
    k = _dw_weight(w, D)
    if bias is not None and _need(bias, _BF16, "dwconv1d bias", 1).numel() != D:
        raise ValueError(f"dwconv1d bias: [{D}] expected")
    u = torch.empty((B, dwconv1d_out_len(N, k, stride), D), device=x.device, dtype=_BF16)
    _launch("dwconv1d_fwd", 2.0 * x.numel() + 2.0 * u.numel(),
            lambda: check(lib.sfcvit_dwconv1d_fwd(_p(x), _p(w), _p(bias), _p(u), B, N, D, k, stride, _stream()), "sfcvit_dwconv1d_fwd"))
    return u


def dwconv1d_bwd(du, x, w, stride=1, want_dx=True, want_dw=True, want_db=True, out=None):
    """-> (dx [B, N, D] bf16, dw like w, db [D]); entries not wanted are None.  dw / db are fp32, or -- with
    out = (dw, db) contiguous bf16 tensors, e.g. views of a flat gradient buffer (None entries are allocated) -- written
    as bf16 in place."""
    _need(du, _BF16, "dwconv1d du", 3)
    _need(x, _BF16, "dwconv1d x", 3)
    B, N, D = x.shape
    k = _dw_weight(w, D)
    if tuple(du.shape) != (B, dwconv1d_out_len(N, k, stride), D):
        raise ValueError(f"dwconv1d du: shape {tuple(du.shape)} does not belong to x {tuple(x.shape)}, k={k}, stride={stride}")
    (dw, db), grad_bf16 = _grad_outs("dwconv1d_bwd", out, (w.shape, (D,)), (want_dw, want_db), x.device,
                                     "contiguous bf16 tensors of the weight's / bias's size")
    dx = torch.empty_like(x) if want_dx else None
    nbytes = lib.sfcvit_dwconv1d_bwd_workspace(B, N, D, k, stride) if (want_dw or want_db) else 0
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8) if nbytes else None
    with _Deferring([t for t in (dw, db) if t is not None], [ws]):
        _launch("dwconv1d_bwd", 4.0 * x.numel() + 4.0 * du.numel() + 2.0 * nbytes,
                lambda: check(lib.sfcvit_dwconv1d_bwd(_p(du), _p(x), _p(w), _p(dx), _p(dw), _p(db), int(grad_bf16), B, N, D, k, stride,
                                                      _p(ws), nbytes, _stream()), "sfcvit_dwconv1d_bwd"))
    return dx, dw, db


# ----------------------------------------------------------------------------
# positional embedding: one table row per token index, added to every image (vit.py:360-361, :382)
# ----------------------------------------------------------------------------
def last_pos_embed_kernel():
    return _last_kernel(lib.sfcvit_last_pos_embed_kernel)


def _pos_table(pos, N, D, name):
    """[N, D] or [1, N, D], contiguous bf16."""
    _need(pos, _BF16, name)
    if tuple(pos.shape) not in ((N, D), (1, N, D)):
        raise ValueError(f"{name}: a table of {N} tokens x {D} channels expected ([{N}, {D}] or [1, {N}, {D}]), got {tuple(pos.shape)}")


def pos_embed_fwd(x, pos):
    """y[b, n, :] = x[b, n, :] + pos[n, :] on x [B, N, D] bf16, pos [N, D] or [1, N, D] bf16 -> [B, N, D] bf16 (one rounding)."""
    _need(x, _BF16, "pos_embed x", 3)
    B, N, D = x.shape
    _pos_table(pos, N, D, "pos_embed pos")
    y = torch.empty_like(x)
    _launch("pos_embed_fwd", 4.0 * x.numel() + 2.0 * pos.numel(),
            lambda: check(lib.sfcvit_pos_embed_fwd(_p(x), _p(pos), _p(y), B, N, D, _stream()), "sfcvit_pos_embed_fwd"))
    return y


def pos_embed_bwd(dy, out=None):
    """-> dpos [N, D] = sum_b dy[b] for dy [B, N, D] bf16: fp32, or -- with out = a contiguous bf16 tensor of N * D elements,
    e.g. a view of a flat gradient buffer -- written as bf16 in place and returned."""
    _need(dy, _BF16, "pos_embed dy", 3)
    B, N, D = dy.shape
    (dpos,), grad_bf16 = _grad_outs("pos_embed_bwd", out, ((N, D),), (True,), dy.device, "a contiguous bf16 tensor of the table's size")
    nbytes = lib.sfcvit_pos_embed_bwd_workspace(B, N, D)
    ws = torch.empty(nbytes, device=dy.device, dtype=torch.uint8) if nbytes else None
    with _Deferring([dpos], [ws]):
        _launch("pos_embed_bwd", 2.0 * dy.numel() + float(dpos.numel() * dpos.element_size()) + 2.0 * nbytes,
                lambda: check(lib.sfcvit_pos_embed_bwd(_p(dy), _p(dpos), int(grad_bf16), B, N, D, _p(ws), nbytes, _stream()),
                              "sfcvit_pos_embed_bwd"))
    return dpos


# ----------------------------------------------------------------------------
# CLS token and token pooling (vit.py:209-210, :237-238, commented out there; altvit's x.mean(dim=1))
# ----------------------------------------------------------------------------
def last_token_pool_kernel():
    return _last_kernel(lib.sfcvit_last_token_pool_kernel)


def cls_prepend_fwd(x, cls):
    """y [B, N + 1, D] = cat([cls, x], dim=1) for x [B, N, D] bf16 and a contiguous bf16 cls of D elements: the bits move."""
    _need(x, _BF16, "cls_prepend x", 3)
    _need(cls, _BF16, "cls_prepend cls")
    B, N, D = x.shape
    if cls.numel() != D:
        raise ValueError(f"cls_prepend cls: {D} channels expected ([{D}] or [1, 1, {D}]), got {tuple(cls.shape)}")
    y = torch.empty((B, N + 1, D), device=x.device, dtype=_BF16)
    _launch("cls_prepend_fwd", 2.0 * x.numel() + 2.0 * y.numel(),
            lambda: check(lib.sfcvit_cls_prepend_fwd(_p(x), _p(cls), _p(y), B, N, D, _stream()), "sfcvit_cls_prepend_fwd"))
    return y


def cls_prepend_bwd(dy, want_dx=True, out=None):
    """dy [B, N + 1, D] bf16 -> (dx [B, N, D] = dy[:, 1:] or None, dcls [D] = sum_b dy[b, 0]): dcls is fp32, or -- with out = a
    contiguous bf16 tensor of D elements, e.g. a view of a flat gradient buffer -- written as bf16 in place and returned."""
    _need(dy, _BF16, "cls_prepend dy", 3)
    B, N1, D = dy.shape
    if N1 < 2:
        raise ValueError("cls_prepend_bwd: dy must hold the CLS row and at least one token")
    (dcls,), grad_bf16 = _grad_outs("cls_prepend_bwd", out, ((D,),), (True,), dy.device, "a contiguous bf16 tensor of D elements")
    dx = torch.empty((B, N1 - 1, D), device=dy.device, dtype=_BF16) if want_dx else None
    nbytes = lib.sfcvit_cls_prepend_bwd_workspace(B, N1 - 1, D)
    ws = torch.empty(nbytes, device=dy.device, dtype=torch.uint8) if nbytes else None
    with _Deferring([dcls], [ws]):
        _launch("cls_prepend_bwd", (4.0 if want_dx else 0.0) * B * (N1 - 1) * D + 2.0 * B * D,
                lambda: check(lib.sfcvit_cls_prepend_bwd(_p(dy), _p(dx), _p(dcls), int(grad_bf16), B, N1 - 1, D, _p(ws), nbytes,
                                                         _stream()), "sfcvit_cls_prepend_bwd"))
    return dx, dcls


def _pool_range(T, first, count):
    first = int(first)
    count = T - first if count is None else int(count)
    if first < 0 or count < 1 or first + count > T:
        raise ValueError(f"token_pool: tokens [{first}, {first} + {count}) are not a non-empty range of the {T} tokens")
    return first, count


def token_pool_fwd(x, first=0, count=None):
    """y [B, D] = mean over tokens [first, first + count) of x [B, T, D] bf16 (fp32 sum, one division, one rounding); count = 1
    copies the row's bits; count = None: to the last token."""
    _need(x, _BF16, "token_pool x", 3)
    B, T, D = x.shape
    first, count = _pool_range(T, first, count)
    y = torch.empty((B, D), device=x.device, dtype=_BF16)
    _launch("token_pool_fwd", 2.0 * B * count * D + 2.0 * B * D,
            lambda: check(lib.sfcvit_token_pool_fwd(_p(x), _p(y), B, T, D, first, count, _stream()), "sfcvit_token_pool_fwd"))
    return y


def token_pool_bwd(dy, T, first=0, count=None):
    """dx [B, T, D] = dy [B, D] / count on tokens [first, first + count), +0 elsewhere: every element written."""
    _need(dy, _BF16, "token_pool dy", 2)
    B, D = dy.shape
    first, count = _pool_range(int(T), first, count)
    dx = torch.empty((B, int(T), D), device=dy.device, dtype=_BF16)
    _launch("token_pool_bwd", 2.0 * dx.numel() + 2.0 * B * D,
            lambda: check(lib.sfcvit_token_pool_bwd(_p(dy), _p(dx), B, int(T), D, first, count, _stream()), "sfcvit_token_pool_bwd"))
    return dx


# ----------------------------------------------------------------------------
# token mixing: GEMMs along the token axis of [B, N, D] (MixerBlock.token_mix)
# ----------------------------------------------------------------------------
def last_tokmix_kernel():
    return _last_kernel(lib.sfcvit_last_tokmix_kernel)


def tokmix_left(w, x, *, transposed=False, bias=None, act=ACT_NONE, residual=None, aux_in=None, want_aux=False, out=None):
    """C_b = epi(op(W) X_b) for every image b: x [B, K, D] bf16 -> [B, M, D] bf16 with w [M, K] (or [K, M] with
    transposed=True) shared across the batch.  Epilogue (sfcvit_tokmix_left): + bias[m] (a row bias), pre-activation
    kept (want_aux), erf-GELU (act), + residual, * gelu'(aux_in).  Returns C, or (C, pre-activation) with want_aux."""
    _need(x, _BF16, "tokmix_left x", 3)
    _need(w, _BF16, "tokmix_left w", 2)
    B, K, D = x.shape
    M, Kw = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
    if Kw != K:
        raise ValueError(f"tokmix_left: contraction mismatch: w {tuple(w.shape)} (transposed={transposed}) against x {tuple(x.shape)}")
    if bias is not None and _need(bias, _BF16, "tokmix_left bias", 1).numel() != M:
        raise ValueError(f"tokmix_left bias: [{M}] expected")
    for t, name in ((residual, "residual"), (aux_in, "aux_in"), (out, "out")):
        if t is not None and tuple(_need(t, _BF16, f"tokmix_left {name}", 3).shape) != (B, M, D):
            raise ValueError(f"tokmix_left {name}: shape {(B, M, D)} expected, got {tuple(t.shape)}")
    c = out if out is not None else torch.empty((B, M, D), device=x.device, dtype=_BF16)
    aux = torch.empty((B, M, D), device=x.device, dtype=_BF16) if want_aux else None
    args = _lib.TokmixArgs()
    args.w, args.x, args.c = w.data_ptr(), x.data_ptr(), c.data_ptr()
    args.bias = bias.data_ptr() if bias is not None else None
    args.residual = residual.data_ptr() if residual is not None else None
    args.aux_in = aux_in.data_ptr() if aux_in is not None else None
    args.aux_out = aux.data_ptr() if aux is not None else None
    args.B, args.M, args.K, args.D = B, M, K, D
    args.w_transposed, args.act = int(transposed), act
    _launch("tokmix_left", 2.0 * B * M * K * D,
            lambda: check(lib.sfcvit_tokmix_left(ctypes.byref(args), _stream()), "sfcvit_tokmix_left"))
    return (c, aux) if want_aux else c


def tokmix_wgrad(g, x, want_dw=True, want_db=True, out=None):
    """-> (dW [M, K] = sum_b G_b X_b^T, db [M] = sum_{b, d} G_b[m, d]) for g [B, M, D], x [B, K, D] bf16; entries not
    wanted are None.  fp32, or -- with out = (dw, db) contiguous bf16 tensors, e.g. views of a flat gradient buffer (None
    entries are allocated) -- written as bf16 in place."""
    _need(g, _BF16, "tokmix_wgrad g", 3)
    _need(x, _BF16, "tokmix_wgrad x", 3)
    B, M, D = g.shape
    K = x.shape[1]
    if x.shape[0] != B or x.shape[2] != D:
        raise ValueError(f"tokmix_wgrad: g {tuple(g.shape)} and x {tuple(x.shape)} must share B and D")
    (dw, db), grad_bf16 = _grad_outs("tokmix_wgrad", out, ((M, K), (M,)), (want_dw, want_db), g.device,
                                     "contiguous bf16 tensors of the weight's / bias's size")
    nbytes = lib.sfcvit_tokmix_wgrad_workspace(B, M, K, D)
    ws = torch.empty(max(nbytes, 16), device=g.device, dtype=torch.uint8)
    with _Deferring([t for t in (dw, db) if t is not None], [ws]):
        _launch("tokmix_wgrad", 2.0 * B * M * K * D,
                lambda: check(lib.sfcvit_tokmix_wgrad(_p(g), _p(x), _p(dw), _p(db), int(grad_bf16), B, M, K, D, _p(ws), nbytes,
                                                      _stream()), "sfcvit_tokmix_wgrad"))
    return dw, db


# ----------------------------------------------------------------------------
# elementwise / loss / optimizer
# ----------------------------------------------------------------------------
def gelu_fwd(x):
    _need(x, _BF16, "gelu x")
    y = torch.empty_like(x)
    check(lib.sfcvit_gelu_fwd(_p(x), _p(y), x.numel(), _stream()), "sfcvit_gelu_fwd")
    return y


def gelu_bwd(dy, x):
    _need(x, _BF16, "gelu x")
    _need(dy, _BF16, "gelu dy")
    dx = torch.empty_like(x)
    check(lib.sfcvit_gelu_bwd(_p(dy), _p(x), _p(dx), x.numel(), _stream()), "sfcvit_gelu_bwd")
    return dx


def gelu_drop_fwd(x, p, seed):
    _need(x, _BF16, "gelu_drop x", 2)
    y = torch.empty_like(x)
    check(lib.sfcvit_gelu_drop_fwd(_p(x), _p(y), x.shape[0], x.shape[1], p, seed, _seed_off(), _stream()), "sfcvit_gelu_drop_fwd")
    return y


def gelu_drop_bwd(dy, x, p, seed):
    _need(x, _BF16, "gelu_drop x", 2)
    _need(dy, _BF16, "gelu_drop dy", 2)
    dx = torch.empty_like(x)
    check(lib.sfcvit_gelu_drop_bwd(_p(dy), _p(x), _p(dx), x.shape[0], x.shape[1], p, seed, _seed_off(), _stream()),
          "sfcvit_gelu_drop_bwd")
    return dx


def dropout_mask(rows, cols, p, seed, device="cuda"):
    """The keep mask as bf16 {0, 1/(1-p)} [rows, cols] (tests / debugging)."""
    out = torch.empty((rows, cols), device=device, dtype=_BF16)
    check(lib.sfcvit_dropout_mask(_p(out), rows, cols, p, seed, _stream()), "sfcvit_dropout_mask")
    return out


def soft_ce(logits, targets, n_classes, gscale):
    """logits bf16 [B, ld] (first n_classes columns are classes), targets fp32 [B, C].
    -> loss_rows fp32 [B], dlogits bf16 [B, ld] (already multiplied by gscale)."""
    _need(logits, _BF16, "soft_ce logits", 2)
    _need(targets, torch.float32, "soft_ce targets", 2)
    B, ld = logits.shape
    loss_rows = torch.empty(B, device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits)
    check(lib.sfcvit_soft_ce(_p(logits), _p(targets), _p(loss_rows), _p(dlogits), B, n_classes, ld, gscale, _stream()),
          "sfcvit_soft_ce")
    return loss_rows, dlogits


def augment_draw(rec, H, W, cfg, seed, step, sample_base=0):
    """Fill rec (int32 [B, 16], HOST tensor, contiguous) with the transform records of samples sample_base .. + B - 1 of
    step `step` (sfcvit_augment_draw: plain host code, no GPU).  cfg: _lib.AugmentCfg."""
    if rec.is_cuda or rec.dtype != torch.int32 or rec.dim() != 2 or rec.size(1) != _lib.AUG_WORDS or not rec.is_contiguous():
        raise ValueError(f"augment_draw rec: expected a contiguous host int32 [B, {_lib.AUG_WORDS}] tensor, got "
                         f"{rec.dtype} {tuple(rec.shape)} on {rec.device}")
    check(lib.sfcvit_augment_draw(_p(rec), rec.size(0), int(H), int(W), ctypes.byref(cfg), int(seed) & (2 ** 64 - 1),
                                  int(step) & (2 ** 64 - 1), int(sample_base)), "sfcvit_augment_draw")
    return rec


def augment_apply(u8, rec, cfg, out=None):
    """u8 uint8 [B, C, H, W] + rec int32 [B, 16] (device copy of augment_draw's records) -> the transformed batch
    [B, C, S, S], fp32 or bf16 as cfg.out_is_bf16 says (sfcvit_augment_apply: one launch).  out: write there instead of
    allocating (a GraphedTrainStep's static image buffer, say)."""
    if not u8.is_cuda:
        raise _lib.SfcvitError(f"augment_apply: the HIP path needs a CUDA (ROCm) tensor, got device {u8.device}; there is no CPU fallback")
    if u8.dim() != 4:
        raise ValueError(f"augment_apply u8: expected [B,C,H,W], got shape {tuple(u8.shape)}")
    u8 = _need(u8 if u8.is_contiguous() else u8.contiguous(), torch.uint8, "augment_apply u8", 4)
    rec = _need(rec, torch.int32, "augment_apply rec", 2)
    B, C, H, W = u8.shape
    if tuple(rec.shape) != (B, _lib.AUG_WORDS):
        raise ValueError(f"augment_apply: rec is {tuple(rec.shape)} for a batch of {B} images (expected [{B}, {_lib.AUG_WORDS}])")
    dtype = _BF16 if cfg.out_is_bf16 else torch.float32
    S = int(cfg.S)
    if out is None:
        out = torch.empty((B, C, S, S), dtype=dtype, device=u8.device)
    else:
        _need(out, dtype, "augment_apply out", 4)
        if tuple(out.shape) != (B, C, S, S):
            raise ValueError(f"augment_apply out: expected {(B, C, S, S)}, got {tuple(out.shape)}")
    check(_launch("augment_apply", 0.0, lambda: lib.sfcvit_augment_apply(_p(u8), _p(rec), _p(out), B, C, H, W, ctypes.byref(cfg),
                                                                          _stream())), "sfcvit_augment_apply")
    return out


def soft_ce_pair(logits, y_a, y_b, mix, n_classes, gscale):
    """logits bf16 [B, ld] (first n_classes columns are classes), y_a / y_b int64 [B] (device), mix: the batch mix whose
    record holds lam -> loss_rows fp32 [B], dlogits bf16 [B, ld] (times gscale), hit_rows fp32 [B]
    (lam * (argmax == y_a) + (1 - lam) * (argmax == y_b)): sfcvit_soft_ce_pair."""
    _need(logits, _BF16, "soft_ce_pair logits", 2)
    _need(y_a, torch.int64, "soft_ce_pair y_a", 1)
    _need(y_b, torch.int64, "soft_ce_pair y_b", 1)
    rec = _need(mix.rec, torch.int32, "soft_ce_pair mix.rec", 1)
    B, ld = logits.shape
    if y_a.numel() != B or y_b.numel() != B or rec.numel() != 8:
        raise ValueError(f"soft_ce_pair: {B} rows of logits, {y_a.numel()} / {y_b.numel()} labels, rec of {rec.numel()} words")
    loss_rows = torch.empty(B, device=logits.device, dtype=torch.float32)
    hit_rows = torch.empty(B, device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits)
    check(lib.sfcvit_soft_ce_pair(_p(logits), _p(y_a), _p(y_b), _p(rec), _p(loss_rows), _p(dlogits), _p(hit_rows), B, n_classes, ld,
                                  gscale, _stream()), "sfcvit_soft_ce_pair")
    return loss_rows, dlogits, hit_rows


def sumsq_accum(g, out):
    is_f32 = g.dtype == torch.float32
    if not is_f32:
        _need(g, _BF16, "sumsq g")
    ws = torch.empty(4096, device=g.device, dtype=torch.uint8)           # SFCVIT_SUMSQ_WORKSPACE_BYTES
    check(lib.sfcvit_sumsq_accum(_p(g), g.numel(), int(is_f32), _p(out), _p(ws), _stream()), "sfcvit_sumsq_accum")


def _adamw_args(param, master, grad, m, v, sumsq, lr, beta1, beta2, eps, weight_decay, max_norm, step, grad_scale, dev_state):
    a = _lib.AdamWArgs()
    a.param, a.master, a.grad, a.m, a.v = (param.data_ptr(), master.data_ptr(), grad.data_ptr(),
                                           m.data_ptr(), v.data_ptr())
    a.sumsq = sumsq.data_ptr() if sumsq is not None else None
    a.n = param.numel()
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.max_norm, a.step = lr, beta1, beta2, eps, weight_decay, max_norm, step
    a.grad_scale = grad_scale
    if dev_state is not None:
        a.dev_state = dev_state.data_ptr()
    return a


def adamw_step(param, master, grad, m, v, sumsq, *, lr, beta1, beta2, eps, weight_decay, max_norm, step,
               grad_scale=1.0, dev_state=None):
    a = _adamw_args(param, master, grad, m, v, sumsq, lr, beta1, beta2, eps, weight_decay, max_norm, step, grad_scale, dev_state)
    check(lib.sfcvit_adamw_step(ctypes.byref(a), _stream()), "sfcvit_adamw_step")


def adamw_ema_step(param, master, grad, m, v, sumsq, ema, ema_decay, ema_warmup=False, *, lr, beta1, beta2, eps, weight_decay,
                   max_norm, step, grad_scale=1.0, dev_state=None):
    """adamw_step plus, in the same kernel, ema <- ema + (1 - d_t) * (master - ema) on the new fp32 master (ema fp32 [n]);
    d_t = ema_decay, or with ema_warmup min(ema_decay, (1 + t) / (10 + t)) with t = `step` (the device counter under
    dev_state): sfcvit_adamw_ema_step.  param, master, m and v get adamw_step's bits."""
    _need(ema, torch.float32, "adamw_ema_step ema", 1)
    if ema.numel() != param.numel():
        raise ValueError(f"adamw_ema_step: ema has {ema.numel()} elements, param {param.numel()}")
    a = _adamw_args(param, master, grad, m, v, sumsq, lr, beta1, beta2, eps, weight_decay, max_norm, step, grad_scale, dev_state)
    e = _lib.EmaArgs()
    e.ema, e.decay, e.warmup = ema.data_ptr(), ema_decay, int(bool(ema_warmup))
    check(lib.sfcvit_adamw_ema_step(ctypes.byref(a), ctypes.byref(e), _stream()), "sfcvit_adamw_ema_step")


def _accum_pair(what, grad, acc):
    _need(grad, _BF16, f"{what} grad", 1)
    _need(acc, torch.float32, f"{what} acc", 1)
    if acc.numel() != grad.numel():
        raise ValueError(f"{what}: acc has {acc.numel()} elements, grad {grad.numel()}")


def grad_accum(grad, acc, first):
    """acc = float(grad) (`first`: acc is not read) or acc + float(grad), one fp32 add per element: a micro-batch's bf16 flat
    gradient folded into the fp32 running sum (sfcvit_grad_accum)."""
    _accum_pair("grad_accum", grad, acc)
    check(lib.sfcvit_grad_accum(_p(grad), _p(acc), grad.numel(), int(bool(first)), _stream()), "sfcvit_grad_accum")


def grad_accum_finish(grad, acc, scale, sumsq=None):
    """grad = bf16((acc + float(grad)) * scale) in place: the last micro-batch joins the sum and the average is formed in one
    pass.  sumsq (fp32 [1], device): the sum of the squares of the stored values is ADDED to it in the same pass, in a fixed
    order (sfcvit_grad_accum_finish) -- what sumsq_accum(grad, sumsq) would give afterwards, without its read of grad."""
    _accum_pair("grad_accum_finish", grad, acc)
    ws = None
    if sumsq is not None:
        _need(sumsq, torch.float32, "grad_accum_finish sumsq")
        ws = torch.empty(4096, device=grad.device, dtype=torch.uint8)    # SFCVIT_SUMSQ_WORKSPACE_BYTES
    check(lib.sfcvit_grad_accum_finish(_p(grad), _p(acc), grad.numel(), float(scale), _p(sumsq), _p(ws), _stream()),
          "sfcvit_grad_accum_finish")
