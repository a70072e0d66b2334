#!/usr/bin/env python3
"""Micro-benchmark of the CLS-token and token-pooling kernels:  python tools/bench_token_pool.py B N D   (default 256 196 768).

With T = N + 1 (the sequence of a model with a CLS token), prints from one process the median over 5 interleaved rounds
(each: device events around 50 calls, after a warm-up round) of microseconds per call and the achieved rate on the
ALGORITHMIC bytes of
    cls_prepend_fwd             2 B N D read + 2 B T D written
    cls_prepend_bwd (bf16 dcls) 2 B T D read + 2 B N D written (+ D)
    cls_prepend_bwd, dcls alone 2 B D read: the launch a frozen tokenizer would pay
    token_pool_fwd mean         2 B N D read (tokens 1 .. N of T) + 2 B D written
    token_pool_fwd CLS          2 B D read + 2 B D written: the read-out of token 0
    token_pool_bwd mean / CLS   2 B D read + 2 B T D written
    layernorm_fwd, [B T, D]     2 * 2 B T D + 8 B T   -- the project's memory-bound yardstick on the same tensor
Bars (bytes moved relative to the yardstick's 4 B T D): prepend forward and backward <= 1.10 x its time, the mean forward
and the pool backward (half the bytes) <= 1.0 x.
Rounds are interleaved (every candidate once per round) so that clock and neighbour drift hits all of them alike; the
spread printed is (max - min) / median over the 5 rounds.  Every call goes straight to the C ABI on preallocated buffers:
no allocator and no Python wrapper in the timed loop.  The timings include launch overhead (what a training step pays);
kernel-only times come from `rocprofv3 --kernel-trace --stats -- python tools/bench_token_pool.py ...`."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
from sfcvit import ops  # noqa: E402
from sfcvit._lib import check, lib  # noqa: E402

args = [int(v) for v in sys.argv[1:]]
B, N, D = args[:3] if len(args) >= 3 else (256, 196, 768)
T = N + 1
if not torch.cuda.is_available():
    raise SystemExit("bench_token_pool: needs the GPU; nothing is measured without one")
ROUNDS, CALLS = 5, 50
g = torch.Generator(device="cuda").manual_seed(0)
rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g).bfloat16()      # noqa: E731
x, cls, dy, gamma, beta, dpooled = rnd(B, N, D), rnd(D), rnd(B, T, D), rnd(D), rnd(D), rnd(B, D)
y, dx, ln_y, pool_dx = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(dy), torch.empty_like(dy)
pooled = torch.empty(B, D, device="cuda", dtype=torch.bfloat16)
mean, rstd = (torch.empty(B * T, device="cuda", dtype=torch.float32) for _ in range(2))
dcls = torch.empty(D, device="cuda", dtype=torch.bfloat16)
ws_bytes = lib.sfcvit_cls_prepend_bwd_workspace(B, N, D)
ws = torch.empty(max(ws_bytes, 16), device="cuda", dtype=torch.uint8)
p = lambda t: ctypes.c_void_p(t.data_ptr())                    # noqa: E731
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def pre_fwd():
    check(lib.sfcvit_cls_prepend_fwd(p(x), p(cls), p(y), B, N, D, st), "cls_prepend_fwd")


def pre_bwd(with_dx):
    return lambda: check(lib.sfcvit_cls_prepend_bwd(p(dy), p(dx) if with_dx else None, p(dcls), 1, B, N, D, p(ws), ws_bytes, st), "cls_prepend_bwd")


def pool_fwd(first, count):
    return lambda: check(lib.sfcvit_token_pool_fwd(p(dy), p(pooled), B, T, D, first, count, st), "token_pool_fwd")


def pool_bwd(first, count):
    return lambda: check(lib.sfcvit_token_pool_bwd(p(dpooled), p(pool_dx), B, T, D, first, count, st), "token_pool_bwd")


def ln_fwd():
    check(lib.sfcvit_layernorm_fwd(p(dy), p(gamma), p(beta), p(ln_y), p(mean), p(rstd), B * T, D, 1e-5, st), "layernorm_fwd")


def timeit(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3


row, img = 2 * B * D, 2 * B * N * D
YARD = "layernorm_fwd (yardstick)"
rows = [("cls_prepend_fwd", pre_fwd, 2 * img + row, 1.10),
        (YARD, ln_fwd, 2 * (img + row) + 8 * B * T, None),
        ("cls_prepend_bwd", pre_bwd(True), 2 * img + row + 2 * D, 1.10),
        ("cls_prepend_bwd dcls alone", pre_bwd(False), row + 2 * D, None),
        ("token_pool_fwd mean", pool_fwd(1, N), img + row, 1.0),
        ("token_pool_fwd CLS", pool_fwd(0, 1), 2 * row, None),
        ("token_pool_bwd mean", pool_bwd(1, N), row + img + row, 1.0),
        ("token_pool_bwd CLS", pool_bwd(0, 1), row + img + row, 1.0)]
names = {}
for name, fn, _, _ in rows:                                    # warm-up round: code objects loaded, clocks up
    timeit(fn)
    names[name] = ops.last_token_pool_kernel()
times = {name: [] for name, _, _, _ in rows}
for _ in range(ROUNDS):
    for name, fn, _, _ in rows:
        times[name].append(timeit(fn))
torch.cuda.synchronize()

print(f"B={B} N={N} T={T} D={D}  workspace cls_prepend_bwd {ws_bytes} bytes  device {torch.cuda.get_device_name(0)}")
med = {name: statistics.median(times[name]) for name, _, _, _ in rows}
for name, _, nbytes, bar in rows:
    t = times[name]
    kernel = "" if name == YARD else f"  [{names[name]}]"
    print(f"{name:28s} {med[name]:9.1f} us  {nbytes / med[name] / 1e6:6.2f} TB/s  spread {(max(t) - min(t)) / med[name] * 100:5.1f} %  "
          f"rounds {' '.join(f'{v:.1f}' for v in t)}{kernel}")
for name, _, _, bar in rows:
    if bar is not None:
        print(f"{name + ' / layernorm_fwd':42s} {med[name] / med[YARD]:.3f}   (bar: <= {bar:.2f})")
