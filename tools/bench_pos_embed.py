#!/usr/bin/env python3
"""Micro-benchmark of the positional-embedding kernels:  python tools/bench_pos_embed.py B N D   (default 256 196 768).

Prints, from one process, the median over 5 interleaved rounds (each: device events around 50 calls, after a warm-up round)
of microseconds per call and the achieved rate on the ALGORITHMIC bytes of
    pos_embed_fwd               2 (2 B N D + N D)
    layernorm_fwd, [B N, D]     2 * 2 B N D + 8 B N   -- the project's memory-bound yardstick: the same activation bytes, more
                                                        arithmetic.  The forward must take at most 1.10 x its time.
    pos_embed_bwd (fp32, bf16)  2 B N D + the table's gradient (+ the partial rows, written and read once, where the plan splits)
    colsum on the [B, N D] view 2 B N D + an [row blocks, N D] fp32 partial written and read + the gradient: the existing path
                                the dedicated backward kernel has to beat by more than the run-to-run spread
Rounds are interleaved (every candidate once per round) so that clock and neighbour drift hits all of them alike; the
spread printed is (max - min) / median over the 5 rounds.  Every call goes straight to the C ABI on preallocated buffers:
no allocator and no Python wrapper in the timed loop.  The timings include launch overhead (what a training step pays);
kernel-only times come from `rocprofv3 --kernel-trace --stats -- python tools/bench_pos_embed.py ...`."""
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
if not torch.cuda.is_available():
    raise SystemExit("bench_pos_embed: needs the GPU; nothing is measured without one")
ROUNDS, CALLS = 5, 50
g = torch.Generator(device="cuda").manual_seed(0)
rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g).bfloat16()      # noqa: E731
x, pos, dy, gamma, beta = rnd(B, N, D), rnd(N, D), rnd(B, N, D), rnd(D), rnd(D)
y = torch.empty_like(x)
mean, rstd = (torch.empty(B * N, device="cuda", dtype=torch.float32) for _ in range(2))
g32, c32 = (torch.empty(N * D, device="cuda", dtype=torch.float32) for _ in range(2))
g16, c16 = (torch.empty(N * D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
ws_pe = lib.sfcvit_pos_embed_bwd_workspace(B, N, D)
ws_cs = lib.sfcvit_colsum_workspace(B, N * D)
ws = torch.empty(max(ws_pe, ws_cs, 16), device="cuda", dtype=torch.uint8)
p = lambda t: ctypes.c_void_p(t.data_ptr())                    # noqa: E731
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def pe_fwd():
    check(lib.sfcvit_pos_embed_fwd(p(x), p(pos), p(y), B, N, D, st), "pos_embed_fwd")


def ln_fwd():
    check(lib.sfcvit_layernorm_fwd(p(x), p(gamma), p(beta), p(y), p(mean), p(rstd), B * N, D, 1e-5, st), "layernorm_fwd")


def pe_bwd(out, bf16):
    return lambda: check(lib.sfcvit_pos_embed_bwd(p(dy), p(out), bf16, B, N, D, p(ws), ws_pe, st), "pos_embed_bwd")


def cs_bwd(out, bf16):
    return lambda: check(lib.sfcvit_colsum(p(dy), B, N * D, N * D, p(out), bf16, p(ws), ws_cs, st), "colsum")


def timeit(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3


act = 2 * B * N * D
rows = [("pos_embed_fwd", pe_fwd, 2 * act + 2 * N * D),
        ("layernorm_fwd (yardstick)", ln_fwd, 2 * act + 8 * B * N),
        ("pos_embed_bwd fp32", pe_bwd(g32, 0), act + 4 * N * D + 2 * ws_pe),
        ("colsum [B, N D] fp32", cs_bwd(c32, 0), act + 4 * N * D + 2 * ws_cs),
        ("pos_embed_bwd bf16", pe_bwd(g16, 1), act + 2 * N * D + 2 * ws_pe),
        ("colsum [B, N D] bf16", cs_bwd(c16, 1), act + 2 * N * D + 2 * ws_cs)]
pe_fwd()
k_fwd = ops.last_pos_embed_kernel()
pe_bwd(g16, 1)()
k_bwd = ops.last_pos_embed_kernel()
for _, fn, _ in rows:                                          # warm-up round: code objects loaded, clocks up
    timeit(fn)
times = {name: [] for name, _, _ in rows}
for _ in range(ROUNDS):
    for name, fn, _ in rows:
        times[name].append(timeit(fn))
torch.cuda.synchronize()
same = torch.equal(g32, c32) and torch.equal(g16, c16)         # (one row block, one range: both add images rl, rl + 8, ... per lane, then the 8 lanes in order)

print(f"B={B} N={N} D={D}  workspace pos_embed_bwd {ws_pe / 1e6:.2f} MB, colsum {ws_cs / 1e6:.2f} MB  kernels [{k_fwd}] [{k_bwd}]  "
      f"device {torch.cuda.get_device_name(0)}")
med = {}
for name, _, nbytes in rows:
    t = times[name]
    med[name] = statistics.median(t)
    print(f"{name:28s} {med[name]:9.1f} us  {nbytes / med[name] / 1e6:6.2f} TB/s  spread {(max(t) - min(t)) / med[name] * 100:5.1f} %  "
          f"rounds {' '.join(f'{v:.1f}' for v in t)}")
print(f"forward / layernorm_fwd                {med['pos_embed_fwd'] / med['layernorm_fwd (yardstick)']:.3f}   (bar: <= 1.10)")
for dt in ("fp32", "bf16"):
    print(f"backward {dt}: dedicated / colsum      {med['pos_embed_bwd ' + dt] / med['colsum [B, N D] ' + dt]:.3f}")
print(f"dedicated and colsum gradients bitwise equal: {same}")
