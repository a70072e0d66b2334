#!/usr/bin/env python3
"""Micro-benchmark of the RoPE kernels:  python tools/bench_rope.py B N H [hd]   (default 256 196 12 64).

Prints, from one process, microseconds per call (device events around 50 calls after 5 warm-up calls) and the achieved rate on
the ALGORITHMIC bytes of
    rope_fwd                    M * 2 Da bf16 read, M * 2 Da bf16 written (q | k in place)                   = 8 M Da bytes
    rope_bwd, no sums           the same, one launch                                                         = 8 M Da bytes
    rope_bwd + second stage     the same (+ the partial-sum workspace, written once and read once by the second stage)
    layernorm_fwd [2 M, Da]     read + write                                                                 = 8 M Da bytes
    layernorm_bwd [4 M / 3, Da] dy + x read, dx written                                                      = 8 M Da bytes
    qk_norm_fwd / qk_norm_bwd   at the same shape (12 M Da bytes each), with their own yardsticks [3 M, Da] / [2 M, Da]
M = B * N, Da = H * kernel head dim.  The LayerNorm lines are the project's memory-bound yardstick on a tensor of the same byte
volume, run first and again last; the figure of merit of a kernel is its rate as a fraction of its yardstick's, and the QK-norm
lines give that fraction for the sibling kernels in the same run.  The table (N * hd * 4 bytes) is not counted: it stays in L2.
The timings include launch overhead (what a training step pays); kernel-only times come from
`rocprofv3 --kernel-trace --stats -- python tools/bench_rope.py ...` by the names printed in the last column."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
from sfcvit import ops, rope  # noqa: E402

args = [int(v) for v in sys.argv[1:]]
B, N, H = args[:3] if len(args) >= 3 else (256, 196, 12)
hd = args[3] if len(args) > 3 else 64
hp = ops.padded_head_dim(hd)
if not torch.cuda.is_available():
    raise SystemExit("bench_rope: needs the GPU; nothing is measured without one")
g = torch.Generator(device="cuda").manual_seed(0)
rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g).bfloat16()      # noqa: E731
M, Da = B * N, H * hp
qkv, dqkv = rnd(M, 3 * Da), rnd(M, 3 * Da)
table = ops.RopeTable(rope.curve_table(N, hd))
ops.rope_fwd(qkv, table, H)
k_fwd = ops.last_rowwise_kernel()
slot, vs = torch.empty(3 * Da, device="cuda", dtype=torch.bfloat16), torch.zeros(Da, device="cuda")
ops.rope_bwd(dqkv, table, H, colsum=slot, vsum=vs)
k_bwd = ops.last_rowwise_kernel()
P = torch.stack([1 + 0.1 * rnd(hd).float(), 0.1 * rnd(hd).float(), 1 + 0.1 * rnd(hd).float(), 0.1 * rnd(hd).float()]).bfloat16()
qkv_n, dqkv_n = rnd(M, 3 * Da), rnd(M, 3 * Da)
raw = ops.qk_norm_fwd(qkv_n, P, H, hd)
dP = torch.empty(4, hd, device="cuda", dtype=torch.bfloat16)
Mb = (4 * M + 2) // 3
x3, x2, xb = rnd(3 * M, Da), rnd(2 * M, Da), rnd(Mb, Da)
dy2, dyb = rnd(2 * M, Da), rnd(Mb, Da)
ln_w, ln_b = rnd(Da), rnd(Da)
_, mean2, rstd2 = ops.layernorm_fwd(x2, ln_w, ln_b)
_, meanb, rstdb = ops.layernorm_fwd(xb, ln_w, ln_b)


def timeit(fn, n=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


nb8, nb12 = 8 * M * Da, 12 * M * Da
ws = ops.lib.sfcvit_rope_bwd_ws(B, N, H, hp)
ws_qk = ops.lib.sfcvit_qk_norm_bwd_ws(M, H, hp)
print(f"B={B} N={N} H={H} hd={hd} (kernel head dim {hp})  M={M} Da={Da}  {nb8 / 1e6:.1f} MB per RoPE call  workspace {ws / 1e6:.2f} MB  "
      f"plan {ops.rope_plan(B, N, H, hp)}  device {torch.cuda.get_device_name(0)}")
# (the kernels run in place: on their own output from the second call on, which moves the same bytes)
ln_f8 = ("layernorm_fwd [2M, Da] (yardstick)", lambda: ops.layernorm_fwd(x2, ln_w, ln_b), nb8, "ln_fwd", "f8")
ln_b8 = ("layernorm_bwd [4M/3, Da] (yardstick)", lambda: ops.layernorm_bwd(dyb, xb, meanb, rstdb, ln_w), 6 * Mb * Da, "ln_bwd", "b8")
ln_f12 = ("layernorm_fwd [3M, Da] (yardstick)", lambda: ops.layernorm_fwd(x3, ln_w, ln_b), nb12, "ln_fwd", "f12")
ln_b12 = ("layernorm_bwd [2M, Da] (yardstick)", lambda: ops.layernorm_bwd(dy2, x2, mean2, rstd2, ln_w), nb12, "ln_bwd", "b12")
rows = [ln_f8, ln_b8, ln_f12, ln_b12,
        ("rope_fwd", lambda: ops.rope_fwd(qkv, table, H), nb8, k_fwd, "f8"),
        ("rope_bwd, no sums", lambda: ops.rope_bwd(dqkv, table, H), nb8, k_bwd, "b8"),
        ("rope_bwd + second stage", lambda: ops.rope_bwd(dqkv, table, H, colsum=slot, vsum=vs), nb8 + 2 * ws, k_bwd + " + rope_bwd_reduce", "b8"),
        ("qk_norm_fwd", lambda: ops.qk_norm_fwd(qkv_n, P, H, hd), nb12, f"qk_norm_fwd_kernel<{hp}>", "f12"),
        ("qk_norm_bwd + second stage", lambda: ops.qk_norm_bwd(dqkv_n, raw, P, H, hd, colsum=slot, grad_out=dP, vsum=vs), nb12 + 2 * ws_qk,
         f"qk_norm_bwd_kernel<{hp}> + qk_norm_bwd_reduce", "b12"),
        ln_f8, ln_b8, ln_f12, ln_b12]
yard = {}
for name, fn, nb, kern, kind in rows:
    us = timeit(fn)
    rate = nb / us / 1e6
    yard.setdefault(kind, rate)
    print(f"{name:38s} {us:9.1f} us  {rate:6.2f} TB/s  {rate / yard[kind]:5.2f} x yardstick   [{kern}]")
