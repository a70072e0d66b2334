#!/usr/bin/env python3
"""Micro-benchmark of the row-wise kernels at the ViT-B step's shapes (M = 50176, D = 768; or `M D` on the command line):
LayerNorm fwd / bwd, the stochastic-depth forms of both (rate 0.1, images of M / B rows with B = 256, 64 or 1), the LayerScale
forms of both (the same with a per-channel scale; the backward reads the branch as a sixth stream), column sums.
The cases run in turn, ROUNDS times over (default 5, third argument); prints the median us per launch with the spread over the
rounds and the achieved HBM rate on the algorithmic bytes.
SFCVIT_LN_BLOCKS=<n> changes the LayerNorm-backward grid (one process per setting)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
from sfcvit import ops  # noqa: E402

M, D = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (50176, 768)      # ViT-L: 36864 1024
g = torch.Generator(device="cuda").manual_seed(0)
x = torch.randn(M, D, device="cuda", generator=g).bfloat16()
dy = torch.randn(M, D, device="cuda", generator=g).bfloat16()
w = torch.randn(D, device="cuda", generator=g).bfloat16()
b = torch.randn(D, device="cuda", generator=g).bfloat16()
lam = (0.1 * torch.randn(D, device="cuda", generator=g)).bfloat16()
big_d = torch.randn(M, D, device="cuda", generator=g).bfloat16()          # the branch a LayerScale backward reads
big = torch.randn(M, 3072, device="cuda", generator=g).bfloat16()
y, mean, rstd = ops.layernorm_fwd(x, w, b, 1e-5)
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
B = next(n for n in (256, 64, 1) if M % n == 0)


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


cases = [("ln_fwd", lambda: ops.layernorm_fwd(x, w, b, 1e-5), 2 * M * D * 2),
         ("ln_bwd", lambda: ops.layernorm_bwd(dy, x, mean, rstd, w), 3 * M * D * 2),
         ("ln_bwd + dropout out + colsum", lambda: ops.layernorm_bwd(dy, x, mean, rstd, w, drop_p=0.1, drop_seed=5, want_colsum=True), 4 * M * D * 2),
         # s = x + c[b] branch, LayerNorm(s): reads x and the branch, writes s and y
         ("add + ln_fwd, drop path 0.1", lambda: ops.add_layernorm_path_fwd(dy, x, w, b, B, 0.1, 1234, 1e-5), 4 * M * D * 2),
         ("ln_bwd path + dropout out + colsum", lambda: ops.layernorm_bwd_path(dy, x, mean, rstd, w, M // B, 0.1, 1234, drop_p=0.1, drop_seed=5,
                                                                              want_colsum=True), 4 * M * D * 2),
         # the LayerScale site: the same streams forward; backward reads the branch too (for dlam): 5 M D elements moved -> 6
         ("add + ln_fwd, layer scale, path 0.1", lambda: ops.add_layernorm_scale_fwd(dy, x, lam, w, b, B, 0.1, 1234, 1e-5), 4 * M * D * 2),
         ("add + ln_fwd, layer scale, no path", lambda: ops.add_layernorm_scale_fwd(dy, x, lam, w, b, B), 4 * M * D * 2),
         ("ln_bwd scale + dropout out + colsum", lambda: ops.layernorm_bwd_scale(dy, x, mean, rstd, w, big_d, lam, M // B, 0.1, 1234, drop_p=0.1,
                                                                               drop_seed=5, want_colsum=True), 5 * M * D * 2),
         ("colsum [M,768]", lambda: ops.colsum(x), M * D * 2),
         ("colsum [M,3072]", lambda: ops.colsum(big), M * 3072 * 2)]
print("SFCVIT_LN_BLOCKS =", os.environ.get("SFCVIT_LN_BLOCKS", "(default)"))
print(f"M = {M}, D = {D}, B = {B}; median of {ROUNDS} rounds of 20 launches [min .. max]")
times = {name: [] for name, _, _ in cases}
for _ in range(ROUNDS):
    for name, fn, _ in cases:
        times[name].append(timeit(fn))
for name, _, nbytes in cases:
    t = sorted(times[name])
    us = t[len(t) // 2]
    print(f"{name:36s} {us:8.1f} us [{t[0]:7.1f} .. {t[-1]:7.1f}]  {nbytes / us / 1e6:6.2f} TB/s")
ops.layernorm_bwd_scale(dy, x, mean, rstd, w, big_d, lam, M // B, 0.1, 1234)
print("ln_bwd scale kernel:", ops.last_rowwise_kernel())
ops.layernorm_bwd(dy, x, mean, rstd, w)
print("ln_bwd kernel:", ops.last_rowwise_kernel(), " SFCVIT_LN_COLS =", os.environ.get("SFCVIT_LN_COLS", "(default)"))
