#!/usr/bin/env python3
"""Masked attention kernels (csrc/attention_masked.hip) next to the production unmasked kernels on the same device, in
one process: forward and backward of
    the production kernel the library picks for the shape (no mask),
    the masked kernels with an all-zero mask (every block visited, no mask read),
    the masked kernels with curve_window(N, W) (only the band's blocks visited),
with the visited-block ratio.  Random q, k, v; HIP events, 20 launches per timing after warm-up, interleaved rounds, median
and min of 5.  Head dim 64.
    python tools/bench_attention_masked.py B N H W [W ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
from sfcvit import masks, ops  # noqa: E402

args = [int(a) for a in sys.argv[1:]]
if len(args) < 4:
    raise SystemExit(__doc__)
B, N, H = args[:3]
windows = args[3:]
hd = 64
g = torch.Generator(device="cuda").manual_seed(0)
qkv = torch.randn(B, N, 3 * H * hd, device="cuda", generator=g).bfloat16()
dout = torch.randn(B, N, H * hd, device="cuda", generator=g).bfloat16()


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


cases = {}
out_u, lse_u = ops.attention_fwd(qkv, H, any_length=True)
name_f = ops.last_attn_kernel()
ops.attention_bwd(qkv, out_u, lse_u, dout, H, any_length=True)
name_b = ops.last_attn_kernel()
cases["unmasked"] = (lambda: ops.attention_fwd(qkv, H, any_length=True),
                     lambda: ops.attention_bwd(qkv, out_u, lse_u, dout, H, any_length=True), "1/1", f"{name_f} | {name_b}")
holders = [("masked, all-zero mask", ops.AttentionMask(torch.zeros(N, N)))]
holders += [(f"masked, curve_window({N}, {w})", ops.AttentionMask(masks.curve_window(N, w))) for w in windows]
for label, hm in holders:
    m, bm = hm.on("cuda")
    o, l = ops.attention_masked_fwd(qkv, H, m, bm)
    cases[label] = (lambda m=m, bm=bm: ops.attention_masked_fwd(qkv, H, m, bm),
                    lambda m=m, bm=bm, o=o, l=l: ops.attention_masked_bwd(qkv, o, l, dout, H, m, bm),
                    f"{hm.visited_blocks}/{hm.total_blocks}", "attn_masked_fwd_kernel | attn_masked_bwd_{kv,q}_kernel")
rows = {k: ([], []) for k in cases}
for rnd in range(5):
    for k, (fwd, bwd, _, _) in cases.items():
        rows[k][0].append(timeit(fwd))
        rows[k][1].append(timeit(bwd))
print(f"B={B} N={N} H={H} hd={hd}  device: {torch.cuda.get_device_name()}")
print(f"{'case':34s} {'blocks':>9s} {'fwd median':>11s} {'fwd min':>9s} {'bwd median':>11s} {'bwd min':>9s}  (us)  kernels")
for k, (f, b) in rows.items():
    f, b = sorted(f), sorted(b)
    print(f"{k:34s} {cases[k][2]:>9s} {f[len(f) // 2]:11.1f} {f[0]:9.1f} {b[len(b) // 2]:11.1f} {b[0]:9.1f}        {cases[k][3]}")
