#!/usr/bin/env python3
"""Relative-position-bias attention kernels (csrc/attention_bias.hip) next to the masked kernels (csrc/attention_masked.hip)
on the same device, in one process, on the same q, k, v: forward and backward of
    the masked kernels with an all-zero mask          | the bias kernels over the all-visible curve index (T = 2 N - 1),
    the masked kernels with curve_window(N, W)        | the bias kernels over curve_offsets(N, window=W)  (same visited blocks).
The bias backward is timed twice, with the table gradient and with a frozen table (dK / dV + dQ only); the table-gradient
part is the difference of the two medians.  Random inputs, table 0.5 * randn; HIP events, 20 launches per timing after
warm-up, interleaved rounds, median and min of 5.  Head dim 64.
    python tools/bench_attention_bias.py B N H [W ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
from sfcvit import masks, ops, relpos  # noqa: E402
from sfcvit._lib import lib  # noqa: E402

args = [int(a) for a in sys.argv[1:]]
if len(args) < 3:
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


cases = {}            # label -> (blocks, {column: fn})
for w in [None] + windows:
    hm = ops.AttentionMask(torch.zeros(N, N) if w is None else masks.curve_window(N, w))
    m, bm = hm.on("cuda")
    o, l = ops.attention_masked_fwd(qkv, H, m, bm)
    label = "masked, all-zero mask" if w is None else f"masked, curve_window({N}, {w})"
    cases[label] = (f"{hm.visited_blocks}/{hm.total_blocks}",
                    {"fwd": lambda m=m, bm=bm: ops.attention_masked_fwd(qkv, H, m, bm),
                     "bwd": lambda m=m, bm=bm, o=o, l=l: ops.attention_masked_bwd(qkv, o, l, dout, H, m, bm)})
    hb = ops.AttentionBiasIndex(*relpos.curve_offsets(N, w))
    hb.on("cuda")
    table = 0.5 * torch.randn(H, hb.n_buckets, device="cuda", generator=g)
    o, l = ops.attention_bias_fwd(qkv, H, table, hb)
    label = f"bias, curve_offsets({N})" if w is None else f"bias, curve_offsets({N}, {w})"
    ws = lib.sfcvit_attention_bias_workspace(B, N, H, hb.visited_blocks)
    cases[label] = (f"{hb.visited_blocks}/{hb.total_blocks}",
                    {"fwd": lambda t=table, hb=hb: ops.attention_bias_fwd(qkv, H, t, hb),
                     "bwd": lambda t=table, hb=hb, o=o, l=l: ops.attention_bias_bwd(qkv, o, l, dout, H, t, hb, table_grad=False),
                     "bwd+table": lambda t=table, hb=hb, o=o, l=l: ops.attention_bias_bwd(qkv, o, l, dout, H, t, hb)},
                    f"T={hb.n_buckets}, table-gradient workspace {ws / 2 ** 20:.1f} MiB")
rows = {k: {c: [] for c in v[1]} for k, v in cases.items()}
for rnd in range(5):
    for k, v in cases.items():
        for c, fn in v[1].items():
            rows[k][c].append(timeit(fn))
print(f"B={B} N={N} H={H} hd={hd}  device: {torch.cuda.get_device_name()}")
print(f"{'case':34s} {'blocks':>7s} {'fwd med':>8s} {'min':>7s} {'dKdV+dQ med':>12s} {'min':>7s} {'with table med':>15s} {'min':>7s} {'table part':>11s}  (us)")
med = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
for k, r in rows.items():
    line = f"{k:34s} {cases[k][0]:>7s} {med(r['fwd']):8.1f} {min(r['fwd']):7.1f} {med(r['bwd']):12.1f} {min(r['bwd']):7.1f}"
    if "bwd+table" in r:
        line += f" {med(r['bwd+table']):15.1f} {min(r['bwd+table']):7.1f} {med(r['bwd+table']) - med(r['bwd']):11.1f}   {cases[k][2]}"
    print(line)
