#!/usr/bin/env python3
"""Attention-probe kernels alone (csrc/attention_probe.hip) next to the attention forward on the same box and shape:
the statistics kernel does the forward's q k^T work without P V; the map kernels are bound by their stores.
Interleaved rounds in ONE process, median of 5 (default ViT-B/16 @ 224: B 256, N 196, H 12, hd 64).
    python tools/bench_attention_probe.py [B N H [hd]]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
from sfcvit import ops  # noqa: E402

args = [int(a) for a in sys.argv[1:]]
B, N, H = args[:3] if len(args) >= 3 else (256, 196, 12)
hd = args[3] if len(args) >= 4 else 64
g = torch.Generator(device="cuda").manual_seed(0)
qkv = torch.randn(B, N, 3 * H * hd, device="cuda", generator=g).bfloat16()
out, lse = ops.attention_fwd(qkv, H, any_length=True)
w = int((N - 1) ** 0.5) + 1
i = torch.arange(N, device="cuda")
pos = torch.stack(((i // w) * 16 + 7.5, (i % w) * 16 + 7.5), dim=1).float().contiguous()
stats_out = {k: torch.empty(B, H, N, device="cuda") for k in ops.ATTENTION_STATS}
maps = {("fp32", False): torch.empty(B, H, N, N, device="cuda"),
        ("bf16", False): torch.empty(B, H, N, N, device="cuda", dtype=torch.bfloat16),
        ("fp32", True): torch.empty(B, N, N, device="cuda"),
        ("bf16", True): torch.empty(B, N, N, device="cuda", dtype=torch.bfloat16)}


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


cases = {"attention fwd (q k^T, softmax, P V), p = 0": (lambda: ops.attention_fwd(qkv, H, any_length=True), 4.0, 0),
         "stats: distance + sequence distance + entropy + mass": (lambda: ops.attention_stats(qkv, lse, H, pos=pos, out=stats_out), 2.0, 0)}
for (name, mean), t in maps.items():
    cases[f"map {name}{', mean over heads' if mean else ' per head'}"] = (
        lambda t=t, mean=mean: ops.attention_probs(qkv, lse, H, head_mean=mean, dtype=t.dtype, out=t), 2.0, t.numel() * t.element_size())
rows = {k: [] for k in cases}
for rnd in range(5):
    for k, (fn, _, _) in cases.items():
        rows[k].append(timeit(fn))
print(f"B={B} N={N} H={H} hd={hd}")
for k, v in rows.items():
    v = sorted(v)
    med = v[len(v) // 2]
    fl, stored = cases[k][1] * B * H * N * N * hd, cases[k][2]
    tail = f"   stores {stored / 1e6:8.1f} MB at {stored / med / 1e3:7.1f} GB/s" if stored else ""
    print(f"{k:56s} median {med:8.1f} us  min {v[0]:8.1f}   {fl / med / 1e6:7.1f} TFLOP/s{tail}")
