#!/usr/bin/env python3
"""The fused clip + AdamW kernel alone (28 B of state per parameter: fp32 master / m / v read and written, bf16 gradient
read, bf16 parameter written) at ViT-B (86.6 M) and ViT-L (304 M) sizes; optional A/B against another build of the
library (SFCVIT_LIB).    python tools/bench_adamw.py [--ema] [n_params ...]

--ema: the same loop over ops.adamw_ema_step (the weight average updated in the same kernel: one more fp32 stream in and
out, 36 B per parameter), the plain step next to it in the same process, and what the fusion replaces: a separate
`ema.lerp_(master, 1 - d)` pass over the flat buffers (12 B per parameter)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
from sfcvit import ops  # noqa: E402

argv = sys.argv[1:]
with_ema = "--ema" in argv
sizes = [int(a) for a in argv if a != "--ema"] or [86_567_656, 304_330_000]


def timed(fn):
    """Median over 5 windows of 10 calls, in microseconds per call (device events)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 10 * 1e3)
    return sorted(ts)[len(ts) // 2]


for n in sizes:
    n = n // 8 * 8
    master = torch.randn(n, device="cuda")
    param = master.bfloat16()
    grad = (torch.randn(n, device="cuda") * 1e-2).bfloat16()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    sumsq = torch.ones(1, device="cuda")
    hyper = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-5, max_norm=1.0)

    def step(i=[0]):
        i[0] += 1
        ops.adamw_step(param, master, grad, m, v, sumsq, step=i[0], **hyper)

    if not with_ema:
        med = timed(step)
        print(f"n = {n / 1e6:7.1f} M   {med:8.1f} us   {28.0 * n / med / 1e6:6.2f} TB/s of 28 B/param")
        continue
    ema = master.clone()

    def ema_step(i=[0]):
        i[0] += 1
        ops.adamw_ema_step(param, master, grad, m, v, sumsq, ema, 0.9999, True, step=i[0], **hyper)

    def lerp():
        ema.lerp_(master, 1.0 - 0.9999)

    # plain, fused, plain, fused: the two alternate in one process, the medians of each pair are averaged
    plain, fused = [], []
    for _ in range(2):
        plain.append(timed(step))
        fused.append(timed(ema_step))
    t_plain, t_ema, t_lerp = sum(plain) / 2, sum(fused) / 2, timed(lerp)
    print(f"n = {n / 1e6:7.1f} M   ema {t_ema:8.1f} us   {36.0 * n / t_ema / 1e6:6.2f} TB/s of 36 B/param   plain {t_plain:8.1f} us   "
          f"{28.0 * n / t_plain / 1e6:6.2f} TB/s of 28 B/param   ratio {t_ema / t_plain:5.3f}   fused adds {t_ema - t_plain:7.1f} us   "
          f"separate lerp_ {t_lerp:7.1f} us ({12.0 * n / t_lerp / 1e6:5.2f} TB/s of 12 B/param)")
