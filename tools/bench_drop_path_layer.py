#!/usr/bin/env python3
"""One encoder layer, forward + backward, with and without stochastic depth at ViT-B's shape (B 256, N 196, D 768, H 12, F 3072,
dropout 0.1; or `B N D H F` on the command line): the two variants alternate, ROUNDS rounds (default 7) of 10 steps each, timed
with HIP events; prints the median ms per step of each with the spread, and the difference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
import sfcvit.functional as F  # noqa: E402

B, N, D, H, Fd = (int(v) for v in sys.argv[1:6]) if len(sys.argv) > 5 else (256, 196, 768, 12, 3072)
ROUNDS, STEPS, P, RATE = 7, 10, 0.1, 0.1
g = torch.Generator(device="cuda").manual_seed(0)
r = lambda *s, sc=1.0: (torch.randn(*s, device="cuda", generator=g) * sc).bfloat16().requires_grad_(True)      # noqa: E731
x, dy = r(B, N, D), r(B, N, D).detach()
params = [r(3 * D, D, sc=D ** -0.5), r(3 * D, sc=0.1), r(D, D, sc=D ** -0.5), r(D, sc=0.1), r(D), r(D, sc=0.1),
          r(Fd, D, sc=D ** -0.5), r(Fd, sc=0.1), r(D, Fd, sc=Fd ** -0.5), r(D, sc=0.1), r(D), r(D, sc=0.1)]


def step(rate):
    for t in [x] + params:
        t.grad = None
    F.encoder_layer(x, *params, H, dropout_p=P, **({"drop_path": rate} if rate else {})).backward(dy)


def timeit(rate):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        step(rate)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS


for rate in (0.0, RATE):
    for _ in range(3):
        step(rate)
times = {0.0: [], RATE: []}
for _ in range(ROUNDS):
    for rate in times:
        times[rate].append(timeit(rate))
med = {}
for rate, t in times.items():
    t = sorted(t)
    med[rate] = t[len(t) // 2]
    print(f"drop_path {rate}: {med[rate]:.3f} ms per forward + backward [{t[0]:.3f} .. {t[-1]:.3f}] over {ROUNDS} rounds of {STEPS}")
extra = 2 * B * N * D * 2
print(f"difference {1e3 * (med[RATE] - med[0.0]):+.1f} us; the byte count predicts one extra pass of {extra / 2e6:.0f} MB per site "
      f"forward ({extra / 1e6:.0f} MB per layer), none backward")
