#!/usr/bin/env python3
"""One encoder layer, forward + backward, post-norm and pre-norm at ViT-B's shape (B 256, N 196, D 768, H 12, F 3072, dropout 0.1;
or `B N D H F` on the command line): post-norm (F.encoder_layer), pre-norm ReLU, pre-norm GELU, pre-norm GELU with LayerScale, and
the same four with DropPath 0.1.  The variants alternate, ROUNDS rounds (default 7) of 10 steps each, timed with HIP events; prints
the median ms per step of each with the spread and the difference to the post-norm line of the same DropPath setting.  Plain
pre-norm ReLU runs the post-norm layer's kernels, so its line is the check that the composition costs nothing."""
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
x, dy, dn = r(B, N, D), r(B, N, D).detach(), r(B, N, D).detach()
n = torch.nn.functional.layer_norm(x.detach().float(), (D,)).bfloat16().requires_grad_(True)
params = [r(3 * D, D, sc=D ** -0.5), r(3 * D, sc=0.1), r(D, D, sc=D ** -0.5), r(D, sc=0.1), r(D), r(D, sc=0.1),
          r(Fd, D, sc=D ** -0.5), r(Fd, sc=0.1), r(D, Fd, sc=Fd ** -0.5), r(D, sc=0.1), r(D), r(D, sc=0.1)]
lam = r(2, D, sc=0.1)

# name -> (pre-norm?, activation, LayerScale?, DropPath rate)
VARIANTS = {}
for rate in (0.0, RATE):
    tag = f", drop path {rate}" if rate else ""
    VARIANTS["post-norm relu" + tag] = (False, "relu", False, rate)
    VARIANTS["pre-norm relu" + tag] = (True, "relu", False, rate)
    VARIANTS["pre-norm gelu" + tag] = (True, "gelu", False, rate)
    VARIANTS["pre-norm gelu + layer scale" + tag] = (True, "gelu", True, rate)


def step(pre, act, scale, rate):
    for t in [x, n, lam] + params:
        t.grad = None
    path = {"drop_path": rate} if rate else {}
    if not pre:
        F.encoder_layer(x, *params, H, dropout_p=P, **path).backward(dy)
        return
    s2, n2 = F.pre_norm_layer(x, n, *params, H, dropout_p=P, activation=act, layer_scale=lam if scale else None, **path)
    torch.autograd.backward([s2, n2], [dy, dn])


def timeit(v):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        step(*v)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS


for v in VARIANTS.values():
    for _ in range(3):
        step(*v)
times = {k: [] for k in VARIANTS}
for _ in range(ROUNDS):
    for k, v in VARIANTS.items():
        times[k].append(timeit(v))
med = {}
print(f"B {B} N {N} D {D} H {H} F {Fd}, dropout {P}; median ms per forward + backward of {ROUNDS} rounds of {STEPS} [min .. max]")
for k, t in times.items():
    t = sorted(t)
    med[k] = t[len(t) // 2]
    base = med["post-norm relu" + (k[k.index(", drop path"):] if ", drop path" in k else "")]
    print(f"{k:44s} {med[k]:7.3f} ms [{t[0]:7.3f} .. {t[-1]:7.3f}]  {1e3 * (med[k] - base):+7.1f} us against post-norm")
