#!/usr/bin/env python3
"""Micro-benchmark of the token-mix kernels:  python tools/bench_token_mix.py B N D [hid]   (default 256 196 768, hid = 2 D).

Prints, from one process, microseconds per call (device events around 20 calls after 3 warm-up calls) and TFLOP/s of
    the four left-multiply jobs (fc1, fc2, dU, dz) and the two weight gradients, 2 B hid N D flops each
    F.token_mix forward                4 B hid N D
    F.token_mix forward + backward    12 B hid N D
and of the YARDSTICK: the torch spelling of the reference's two lines (src/models/vit.py:269-271) in bf16 with the same
weights -- layer_norm, transpose, Linear, GELU, Linear, transpose, residual, with the transposing copies torch makes --
forward and forward + backward through torch's autograd.  The last line is the ratio yardstick / HIP (above 1: the HIP
block is faster).  The timings include launch overhead (what a training step pays)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402
from sfcvit import functional as F, ops  # noqa: E402

args = [int(v) for v in sys.argv[1:]]
B, N, D = args[:3] if len(args) >= 3 else (256, 196, 768)
hid = args[3] if len(args) > 3 else 2 * D
if not torch.cuda.is_available():
    raise SystemExit("bench_token_mix: needs the GPU; nothing is measured without one")
g = torch.Generator(device="cuda").manual_seed(0)
rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g).bfloat16()      # noqa: E731
x, dy = rnd(B, N, D), rnd(B, N, D)
ln_w, ln_b = rnd(D) * 0.1 + 1, rnd(D) * 0.1
w1, b1, w2, b2 = rnd(hid, N) * N ** -0.5, rnd(hid) * 0.1, rnd(N, hid) * hid ** -0.5, rnd(N) * 0.1
z = ops.layernorm_fwd(x.view(B * N, D), ln_w, ln_b)[0].view(B, N, D)
h, u = ops.tokmix_left(w1, z, bias=b1, act=ops.ACT_GELU, want_aux=True)
du = ops.tokmix_left(w2, dy, transposed=True, aux_in=u)


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


PARAMS = (ln_w, ln_b, w1, b1, w2, b2)


def leaves():
    return x.detach().requires_grad_(True), [t.detach().requires_grad_(True) for t in PARAMS]


def hip_fwd():
    with torch.no_grad():
        return F.token_mix(x, *PARAMS)


def hip_block():
    xr, ps = leaves()
    F.token_mix(xr, *ps).backward(dy)


def torch_lines(xr, ps):
    lw, lb, a1, c1, a2, c2 = ps
    t = TF.layer_norm(xr, (D,), lw, lb).transpose(1, 2)
    return xr + TF.linear(TF.gelu(TF.linear(t, a1, c1)), a2, c2).transpose(1, 2)


def torch_fwd():
    with torch.no_grad():
        return torch_lines(x, PARAMS)


def torch_block():
    xr, ps = leaves()
    torch_lines(xr, ps).backward(dy)


unit = 2.0 * B * hid * N * D
print(f"B={B} N={N} D={D} hid={hid}  hidden tensor {2 * B * hid * D / 1e6:.0f} MB  wgrad workspace "
      f"{ops.lib.sfcvit_tokmix_wgrad_workspace(B, hid, N, D) / 1e6:.1f} MB  device {torch.cuda.get_device_name(0)}")
rows = [("fc1  W1 z + b1, GELU, U kept", lambda: ops.tokmix_left(w1, z, bias=b1, act=ops.ACT_GELU, want_aux=True), unit),
        ("fc2  W2 H + b2 + x", lambda: ops.tokmix_left(w2, h, bias=b2, residual=x), unit),
        ("dU   (W2^T dy) gelu'(U)", lambda: ops.tokmix_left(w2, dy, transposed=True, aux_in=u), unit),
        ("dz   W1^T dU", lambda: ops.tokmix_left(w1, du, transposed=True), unit),
        ("dW1, db1", lambda: ops.tokmix_wgrad(du, z), unit),
        ("dW2, db2", lambda: ops.tokmix_wgrad(dy, h), unit)]
for name, fn, flops in rows:
    fn()
    kern = ops.last_tokmix_kernel()
    us = timeit(fn)
    print(f"{name:36s} {us:9.1f} us  {flops / us / 1e6:7.1f} TFLOP/s   [{kern}]")
res = {}
for name, fn, flops in (("token_mix forward (HIP)", hip_fwd, 2 * unit), ("yardstick forward (torch)", torch_fwd, 2 * unit),
                        ("token_mix fwd + bwd (HIP)", hip_block, 6 * unit), ("yardstick fwd + bwd (torch)", torch_block, 6 * unit),
                        ("token_mix fwd + bwd (HIP, again)", hip_block, 6 * unit)):
    res[name] = us = timeit(fn, 10)
    print(f"{name:36s} {us:9.1f} us  {flops / us / 1e6:7.1f} TFLOP/s")
hip = min(res["token_mix fwd + bwd (HIP)"], res["token_mix fwd + bwd (HIP, again)"])
print(f"ratio yardstick / HIP: forward {res['yardstick forward (torch)'] / res['token_mix forward (HIP)']:.3f}  "
      f"forward + backward {res['yardstick fwd + bwd (torch)'] / hip:.3f}")
