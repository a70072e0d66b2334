#!/usr/bin/env python3
"""The gradient-accumulation kernels alone, next to the kernels they sit beside, at ViT-B (86.6 M) and ViT-L (304.3 M)
parameter counts -- the method of tools/bench_adamw.py: one process per line (one size each), warmed, HIP events, the cases
alternating in one process, median of the windows with [min .. max].    python tools/bench_grad_accum.py [n_params]

    grad_accum first       acc = float(grad)                      6 B / parameter (2 read, 4 written)
    grad_accum             acc += float(grad)                    10 B            (2 + 4 read, 4 written)
    grad_accum_finish      grad = bf16((acc + grad) * scale),     8 B            (2 + 4 read, 2 written)
                           sum of squares in the same pass
    sumsq_accum            the clip's sum of squares              2 B
    adamw_step             fused clip + AdamW                    28 B            the yardstick: its bytes per second in THIS process
and the step-level pair: "finish with sumsq" against "grad_accum + sumsq_accum", the unfused alternative for the last
micro-batch (which would still owe the pass that writes the average).  Without an argument it runs itself once per size."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [86_567_656, 304_330_000]

if len(sys.argv) < 2:
    for n in SIZES:
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), str(n)])
        if rc:
            sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
from sfcvit import ops  # noqa: E402

n = int(sys.argv[1]) // 8 * 8
master = torch.randn(n, device="cuda")
param = master.bfloat16()
grad = (torch.randn(n, device="cuda") * 1e-2).bfloat16()
m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
acc, zero = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
sumsq = torch.ones(1, device="cuda")
hyper = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-5, max_norm=1.0)
step_no = [0]


def adamw():
    step_no[0] += 1
    ops.adamw_step(param, master, grad, m, v, sumsq, step=step_no[0], **hyper)


def finish():                  # scale 1 onto a zero sum: the gradient keeps its values from call to call
    ops.grad_accum_finish(grad, zero, 1.0, sumsq)


def unfused():
    ops.grad_accum(grad, acc, False)
    ops.sumsq_accum(grad, sumsq)


CASES = [("grad_accum first", 6, lambda: ops.grad_accum(grad, acc, True)),
         ("grad_accum", 10, lambda: ops.grad_accum(grad, acc, False)),
         ("grad_accum_finish + sumsq", 8, finish),
         ("sumsq_accum", 2, lambda: ops.sumsq_accum(grad, sumsq)),
         ("adamw_step", 28, adamw),
         ("grad_accum + sumsq_accum", 12, unfused)]


def windows(fn, count=5, calls=10):
    """Microseconds per call of `count` windows of `calls` calls (device events), after three warm calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(count):
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / calls * 1e3)
    return ts


times = {name: [] for name, _, _ in CASES}
for _ in range(2):             # the cases alternate: two rounds over all of them in one process
    for name, _, fn in CASES:
        times[name] += windows(fn)
    acc.zero_()
med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
yard = 28.0 * n / med["adamw_step"] / 1e6
print(f"n = {n / 1e6:.1f} M parameters; yardstick adamw_step {yard:.2f} TB/s of its 28 B/param in this process")
for name, nbytes, _ in CASES:
    t = times[name]
    rate = nbytes * n / med[name] / 1e6
    print(f"  {name:28s} {med[name]:8.1f} us [{min(t):8.1f} .. {max(t):8.1f}]   {rate:5.2f} TB/s of {nbytes:2d} B/param   {rate / yard:5.3f} of the yardstick")
fused, alt = med["grad_accum_finish + sumsq"], med["grad_accum + sumsq_accum"]
print(f"  last micro-batch: finish with sumsq {fused:.1f} us against grad_accum + sumsq_accum {alt:.1f} us: the pair costs {alt - fused:+.1f} us "
      f"(fused / pair {fused / alt:.3f}), and the pair has not yet written the average")
