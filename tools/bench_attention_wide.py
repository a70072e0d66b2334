#!/usr/bin/env python3
"""Attention kernels for head dims 128 / 192 / 256, alone, in ONE process: forward and backward timed with HIP events
after warm-up.  At a shape both families take (B 64, N 256, H 4, hd 128) the streaming kernels (SFCVIT_ATTN_WIDE_STREAM=1)
and the whole-sequence kernels run alternately; then the shapes only the streaming kernels take.  torch's own
scaled_dot_product_attention at the same shapes is printed as context where it runs.
    python tools/bench_attention_wide.py [--rounds 5] [--reps 20]
FLOP counted: forward 4 B H N^2 hd, backward 2.5 x that."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd"))
import torch  # noqa: E402
from sfcvit import ops  # noqa: E402

ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
SHARED = (64, 256, 4, 128)
STREAM_ONLY = [(64, 256, 4, 192), (64, 576, 8, 128), (8, 3136, 4, 192)]


def timeit(fn, reps=REPS):
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


def setup(B, N, H, hd):
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B, N, 3 * H * hd, device="cuda", generator=g).bfloat16()
    dout = torch.randn(B, N, H * hd, device="cuda", generator=g).bfloat16()
    out, lse = ops.attention_fwd(qkv, H, any_length=True)
    return qkv, dout, out, lse


def kernels(B, N, H, hd, stream):
    """(fwd fn, bwd fn, kernel names) with SFCVIT_ATTN_WIDE_STREAM set for the calls (read per call by the library)"""
    qkv, dout, out, lse = setup(B, N, H, hd)

    def with_switch(fn):
        def run():
            os.environ["SFCVIT_ATTN_WIDE_STREAM"] = "1" if stream else "0"
            try:
                return fn()
            finally:
                os.environ.pop("SFCVIT_ATTN_WIDE_STREAM", None)
        return run
    fwd = with_switch(lambda: ops.attention_fwd(qkv, H, any_length=True))
    bwd = with_switch(lambda: ops.attention_bwd(qkv, out, lse, dout, H, any_length=True))
    fwd()
    kf = ops.last_attn_kernel()
    bwd()
    return fwd, bwd, (kf, ops.last_attn_kernel())


def sdpa(B, N, H, hd):
    """torch's scaled_dot_product_attention at the same shape (bf16, [B, H, N, hd]): (fwd fn, fwd + bwd fn) or None."""
    try:
        g = torch.Generator(device="cuda").manual_seed(0)
        q, k, v = (torch.randn(B, H, N, hd, device="cuda", generator=g).bfloat16().requires_grad_(True) for _ in range(3))
        do = torch.randn(B, H, N, hd, device="cuda", generator=g).bfloat16()
        f = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v)          # noqa: E731
        fb = lambda: torch.autograd.grad(f(), (q, k, v), do)                            # noqa: E731
        fb()
        return f, fb
    except Exception as e:                                                              # context only, never a gate
        print(f"  torch SDPA at B={B} N={N} H={H} hd={hd}: not run ({type(e).__name__}: {str(e)[:80]})")
        return None


def report(label, B, N, H, hd, fwd_us, bwd_us):
    fl = 4.0 * B * H * N * N * hd
    med = lambda v: sorted(v)[len(v) // 2]                                              # noqa: E731
    f, b = med(fwd_us), med(bwd_us)
    print(f"  {label:44s} fwd {f:9.1f} us ({fl / f / 1e6:6.1f} TFLOP/s, min {min(fwd_us):8.1f})   "
          f"bwd {b:9.1f} us ({2.5 * fl / b / 1e6:6.1f} TFLOP/s, min {min(bwd_us):8.1f})")
    return f, b


def main():
    print(f"rounds {ROUNDS}, {REPS} launches per timing; medians over rounds")
    B, N, H, hd = SHARED
    print(f"B={B} N={N} H={H} hd={hd}: streaming vs whole-sequence kernels, alternating")
    runs = {s: kernels(B, N, H, hd, s) for s in (True, False)}
    times = {s: ([], []) for s in runs}
    for _ in range(ROUNDS):
        for s in (True, False):
            times[s][0].append(timeit(runs[s][0]))
            times[s][1].append(timeit(runs[s][1]))
    res = {s: report(" / ".join(runs[s][2]), B, N, H, hd, *times[s]) for s in (True, False)}
    print(f"  streaming / whole-sequence time: fwd {res[True][0] / res[False][0]:.2f}x, bwd {res[True][1] / res[False][1]:.2f}x")
    ctx = sdpa(B, N, H, hd)
    if ctx:
        report("torch SDPA (context; bwd column = fwd + bwd)", B, N, H, hd, [timeit(ctx[0]) for _ in range(ROUNDS)],
               [timeit(ctx[1]) for _ in range(ROUNDS)])
    for B, N, H, hd in STREAM_ONLY:
        print(f"B={B} N={N} H={H} hd={hd}")
        fwd, bwd, names = kernels(B, N, H, hd, False)
        report(" / ".join(names), B, N, H, hd, [timeit(fwd) for _ in range(ROUNDS)], [timeit(bwd) for _ in range(ROUNDS)])
        ctx = sdpa(B, N, H, hd)
        if ctx:
            report("torch SDPA (context; bwd column = fwd + bwd)", B, N, H, hd, [timeit(ctx[0]) for _ in range(ROUNDS)],
                   [timeit(ctx[1]) for _ in range(ROUNDS)])


if __name__ == "__main__":
    main()
