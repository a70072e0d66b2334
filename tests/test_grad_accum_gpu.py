"""Gradient accumulation on the GPU: the two kernels (sfcvit_grad_accum, sfcvit_grad_accum_finish) bit for bit against
tests/grad_accum_ref.py, FusedAdamW.accumulate() / fold() / step(), train_step(accum_steps=K) against one pass over the whole
batch, the once-per-optimizer-step state, and data parallelism with one exchange per optimizer step.

Bars.  acc and grad: bit equality with the numpy restatement (every operation is a single correctly rounded fp32 one, so there
is nothing to tolerate).  *sumsq: rtol 1e-4 of the fp64 sum of the squares of the stored bf16 values, the bar
tests/test_kernels_gpu.py::test_adamw_and_clip holds sumsq_accum to.  The clip + AdamW step behind a fold: that test's
atol 1e-6 / rtol 1e-5 on the master.  K micro-batches against one batch: the three bars of tests/test_distributed_gpu.py (two
half-batches on two ranks and two half-batches accumulated on one rank compute the same sum, and accumulation rounds it once
instead of twice).  Every test prints its figure before asserting."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

import grad_accum_ref as ref
from guarded import assert_guards_intact, guarded_inout, guarded_workspace
from oracle import formula, vit_oracle
from oracle.cases import MODEL_CASES
from test_distributed_gpu import LR, STEPS, _setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd")
BF16 = torch.bfloat16
SIZES = [1, 3, 4, 7, 2048, 2451, 3 * 2048 * 256 * 8 + 5]      # tail only, under-4, one group, remainder group, past the grid cap
SUMSQ_WS = 4096                                                # SFCVIT_SUMSQ_WORKSPACE_BYTES


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


# ---- 1. kernel bits ---------------------------------------------------------------------------------------------------------
def _micro_grads(n):
    """Three bf16 micro-batch gradients.  Magnitudes (|N(0, 1)| + 0.5) * 2^e, e in -2 .. 2 per element: at least 1 / 8.  Below
    2048 elements the three share each element's sign, so that the average is at least 1 / 8 in magnitude and s >= 2^-6 even
    for n = 1: the fp32 rounding of 2.5 + s (half an ulp of a number in [2, 4): 2^-23) is then under 8 % of the bar on s, and
    what the bar measures is the kernel's sum.  From 2048 on the signs are free (cancellation in the fp32 adds) and s >> 2.5."""
    gen = torch.Generator().manual_seed(7000 + n % 9973)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    out = []
    for _ in range(3):
        mag = (torch.randn(n, generator=gen).abs() + 0.5) * 2.0 ** torch.randint(-2, 3, (n,), generator=gen).float()
        if n >= 2048:
            sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        out.append((mag * sign).to(BF16))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_kernels_match_the_reference_bit_for_bit(ops, n):
    """K = 3 calls -- first, add, finish with the sum of squares -- on guarded buffers; acc starts as NaN (it is not read when
    first != 0), *sumsq starts at 2.5 and comes back as 2.5 + s; run twice: the same *sumsq bits."""
    from sfcvit import _lib
    lib, stream = _lib.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    grads = _micro_grads(n)
    bits = [_np_bits(g) for g in grads]
    want_acc1 = ref.accum(bits[0], None, True)
    want_acc2 = ref.accum(bits[1], want_acc1, False)
    want_grad, want_sumsq, _ = ref.fold(bits)
    runs = []
    for fill in (0xFF, 0x00):                                  # the workspace's content must not matter
        grad = guarded_inout("grad", grads[0].cuda())
        acc = guarded_inout("acc", torch.full((n,), float("nan"), device="cuda"))
        sumsq = guarded_inout("sumsq", torch.full((1,), 2.5, device="cuda"))
        ws = guarded_workspace("workspace", SUMSQ_WS, fill)
        bufs = [grad, acc, sumsq, ws]
        ops.grad_accum(grad.t, acc.t, True)
        assert np.array_equal(acc.t.cpu().numpy().view(np.uint32), want_acc1.view(np.uint32)), "first"
        grad.t.copy_(grads[1].cuda())
        ops.grad_accum(grad.t, acc.t, False)
        assert np.array_equal(acc.t.cpu().numpy().view(np.uint32), want_acc2.view(np.uint32)), "add"
        assert np.array_equal(_np_bits(grad.t), bits[1])       # grad is only read
        grad.t.copy_(grads[2].cuda())
        rc = lib.sfcvit_grad_accum_finish(grad.ptr(), acc.ptr(), n, float(ref.scale_of(3)), sumsq.ptr(), ws.ptr(), stream)
        assert rc == 0, lib.sfcvit_last_error().decode()
        torch.cuda.synchronize()
        assert_guards_intact(bufs, f"n {n}")
        assert np.array_equal(_np_bits(grad.t), want_grad), "finish"
        assert np.array_equal(acc.t.cpu().numpy().view(np.uint32), want_acc2.view(np.uint32))      # acc is only read
        runs.append(sumsq.t.clone())
    s = float(runs[0]) - 2.5
    ratio = abs(s - want_sumsq) / (1e-4 * want_sumsq)
    print(f"n {n}: s = {s:.6g}, fp64 sum of squares {want_sumsq:.6g}, |s - fp64| / (1e-4 * fp64) = {ratio:.4f}")
    assert want_sumsq >= 2.0 ** -6 and ratio <= 1.0
    assert _same_bits(runs[0], runs[1])
    # without a sum of squares: the same gradient bits, no workspace
    grad = guarded_inout("grad", grads[2].cuda())
    acc = guarded_inout("acc", torch.from_numpy(want_acc2).cuda())
    ops.grad_accum_finish(grad.t, acc.t, float(ref.scale_of(3)))
    torch.cuda.synchronize()
    assert_guards_intact([grad, acc], f"n {n}, no sumsq")
    assert np.array_equal(_np_bits(grad.t), want_grad)


def test_inf_and_nan_propagate(ops):
    g0 = torch.tensor([1.0, float("inf"), float("nan"), -2.0, 3.0e38, 1.0, 1.0, 1.0, 0.5], dtype=torch.float32).to(BF16)
    g1 = torch.tensor([1.0, 1.0, 1.0, float("-inf"), 3.0e38, 1.0, 1.0, 1.0, 0.5], dtype=torch.float32).to(BF16)
    want, want_sumsq, _ = ref.fold([_np_bits(g0), _np_bits(g1)])
    grad, acc, sumsq = g0.cuda(), torch.empty(9, device="cuda"), torch.zeros(1, device="cuda")
    ops.grad_accum(grad, acc, True)
    grad.copy_(g1)
    ops.grad_accum_finish(grad, acc, 0.5, sumsq)
    got = grad.float().cpu()
    print(got.tolist(), float(sumsq))
    assert np.array_equal(_np_bits(grad), want)
    assert torch.isinf(got[1]) and torch.isnan(got[2]) and got[3] == float("-inf") and torch.isinf(got[4]) and got[0] == 1.0
    assert torch.isnan(sumsq).all() and np.isnan(want_sumsq)   # the clip sees them as it does today


# ---- 2. the exact step ------------------------------------------------------------------------------------------------------
def _tiny(dropout=0.0):
    from sfcvit.models import VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    cfg, _ = MODEL_CASES["hilbert32_1d"]
    pe = HilbertEmbedding1D(cfg.img_size, cfg.patch_size, cfg.in_channels, cfg.embed_dim)
    model = VisionTransformer1D(pe, depth=cfg.depth, n_heads=cfg.n_heads, mlp_dim=cfg.mlp_dim, num_classes=cfg.num_classes,
                                dropout_p=dropout, head_dropout_p=dropout)
    model.load_state_dict(vit_oracle.formula_state(cfg))
    x = formula.image_batch(4, cfg.in_channels, cfg.img_size, cfg.img_size).cuda()
    tgt = formula.soft_targets(4, cfg.num_classes).cuda()
    return model.to("cuda", dtype=BF16), x, tgt


def _one_step(max_grad_norm, k):
    """One optimizer step on the same micro-batch taken k times (k = 1: a plain step).  A backward pass before it builds the
    flat layout, so that every measured pass writes the gradient slots in place, as every pass after a run's first does."""
    from sfcvit import functional as F
    from sfcvit.training import FusedAdamW
    model, x, tgt = _tiny()
    model.eval()
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2, max_grad_norm=max_grad_norm, ema_decay=0.5)
    F.soft_target_cross_entropy(model(x), tgt).backward()
    opt._build()
    opt.zero_grad()
    for j in range(k):
        F.soft_target_cross_entropy(model(x), tgt).backward()
        if j < k - 1:
            opt.accumulate()
    opt.step()
    return opt


@pytest.fixture(scope="module")
def plain_steps():
    return {mgn: _one_step(mgn, 1) for mgn in (None, 1e6)}


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("max_grad_norm", [None, 1e6], ids=["no-clip", "clip-1e6"])
def test_the_same_micro_batch_k_times_is_one_plain_step(plain_steps, max_grad_norm, k):
    """(g + g) / 2 and (g + g + g + g) / 4 are g exactly, so param, master, m, v and ema have the plain step's bits.  With
    max_grad_norm=1e6 the fused sum of squares runs and the clip coefficient is exactly 1."""
    want, got = plain_steps[max_grad_norm], _one_step(max_grad_norm, k)
    assert got.step_count == 1 and want.step_count == 1 and got.pending == 0 and got.acc is not None and want.acc is None
    for name in ("flat_grad", "flat_param", "master", "m", "v", "ema"):
        diff = int((_bits(getattr(got, name)) != _bits(getattr(want, name))).sum())
        print(f"K {k} max_grad_norm {max_grad_norm} {name}: differing elements {diff}")
        assert diff == 0, name
    assert float((got.ema - got.master).abs().max()) > 0       # the step moved the weights and the average followed half-way
    if max_grad_norm is not None:
        a, b = float(got.grad_norm()), float(want.grad_norm())
        print("grad_norm fused", a, "sumsq_accum", b)
        assert a > 0 and abs(a - b) <= 1e-4 * b                 # the norm of the averaged gradient


# ---- 3. the clip binds ------------------------------------------------------------------------------------------------------
def test_fold_with_sumsq_then_adamw_when_the_clip_binds(ops):
    """Raw flat buffers, random gradients of norm ~ 300 (far above max_norm 1), three optimizer steps of K = 3 micro-batches:
    fold-with-sumsq + adamw_step against grad_accum_ref + AdamW restated in float64."""
    gen = torch.Generator().manual_seed(8)
    n, k = 10007, 3
    hyper = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-5, max_norm=1.0)
    w0 = torch.randn(n, generator=gen)
    master, m, v = w0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    param, grad, acc, sumsq = master.to(BF16), torch.empty(n, device="cuda", dtype=BF16), torch.empty(n, device="cuda"), torch.zeros(1, device="cuda")
    w, m64, v64 = w0.double().numpy(), np.zeros(n), np.zeros(n)
    for step in range(1, 4):
        micro = [(torch.randn(n, generator=gen) * 3).to(BF16) for _ in range(k)]
        for j, g in enumerate(micro):
            grad.copy_(g)
            if j < k - 1:
                ops.grad_accum(grad, acc, j == 0)
        sumsq.zero_()
        ops.grad_accum_finish(grad, acc, float(ref.scale_of(k)), sumsq)
        ops.adamw_step(param, master, grad, m, v, sumsq, step=step, **hyper)
        avg_bits, ss, _ = ref.fold([_np_bits(g) for g in micro])
        g64 = ref.bf16_to_f32(avg_bits).astype(np.float64)
        norm = np.sqrt(ss)
        assert norm > 100
        g64 = g64 * min(1.0, hyper["max_norm"] / (norm + 1e-6))
        w = w * (1 - hyper["lr"] * hyper["weight_decay"])
        m64 = hyper["beta1"] * m64 + (1 - hyper["beta1"]) * g64
        v64 = hyper["beta2"] * v64 + (1 - hyper["beta2"]) * g64 * g64
        bc1, bc2 = 1 - hyper["beta1"] ** step, 1 - hyper["beta2"] ** step
        w = w - hyper["lr"] / bc1 * m64 / (np.sqrt(v64) / np.sqrt(bc2) + hyper["eps"])
        got = master.double().cpu().numpy()
        worst = float((np.abs(got - w) / (1e-6 + 1e-5 * np.abs(w))).max())
        print(f"step {step}: gradient norm {norm:.1f}, worst |err| / (atol 1e-6 + rtol 1e-5 |w|) = {worst:.4f}")
        assert worst <= 1.0
        assert np.array_equal(_np_bits(grad), avg_bits) and torch.equal(param, master.to(BF16))
    assert float(np.abs(w - w0.double().numpy()).max()) > 1e-4  # the steps moved the weights


# ---- 4. K micro-batches equal one batch ---------------------------------------------------------------------------------------
def _run(accum_steps):
    from sfcvit.training import FusedAdamW, train_step
    model, x, tgt = _setup()
    init = {k: v.detach().clone().bfloat16().float() for k, v in model.named_parameters()}
    model = model.to("cuda", dtype=BF16).eval()                 # dropout off: the runs must see the same function
    opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=5e-2, max_grad_norm=1.0)
    losses = [float(train_step(model, x.cuda(), tgt.cuda(), opt, accum_steps=accum_steps)) for _ in range(STEPS)]
    names = {id(p): k for k, p in model.named_parameters()}
    master = {names[id(p)]: opt.master[o:o + p.numel()].view(p.shape).cpu() for p, o in zip(opt.active, opt.offsets)}
    return losses, master, init, opt


@pytest.fixture(scope="module")
def one_pass():
    """Batch 8 in one pass, STEPS steps: computed once, shared and left unchanged."""
    return _run(1)


def _three_bars(master, got, init, what):
    confident = total = 0
    worst = 0.0
    for k, w in master.items():
        upd, acc = (w - init[k]).flatten(), (got[k] - init[k]).flatten()
        worst = max(worst, float((upd - acc).abs().max()) / (2.1 * LR * STEPS))
        mask = upd.abs() >= 0.8 * LR * STEPS
        confident += int(mask.sum())
        total += mask.numel()
        if int(mask.sum()) >= 8:
            agree = float((torch.sign(upd[mask]) == torch.sign(acc[mask])).float().mean())
            assert agree >= 0.9, (what, k, agree)
    print(f"{what}: worst |update difference| / (2.1 * LR * STEPS) = {worst:.4f}, confident elements {confident} of {total}")
    assert worst <= 1.0, what
    assert confident >= 0.1 * total, what


@pytest.mark.parametrize("k", [2, 4])
def test_k_micro_batches_match_one_pass_over_the_batch(one_pass, k):
    losses, master, init, _ = one_pass
    got_losses, got, _, opt = _run(k)
    assert opt.step_count == STEPS and opt.pending == 0
    for s in range(STEPS):                                      # the mean of the micro-batch losses is the batch loss
        assert abs(got_losses[s] - losses[s]) <= 1e-2 * abs(losses[s]) + 2e-3, (s, got_losses, losses)
    _three_bars(master, got, init, f"accum_steps {k}")


def test_an_optimizer_that_never_accumulates_allocates_nothing(one_pass):
    opt = one_pass[3]
    assert opt.acc is None and opt.pending == 0 and opt.step_count == STEPS


# ---- 5. once per optimizer step -------------------------------------------------------------------------------------------------
def test_step_state_scheduler_and_masks_advance_per_optimizer_step():
    """Device step state in use, dropout 0.1, train mode: begin_step() once, two passes over the SAME images.  The device
    counter, step_count and the scheduler advance by one; the two passes draw different masks (different logits)."""
    from sfcvit import functional as F
    from sfcvit import ops
    from sfcvit.training import AccumSteps, FusedAdamW, WarmupCosine
    model, x, tgt = _tiny(dropout=0.1)
    model.train()
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2)
    try:
        opt.use_device_state(seed_base=4242)
        sched = WarmupCosine(opt, 2, 10)
        seq = AccumSteps(opt, sched, None, n_batches=2, accum_steps=2)
        logits = []
        for j in range(2):
            seq.begin(j)
            out = model(x)
            seq.backward(F.soft_target_cross_entropy(out, tgt))
            stepped = seq.end()
            assert stepped == (j == 1)
            logits.append(out.detach().float())
        state = opt.dev_state.cpu()
        differing = int((logits[0] != logits[1]).sum())
        print("dev_state", state.tolist()[:2], "step_count", opt.step_count, "scheduler n", sched.n, "logits differing", differing, "of",
              logits[0].numel())
        assert int(state[1]) == 1 and opt.step_count == 1 and sched.n == 1 and opt.pending == 0
        assert differing > 0
        assert opt.lr == sched.lr_at(1)
        seq.begin(0)                                            # the next optimizer step advances the counter again
        assert int(opt.dev_state[1]) == 2
    finally:
        opt.release_device_state()
        ops.STEP_STATE = None


class _Loader:
    def __init__(self, x, y, batch):
        self.batches = [(x[i:i + batch], y[i:i + batch]) for i in range(0, len(x), batch)]
        self.dataset = range(len(x))

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


@pytest.mark.parametrize("loop", ["host-mix", "device-mix", "plain"])
def test_epoch_loops_step_once_per_group_of_loader_batches(loop):
    """Five loader batches of 4 with accum_steps=2: three optimizer steps (the last on one batch), three scheduler steps,
    nothing left pending, finite loss."""
    import math
    from sfcvit.training import FusedAdamW, SoftTargetCrossEntropy, WarmupCosine
    from sfcvit.training.loops import train_with_mixup_or_cutmix, train_with_scheduler
    model, _, _ = _tiny(dropout=0.1)
    cfg, _ = MODEL_CASES["hilbert32_1d"]
    x = formula.image_batch(20, cfg.in_channels, cfg.img_size, cfg.img_size)
    y = torch.arange(20) % cfg.num_classes
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2)
    sched = WarmupCosine(opt, 1, 6)
    np.random.seed(0)
    torch.manual_seed(0)
    if loop == "plain":
        loss, acc = train_with_scheduler(model, _Loader(x, y, 4), torch.nn.CrossEntropyLoss(), opt, sched, "cuda", accum_steps=2)
    else:
        loss, acc = train_with_mixup_or_cutmix(model, _Loader(x, y, 4), SoftTargetCrossEntropy(), opt, sched, "cuda",
                                               device_mix=loop == "device-mix", accum_steps=2)
    print(loop, "loss", loss, "accuracy", acc, "steps", opt.step_count, "scheduler", sched.n)
    assert opt.step_count == 3 and sched.n == 3 and opt.pending == 0 and opt.acc is not None
    assert math.isfinite(loss) and 0.0 <= acc <= 1.0
    assert bool(torch.isfinite(opt.master).all()) and float(opt.grad_norm()) > 0


# ---- 6. data parallel: two gloo ranks on card 0 ---------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from sfcvit.training import FusedAdamW, GradReducer, train_step
    from sfcvit.training.distributed import dist_timeout
    torch.cuda.set_device(0)                                    # the gloo rehearsal: both ranks share card 0
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=dist_timeout())
    model, x, tgt = _setup()
    per = x.shape[0] // world
    x, tgt = x[rank * per:(rank + 1) * per].to(dev), tgt[rank * per:(rank + 1) * per].to(dev)
    model = model.to(dev, dtype=BF16).eval()
    opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=5e-2, max_grad_norm=1.0)
    red = GradReducer(opt, bucket_bytes=1 << 16)                # overlap=True: its hooks stay silent in a step that accumulates
    losses = [float(train_step(model, x, tgt, opt, reducer=red, accum_steps=2)) for _ in range(STEPS)]   # each wait bounded by SFCVIT_DIST_TIMEOUT
    names = {id(p): k for k, p in model.named_parameters()}
    master = {names[id(p)]: opt.master[o:o + p.numel()].view(p.shape).cpu() for p, o in zip(opt.active, opt.offsets)}
    torch.save({"losses": losses, "master": master, "buckets": len(red.buckets), "exchanges": red.step_no}, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_of_two_micro_batches_match_one_rank_in_one_pass(tmp_path, one_pass):
    """Batch 8 as 2 ranks x 2 micro-batches of 2, gradients exchanged once per optimizer step through the host-staged gloo
    mode, against one rank taking the same steps on the whole batch in one pass."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "rank")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert r0["buckets"] > 1 and r0["exchanges"] == r1["exchanges"] == STEPS      # one exchange per optimizer step
    for k in r0["master"]:
        assert torch.equal(r0["master"][k], r1["master"][k]), k                    # replicas stay bit-identical
    losses, master, init, _ = one_pass
    for s in range(STEPS):
        assert abs(0.5 * (r0["losses"][s] + r1["losses"][s]) - losses[s]) <= 1e-2 * abs(losses[s]) + 2e-3
    _three_bars(master, r0["master"], init, "2 ranks x 2 micro-batches")
