"""TokenAggregator on the GPU: the depth-wise sequence convolution kernels (sfcvit_dwconv1d_fwd / _bwd), F.token_aggregator,
the module, the models' `token_aggregator` option and main.py --token-aggregator.

Reference: fp64 torch on the CPU (tests/token_agg_ref.py) evaluated on the SAME bf16-rounded inputs.
Bounds (from the number formats, not from measurements):
    u, dx         |err| <= 2^-8 |ref| + (k + 1) 2^-23 (|bias| + sum_t |w x|)
                  one bf16 rounding is 2^-9 relative, an fp32 sum of k + 1 terms at most (k + 1) 2^-24 of the absolute
                  sum; both doubled
    fp32 dw, db   |err| <= R 2^-24 sum |terms|, R = B * Nout terms: the worst case of any summation order
    bf16 dw, db   the fp32 bound + 2^-8 |ref|
Exact-answer inputs (small integers and halves) must come out bit for bit.  Every test prints its figure before asserting."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from oracle import formula
from oracle.cases import MODEL_CASES
from token_agg_ref import aggregator_ref, case_inputs, dwconv_abs_ref, dwconv_grads_ref, dwconv_ref, load_fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16

# (B, N, D, k, s): N < k, one row, D not a multiple of the 256-channel slab, more than one slab, k = 1, the ViT-B width with
# an odd N, even k (Nout = N + 1), strides
EXACT_SHAPES = [(2, 1, 8, 3, 1), (2, 2, 8, 5, 1), (2, 5, 72, 3, 1), (3, 64, 192, 3, 1), (2, 65, 200, 1, 1), (2, 197, 768, 3, 1),
                (2, 9, 16, 2, 1), (2, 9, 16, 4, 2), (2, 13, 24, 9, 4)]
IDS = ["B%d-N%d-D%d-k%d-s%d" % s for s in EXACT_SHAPES]


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def _exact_inputs(B, N, D, k, s, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + N * 7 + D)
    n_out = (N + 2 * (k // 2) - k) // s + 1
    x = torch.randint(-2, 3, (B, N, D), generator=g).float()
    w = torch.randint(-2, 3, (D, k), generator=g).float() / 2
    b = torch.randint(-1, 2, (D,), generator=g).float()
    du = torch.randint(-2, 3, (B, n_out, D), generator=g).float()
    return x, w, b, du


def _random_inputs(B, N, D, k, s, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    n_out = (N + 2 * (k // 2) - k) // s + 1
    r = lambda *shape: torch.randn(*shape, generator=g).to(BF16).float()      # noqa: E731  (bf16-rounded values, held in fp32)
    return r(B, N, D), r(D, k) * 0.5, r(D), r(B, n_out, D)


def _dev(*ts):
    return [t.to(BF16).cuda() for t in ts]


# ---- 1. exact answers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=IDS)
def test_exact_inputs_give_exact_answers(shape, ops):
    B, N, D, k, s = shape
    x, w, b, du = _exact_inputs(*shape)
    u_ref, dx_ref, dw_ref, db_ref = dwconv_grads_ref(x, w, b, du, s)
    assert torch.equal(u_ref.to(BF16).double(), u_ref) and torch.equal(dx_ref.to(BF16).double(), dx_ref)   # representable
    xd, wd, bd, dud = _dev(x, w, b, du)
    u = ops.dwconv1d_fwd(xd, wd, bd, s)
    dx, dw, db = ops.dwconv1d_bwd(dud, xd, wd, s)
    assert u.shape == u_ref.shape and u.dtype == BF16 and dx.shape == x.shape
    assert dw.dtype == torch.float32 and dw.shape == (D, k) and db.shape == (D,)
    bad = {"u": int((u.cpu().double() != u_ref).sum()), "dx": int((dx.cpu().double() != dx_ref).sum()),
           "dw": int((dw.cpu().double() != dw_ref).sum()), "db": int((db.cpu().double() != db_ref).sum())}
    print(shape, ops.last_dwconv_kernel(), "elements that differ:", bad)
    assert not any(bad.values()), bad
    # the Conv1d parameter layout [D, 1, k] is the same memory
    assert torch.equal(ops.dwconv1d_fwd(xd, wd.view(D, 1, k), bd, s), u)


@pytest.mark.parametrize("shape", [(2, 5, 72, 3, 1), (2, 13, 24, 9, 4), (2, 9, 16, 4, 2)], ids=["k3", "k9s4", "k4s2"])
def test_nothing_leaks_across_the_batch_boundary(shape, ops):
    B, N, D, k, s = shape
    x = torch.zeros(B, N, D)
    x[0] = 2.0
    _, w, b, du = _exact_inputs(*shape)
    w = w.abs() + 0.5                                            # every tap non-zero: a leak would show
    xd, wd, bd = _dev(x, w, b)
    u = ops.dwconv1d_fwd(xd, wd, bd, s).cpu().float()
    assert torch.equal(u[1], b.expand_as(u[1])), "image 1 (all zero) must come out as the bias"
    assert torch.equal(u.double(), dwconv_ref(x, w, b, s))
    du = torch.zeros_like(du)
    du[0] = 1.0
    dx, _, _ = ops.dwconv1d_bwd(du.to(BF16).cuda(), xd, wd, s)
    assert float(dx[1].abs().max()) == 0.0


# ---- 2. random inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 197, 768, 3, 1), (2, 50, 256, 5, 2)], ids=["vitb-k3", "k5s2"])
def test_random_inputs_within_the_format_bounds(shape, ops):
    B, N, D, k, s = shape
    x, w, b, du = _random_inputs(*shape)
    ref = dwconv_grads_ref(x, w, b, du, s)
    mag = dwconv_abs_ref(x, w, b, du, s)
    xd, wd, bd, dud = _dev(x, w, b, du)
    u = ops.dwconv1d_fwd(xd, wd, bd, s)
    dx, dw, db = ops.dwconv1d_bwd(dud, xd, wd, s)
    dwb, dbb = torch.empty(D, k, device="cuda", dtype=BF16), torch.empty(D, device="cuda", dtype=BF16)
    _, dwb2, dbb2 = ops.dwconv1d_bwd(dud, xd, wd, s, want_dx=False, out=(dwb, dbb))
    assert dwb2 is dwb and dbb2 is dbb
    R = B * u.shape[1]
    row = (k + 1) * 2.0 ** -23
    # dx has no bias term: its magnitude sum is mag[1] as it stands; u's includes |bias| (dwconv_abs_ref adds it)
    checks = [("u", u, ref[0], 2.0 ** -8 * ref[0].abs() + row * mag[0]),
              ("dx", dx, ref[1], 2.0 ** -8 * ref[1].abs() + row * mag[1]),
              ("dw", dw, ref[2], R * 2.0 ** -24 * mag[2]),
              ("db", db, ref[3], R * 2.0 ** -24 * mag[3]),
              ("dw bf16", dwb, ref[2], R * 2.0 ** -24 * mag[2] + 2.0 ** -8 * ref[2].abs()),
              ("db bf16", dbb, ref[3], R * 2.0 ** -24 * mag[3] + 2.0 ** -8 * ref[3].abs())]
    worst = {}
    for name, got, want, bound in checks:
        err = (got.cpu().double() - want).abs()
        worst[name] = float((err / bound.clamp_min(1e-300)).max())
    print(shape, "worst err / bound:", worst)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_two_runs_give_the_same_bits(ops):
    shape = (2, 197, 768, 3, 1)
    xd, wd, bd, dud = _dev(*_random_inputs(*shape, seed=3))
    a = (ops.dwconv1d_fwd(xd, wd, bd, 1), *ops.dwconv1d_bwd(dud, xd, wd, 1))
    b = (ops.dwconv1d_fwd(xd, wd, bd, 1), *ops.dwconv1d_bwd(dud, xd, wd, 1))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---- 3. guards and NULL outputs --------------------------------------------------------------------------------------------
GUARD = 256


def _guarded(n, dtype):
    """n elements with GUARD sentinel elements on both sides -> (whole buffer, the n-element view)."""
    fill = 0xA5 if dtype == torch.uint8 else float("nan")
    flat = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return flat, flat[GUARD:GUARD + n]


def _guards_intact(flat, n):
    g = torch.cat([flat[:GUARD], flat[GUARD + n:]])
    return bool((g == 0xA5).all()) if flat.dtype == torch.uint8 else bool(torch.isnan(g).all())


@pytest.mark.parametrize("shape", [(2, 5, 72, 3, 1), (1, 65, 200, 4, 2)], ids=["k3", "k4s2"])
def test_nothing_is_written_outside_the_outputs_or_the_workspace(shape, ops):
    from sfcvit._lib import check, lib
    B, N, D, k, s = shape
    x, w, b, du = _exact_inputs(*shape)
    ref = dwconv_grads_ref(x, w, b, du, s)
    xd, wd, bd, dud = _dev(x, w, b, du)
    n_out = du.shape[1]
    p = lambda t: ctypes.c_void_p(t.data_ptr())                # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    u_flat, u = _guarded(B * n_out * D, BF16)
    check(lib.sfcvit_dwconv1d_fwd(p(xd), p(wd), p(bd), p(u), B, N, D, k, s, st), "fwd")
    nbytes = lib.sfcvit_dwconv1d_bwd_workspace(B, N, D, k, s)
    ws_flat, ws = _guarded(nbytes, torch.uint8)
    dx_flat, dx = _guarded(B * N * D, BF16)
    dw_flat, dw = _guarded(D * k, torch.float32)
    db_flat, db = _guarded(D, torch.float32)
    check(lib.sfcvit_dwconv1d_bwd(p(dud), p(xd), p(wd), p(dx), p(dw), p(db), 0, B, N, D, k, s, p(ws), nbytes, st), "bwd")
    torch.cuda.synchronize()
    for name, flat, n in (("u", u_flat, u.numel()), ("dx", dx_flat, dx.numel()), ("dw", dw_flat, dw.numel()),
                          ("db", db_flat, db.numel()), ("workspace", ws_flat, nbytes)):
        assert _guards_intact(flat, n), name
    assert torch.equal(u.cpu().double().view(ref[0].shape), ref[0]) and torch.equal(dx.cpu().double().view(ref[1].shape), ref[1])
    assert torch.equal(dw.cpu().double().view(D, k), ref[2]) and torch.equal(db.cpu().double(), ref[3])
    # bf16 gradient outputs: exactly D * k and D elements
    dwb_flat, dwb = _guarded(D * k, BF16)
    dbb_flat, dbb = _guarded(D, BF16)
    check(lib.sfcvit_dwconv1d_bwd(p(dud), p(xd), p(wd), None, p(dwb), p(dbb), 1, B, N, D, k, s, p(ws), nbytes, st), "bwd bf16")
    torch.cuda.synchronize()
    assert _guards_intact(dwb_flat, D * k) and _guards_intact(dbb_flat, D) and _guards_intact(ws_flat, nbytes)
    assert not torch.isnan(dwb.float()).any() and not torch.isnan(dbb.float()).any()


@pytest.mark.parametrize("shape", [(2, 37, 72, 3, 1), (2, 13, 24, 5, 2)], ids=["k3", "k5s2"])
def test_null_outputs_skip_that_output_only(shape, ops):
    B, N, D, k, s = shape
    xd, wd, bd, dud = _dev(*_random_inputs(*shape, seed=5))
    dx, dw, db = ops.dwconv1d_bwd(dud, xd, wd, s)
    a = ops.dwconv1d_bwd(dud, xd, wd, s, want_dx=False)
    assert a[0] is None and torch.equal(a[1], dw) and torch.equal(a[2], db)
    a = ops.dwconv1d_bwd(dud, xd, wd, s, want_dw=False, want_db=False)
    assert a[1] is None and a[2] is None and torch.equal(a[0], dx)
    a = ops.dwconv1d_bwd(dud, xd, wd, s, want_dw=False)
    assert a[1] is None and torch.equal(a[0], dx) and torch.equal(a[2], db)
    a = ops.dwconv1d_bwd(dud, xd, wd, s, want_db=False)
    assert a[2] is None and torch.equal(a[0], dx) and torch.equal(a[1], dw)


def test_kernels_are_graph_capturable(ops):
    shape = (2, 37, 72, 3, 1)
    xd, wd, bd, dud = _dev(*_random_inputs(*shape, seed=6))
    want = (ops.dwconv1d_fwd(xd, wd, bd, 1), *ops.dwconv1d_bwd(dud, xd, wd, 1))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = (ops.dwconv1d_fwd(xd, wd, bd, 1), *ops.dwconv1d_bwd(dud, xd, wd, 1))
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(want, got))


# ---- 4. F.token_aggregator and the module against the fixture ----------------------------------------------------------------
def _cos_norm(g, r):
    g, r = g.double().flatten().cpu(), r.double().flatten()
    return float(torch.dot(g, r) / (g.norm() * r.norm() + 1e-30)), float(g.norm() / (r.norm() + 1e-30))


def _module_from(sd, D, k):
    from sfcvit.models import TokenAggregator
    mod = TokenAggregator(D, k)
    mod.load_state_dict(sd)
    return mod.to("cuda", dtype=BF16)


@pytest.mark.parametrize("idx", [0, 1])
def test_function_and_module_match_the_fixture(idx):
    """Block-level bf16 against the reference's fp32 (tests/test_parity_gpu.py's stated tolerances): output within
    1e-2 max |ref|, every gradient cosine >= 0.99 and norm within 5 %."""
    import sfcvit.functional as F
    case = load_fixture()["cases"][idx]
    B, N, D, k = case["B"], case["N"], case["D"], case["k"]
    x, cot, sd = case_inputs(B, N, D, k)
    y_ref = torch.tensor(case["y"]).view(B, N, D)
    mod = _module_from(sd, D, k)
    xd = x.cuda().to(BF16).requires_grad_(True)
    y = mod(xd)
    (y.float() * cot.cuda()).sum().backward()
    err = float((y.float().cpu() - y_ref).abs().max() / y_ref.abs().max())
    figures = {"y": err, "dx": _cos_norm(xd.grad, torch.tensor(case["dx"]))}
    for key, p in mod.named_parameters():
        figures[key] = _cos_norm(p.grad, torch.tensor(case["grads"][key]))
    print(figures)
    assert err <= 1e-2
    for key, (cos, ratio) in ((k2, v) for k2, v in figures.items() if k2 != "y"):
        assert cos >= 0.99 and abs(ratio - 1) <= 5e-2, (key, cos, ratio)
    # the functional form on fp32 parameters (cast on entry) computes the same thing
    ps = {k2: v.cuda().requires_grad_(True) for k2, v in sd.items()}
    y2 = F.token_aggregator(xd.detach(), ps["dw.weight"], ps["dw.bias"], ps["pw.weight"], ps["pw.bias"], ps["norm.weight"],
                            ps["norm.bias"])
    assert torch.equal(y2, y)
    y2.float().sum().backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in ps.values())
    # F.dwconv1d alone, against fp64 on the bf16-rounded inputs (loose form of the kernel tests: the autograd plumbing)
    xb, wb, bb = x.to(BF16), sd["dw.weight"].to(BF16), sd["dw.bias"].to(BF16)
    xq = xb.cuda().requires_grad_(True)
    wq, bq = wb.cuda().requires_grad_(True), bb.cuda().requires_grad_(True)
    u = F.dwconv1d(xq, wq, bq)
    (u.float() * cot.cuda()).sum().backward()
    ref = dwconv_grads_ref(xb.float(), wb.float().view(D, k), bb.float(), cot.to(BF16).float(), 1)
    for got, want in ((u, ref[0]), (xq.grad, ref[1]), (wq.grad.view(D, k), ref[2]), (bq.grad, ref[3])):
        cos, ratio = _cos_norm(got.detach(), want)
        assert cos >= 0.999 and abs(ratio - 1) <= 2e-2, (cos, ratio)


def test_gradient_slots_hold_what_plain_autograd_returns():
    """Gradients written straight into FusedAdamW's flat buffer (FlatGradBuffer slots) equal those returned as tensors."""
    from sfcvit.training import FusedAdamW
    B, N, D, k = 2, 12, 24, 5
    x, cot, sd = case_inputs(B, N, D, k)
    xd, cd = x.cuda().to(BF16), cot.cuda()
    plain = _module_from(sd, D, k)
    (plain(xd).float() * cd).sum().backward()
    slotted = _module_from(sd, D, k)
    opt = FusedAdamW(slotted.parameters(), lr=0.0, weight_decay=0.0)
    (slotted(xd).float() * cd).sum().backward()
    opt.step()                                                   # lays the flat buffers out; lr 0: the weights stay
    opt.zero_grad()
    (slotted(xd).float() * cd).sum().backward()
    torch.cuda.synchronize()
    for (key, p), (_, q) in zip(plain.named_parameters(), slotted.named_parameters()):
        assert hasattr(q, "_sfcvit_slot"), key
        assert q.grad.data_ptr() == opt.flat_grad.data_ptr() + 2 * q._sfcvit_slot[1], key     # the slot itself, not a copy
        assert torch.equal(p.grad, q.grad), key


# ---- 5. model level --------------------------------------------------------------------------------------------------------
def _tiny_model(option=True, seed=11, dropout=0.0):
    from sfcvit.models import VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    cfg, batch = MODEL_CASES["hilbert32_1d"]
    torch.manual_seed(seed)
    pe = HilbertEmbedding1D(cfg.img_size, cfg.patch_size, cfg.in_channels, cfg.embed_dim)
    model = VisionTransformer1D(pe, depth=cfg.depth, n_heads=cfg.n_heads, mlp_dim=cfg.mlp_dim, num_classes=cfg.num_classes,
                                dropout_p=dropout, head_dropout_p=dropout, token_aggregator=option)
    x = formula.image_batch(batch, 3, cfg.img_size, cfg.img_size).cuda()
    tgt = formula.soft_targets(batch, cfg.num_classes).cuda()
    return model.to("cuda", dtype=BF16), x, tgt


def test_model_with_the_aggregator_trains():
    import sfcvit.functional as F
    from sfcvit.training import FusedAdamW, train_step
    model, x, tgt = _tiny_model()
    model.train()
    loss = F.soft_target_cross_entropy(model(x), tgt)
    loss.backward()
    for key, p in model.named_parameters():
        if key.startswith("ta."):
            assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()) and float(p.grad.float().abs().max()) > 0, key
    assert sum(k.startswith("ta.") for k, _ in model.named_parameters()) == 6
    model.zero_grad()
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    losses = [float(train_step(model, x, tgt, opt)) for _ in range(3)]       # the third call measures the loss after two steps
    print(losses)
    assert all(v == v for v in losses) and losses[2] < losses[0], losses


def test_default_models_are_untouched_by_the_option():
    a, x, _ = _tiny_model(option=False, seed=5)
    b, _, _ = _tiny_model(option=False, seed=5)
    on, _, _ = _tiny_model(option=True, seed=5)
    sa, sb, son = a.state_dict(), b.state_dict(), on.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert sorted(set(son) - set(sa)) == sorted("ta." + k for k in ("dw.weight", "dw.bias", "pw.weight", "pw.bias", "norm.weight", "norm.bias"))
    assert all(torch.equal(son[k], sa[k]) for k in sa)
    with torch.no_grad():
        ya, yb, yon = a.eval()(x), b.eval()(x), on.eval()(x)
    assert torch.equal(ya, yb)                                   # same seed, same bits
    assert not torch.equal(ya, yon)                              # the aggregator is in the path when asked for


def test_torch_compile_traces_the_model_with_the_aggregator_into_one_graph():
    import sfcvit.library  # noqa: F401  (registers the ops)
    model, x, _ = _tiny_model()
    model.eval()
    assert hasattr(torch.ops.sfcvit, "token_aggregator") and hasattr(torch.ops.sfcvit, "token_aggregator_bwd")
    with torch.no_grad():
        want = model(x)
    try:
        ex = torch._dynamo.explain(model)(x)
        assert ex.graph_break_count == 0 and ex.graph_count == 1, (ex.graph_break_count, ex.graph_count, ex.break_reasons)
        torch._dynamo.reset()
        compiled = torch.compile(model)
        with torch.no_grad():
            got = compiled(x)
        assert torch.equal(got, want)
        # backward through the traced ops: the eager gradients (same kernels, fresh tensors)
        model.train()
        model.zero_grad()
        model(x).float().sum().backward()
        eager = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        model.zero_grad()
        compiled(x).float().sum().backward()
        for k, p in model.named_parameters():
            if k.startswith("ta."):
                assert torch.equal(p.grad, eager[k]), k
    finally:
        torch._dynamo.reset()


def test_graphed_train_step_takes_the_eager_steps():
    """As tests/test_parity_gpu.py's graph test: the captured step gives the eager device-state step's loss bit for bit."""
    from sfcvit import ops
    from sfcvit.training import FusedAdamW, GraphedTrainStep, train_step
    try:
        model_e, x, tgt = _tiny_model(dropout=0.1)
        model_e.train()
        opt_e = FusedAdamW(model_e.parameters(), lr=1e-3, weight_decay=5e-2)
        opt_e.use_device_state(seed_base=4242)
        eager = [float(train_step(model_e, x, tgt, opt_e)) for _ in range(4)]
        model_g, _, _ = _tiny_model(dropout=0.1)
        model_g.train()
        opt_g = FusedAdamW(model_g.parameters(), lr=1e-3, weight_decay=5e-2)
        opt_g.use_device_state(seed_base=4242)
        step = GraphedTrainStep(model_g, x.clone(), tgt.clone(), opt_g, warmup=2, preserve_state=False)
        graphed = [float(step()) for _ in range(2)]
        print(eager, graphed)
        assert graphed == eager[2:], (graphed, eager)
        for (k, a), (_, b) in zip(model_e.state_dict().items(), model_g.state_dict().items()):
            assert torch.equal(a, b), k
        step.close()
    finally:
        ops.STEP_STATE = None


# ---- 6. main.py ------------------------------------------------------------------------------------------------------------
def test_main_py_trains_and_resumes_with_the_aggregator(tmp_path):
    main = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd", "main.py")
    base = [sys.executable, main, "--synthetic", "--tokenizer", "hilbert", "--img-size", "32", "--patch-size", "16", "--embed-dim", "64",
            "--depth", "1", "--heads", "1", "--mlp-dim", "128", "--batch-size", "64", "--train-size", "256", "--test-size", "128",
            "--warmup-epochs", "0", "--token-aggregator", "--checkpoint-dir", str(tmp_path)]
    out = subprocess.run(base + ["--epochs", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    ckpt = os.path.join(str(tmp_path), "checkpoint_hilbert.pt")
    sd = torch.load(ckpt, map_location="cpu", weights_only=True)["model_state_dict"]
    assert "ta.dw.weight" in sd and list(sd["ta.dw.weight"].shape) == [64, 1, 3]
    out = subprocess.run(base + ["--epochs", "2", "--resume", ckpt], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "Epoch 2/2" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]
