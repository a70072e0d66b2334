"""Streaming attention for head dims 128 / 192 / 256 at any sequence length (csrc/attention_wide_stream.hip), reached
through ops.attention_fwd / _bwd(..., any_length=True), the encoder layer and the reference's default model at 64 px."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SWITCH = "SFCVIT_ATTN_WIDE_STREAM"


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


@pytest.fixture(autouse=True)
def default_switch(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)


def bf(t):
    return t.to(torch.bfloat16)


def close(got, ref, rel=1.0 / 128, abs_scale=1.0 / 64):
    got, ref = got.float(), ref.float()
    tol = rel * ref.abs() + abs_scale * ref.pow(2).mean().sqrt().clamp_min(1e-6)
    bad = (got - ref).abs() > tol
    assert not bad.any(), f"{int(bad.sum())}/{bad.numel()} off, max err {float((got - ref).abs().max())}, ref rms {float(ref.pow(2).mean().sqrt())}"


def attn_ref(qkv, H, mask=None):
    """fp32 attention of a packed projection (mask: dropout keep factors [B, H, N, N]) -> out, lse."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    q, k, v = qkv.float().split(D, dim=-1)
    sp = lambda t: t.reshape(B, N, H, hd).transpose(1, 2)         # noqa: E731
    s = (sp(q) @ sp(k).transpose(-1, -2)) / math.sqrt(hd)
    p = torch.softmax(s, -1)
    if mask is not None:
        p = p * mask
    return (p @ sp(v)).transpose(1, 2).reshape(B, N, D), torch.logsumexp(s, -1)


def inputs(B, N, H, hd, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return bf(torch.randn(B, N, 3 * H * hd, device="cuda", generator=g)), bf(torch.randn(B, N, H * hd, device="cuda", generator=g))


def run(ops, qkv, dout, H, **kw):
    """forward + backward; -> out, lse, dqkv, (forward kernel, backward kernel)"""
    out, lse = ops.attention_fwd(qkv, H, **kw)
    kf = ops.last_attn_kernel()
    dqkv = ops.attention_bwd(qkv, out, lse, dout, H, **kw)
    return out, lse, dqkv, (kf, ops.last_attn_kernel())


def stream_names(hd):
    return (f"attn_wide_stream_fwd_kernel<{hd // 64}>", f"attn_wide_stream_bwd_kv_kernel<{hd // 64}>")


@pytest.mark.parametrize("B,N,H,hd", [(2, 576, 2, 128), (2, 256, 4, 192), (1, 300, 2, 256), (2, 1030, 1, 128),
                                      (3, 257, 1, 192), (1, 3136, 4, 192)])
def test_streaming_attention_against_fp32(ops, B, N, H, hd):
    """Shapes the whole-sequence kernels refuse (ragged last blocks at 1030 and 257; 3136 = the reference model at 224 px):
    out, lse and dqkv with the bars of test_attention_wide_heads, bit-identical from run to run."""
    qkv, dout = inputs(B, N, H, hd, 15)
    out, lse, dqkv, names = run(ops, qkv, dout, H, any_length=True)
    assert names == stream_names(hd)
    qf = qkv.float().requires_grad_(True)
    ref, lse_ref = attn_ref(qf, H)
    ref.backward(dout.float())
    close(out, ref.detach())
    assert torch.allclose(lse, lse_ref.detach(), atol=2e-2, rtol=1e-2)
    close(dqkv, qf.grad, rel=1.0 / 64, abs_scale=1.0 / 32)
    o2, l2, d2, _ = run(ops, qkv, dout, H, any_length=True)
    assert torch.equal(o2, out) and torch.equal(l2, lse) and torch.equal(d2, dqkv)
    with pytest.raises(Exception, match="LDS"):                 # the default entry point keeps its contract
        ops.attention_fwd(qkv, H)


def test_streaming_attention_dropout_matches_the_mask_function(ops):
    B, N, H, hd, p, seed = 2, 256, 4, 192, 0.1, 99
    qkv, dout = inputs(B, N, H, hd, 16)
    mask = ops.dropout_mask(B * H * N, N, p, seed).float().view(B, H, N, N)
    qf = qkv.float().requires_grad_(True)
    ref, _ = attn_ref(qf, H, mask)
    ref.backward(dout.float())
    out, lse, dqkv, names = run(ops, qkv, dout, H, dropout_p=p, dropout_seed=seed, any_length=True)
    assert names == stream_names(hd)
    close(out, ref.detach())
    close(dqkv, qf.grad, rel=1 / 48, abs_scale=1 / 24)
    assert torch.equal(run(ops, qkv, dout, H, dropout_p=p, dropout_seed=seed, any_length=True)[2], dqkv)


def test_streaming_backward_column_sums_are_those_of_its_dqkv(ops):
    """The in_proj bias gradient on the STREAM path (the column-sum pass over dqkv)."""
    B, N, H, hd = 2, 300, 2, 128
    qkv, dout = inputs(B, N, H, hd, 17)
    out, lse = ops.attention_fwd(qkv, H, any_length=True)
    dqkv, cs = ops.attention_bwd(qkv, out, lse, dout, H, colsum=True, any_length=True)
    assert ops.last_attn_kernel() == stream_names(hd)[1]
    x = dqkv.float().view(B * N, -1)
    assert (cs - x.sum(0)).abs().max() <= 1e-4 * x.abs().sum(0).max()
    assert torch.equal(dqkv, ops.attention_bwd(qkv, out, lse, dout, H, any_length=True))
    cb = torch.empty(3 * H * hd, device="cuda", dtype=torch.bfloat16)
    ops.attention_bwd(qkv, out, lse, dout, H, colsum=cb, any_length=True)
    assert torch.equal(cb, cs.to(torch.bfloat16))


@pytest.mark.parametrize("N,hd", [(1, 128), (5, 128), (64, 128), (196, 128), (1, 192), (5, 192), (64, 192), (1, 256),
                                  (64, 256)])
def test_forced_streaming_agrees_with_the_whole_sequence_kernels(ops, monkeypatch, N, hd):
    B, H = 2, 2
    qkv, dout = inputs(B, N, H, hd, 18)
    for p in (0.0, 0.1):
        kw = dict(dropout_p=p, dropout_seed=7, any_length=True)
        wide = run(ops, qkv, dout, H, **kw)
        assert wide[3] == (f"attn_wide_fwd_kernel<{hd // 64}>", f"attn_wide_bwd_kv_kernel<{hd // 64}>")
        monkeypatch.setenv(SWITCH, "1")
        got = run(ops, qkv, dout, H, **kw)
        monkeypatch.delenv(SWITCH)
        assert got[3] == stream_names(hd)
        close(got[0], wide[0])
        assert torch.allclose(got[1], wide[1], atol=2e-2, rtol=1e-2)
        close(got[2], wide[2], rel=1.0 / 64, abs_scale=1.0 / 32)
    qf = qkv.float().requires_grad_(True)
    ref, lse_ref = attn_ref(qf, H)
    ref.backward(dout.float())
    monkeypatch.setenv(SWITCH, "1")
    out, lse, dqkv, _ = run(ops, qkv, dout, H, any_length=True)
    close(out, ref.detach())
    assert torch.allclose(lse, lse_ref.detach(), atol=2e-2, rtol=1e-2)
    close(dqkv, qf.grad, rel=1.0 / 64, abs_scale=1.0 / 32)


@pytest.mark.parametrize("B,N,H,hd", [(2, 196, 2, 128), (2, 64, 4, 192), (4, 196, 12, 64), (2, 576, 16, 64)])
def test_any_length_changes_nothing_where_todays_kernels_run(ops, B, N, H, hd):
    qkv, dout = inputs(B, N, H, hd, 19)
    for p in (0.0, 0.1):
        a = run(ops, qkv, dout, H, dropout_p=p, dropout_seed=3)
        b = run(ops, qkv, dout, H, dropout_p=p, dropout_seed=3, any_length=True)
        assert a[3] == b[3] and "stream" not in a[3][0]
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x, y)


def _layer_params(D, Fd, gen):
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)    # noqa: E731
    w = {"self_attn.in_proj_weight": r(3 * D, D) / math.sqrt(D), "self_attn.in_proj_bias": r(3 * D) * 0.1,
         "self_attn.out_proj.weight": r(D, D) / math.sqrt(D), "self_attn.out_proj.bias": r(D) * 0.1,
         "norm1.weight": 1 + 0.1 * r(D), "norm1.bias": 0.1 * r(D),
         "linear1.weight": r(Fd, D) / math.sqrt(D), "linear1.bias": r(Fd) * 0.1,
         "linear2.weight": r(D, Fd) / math.sqrt(Fd), "linear2.bias": r(D) * 0.1,
         "norm2.weight": 1 + 0.1 * r(D), "norm2.bias": 0.1 * r(D)}
    return {k: v.bfloat16().float() for k, v in w.items()}


@pytest.mark.parametrize("D,H,N", [(256, 2, 576), (192, 2, 300), (768, 4, 256)])
def test_encoder_layer_against_the_oracle(ops, D, H, N):
    """functional.encoder_layer in eval mode against oracle.vit_oracle.encoder_layer in fp32 (hd 128, 96 padded to 128,
    192), output and the input / parameter gradients, with the bars of the encoder-layer tests in test_kernels_gpu.py."""
    from oracle import vit_oracle
    from sfcvit import functional as F
    B, Fd = 2, 512
    gen = torch.Generator(device="cuda").manual_seed(21)
    w = _layer_params(D, Fd, gen)
    names = list(w)
    x = bf(torch.randn(B, N, D, device="cuda", generator=gen)).float()
    r = torch.randn(B, N, D, device="cuda", generator=gen)
    ref_w = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    xr = x.clone().requires_grad_(True)
    yr = vit_oracle.encoder_layer(xr, ref_w, "", H)
    (yr * r).sum().backward()
    mine = [w[k].clone().requires_grad_(True) for k in names]
    xm = x.clone().requires_grad_(True)
    ops.KERNEL_LOG = []                          # (backward runs on autograd's thread: the log, not last_attn_kernel)
    try:
        y = F.encoder_layer(xm, *mine, H)
        (y.float() * r).sum().backward()
    finally:
        ran, ops.KERNEL_LOG = ops.KERNEL_LOG, None
    assert set(stream_names(128 if D // H <= 128 else D // H)) <= set(ran), ran
    close(y, yr.detach(), rel=1 / 64, abs_scale=1 / 32)
    for n, t, tr in [("x", xm, xr)] + [(n, t, ref_w[n]) for n, t in zip(names, mine)]:
        g, gr = t.grad.flatten().float(), tr.grad.flatten()
        cos = float(torch.dot(g, gr) / (g.norm() * gr.norm() + 1e-30))
        assert cos >= 0.995, (n, cos)
        assert abs(float(g.norm() / gr.norm()) - 1) <= 3e-2, n


def test_reference_default_model_trains_at_64_px():
    """main.py:269-282's model with the reference's own 4 heads (head dim 192) at TinyImageNet's 64 px: N = 256, where
    the whole-sequence kernels would need 192 KiB of LDS.  Three reference-style epochs on synthetic batches lower the
    loss and keep everything finite."""
    from src.models.vit import VisionTransformer1D
    from src.tokenizers.multiscale.multi_morton import HierarchicalMortonEmbedding
    from src.training.train import evaluate, train_with_mixup_or_cutmix
    from sfcvit import ops
    from sfcvit.training import FusedAdamW, SoftTargetCrossEntropy
    torch.manual_seed(42)
    np.random.seed(42)
    pe = HierarchicalMortonEmbedding(64, 3, [16, 4, 1], 256)
    model = VisionTransformer1D(pe, depth=8, n_heads=4, mlp_dim=512, num_classes=10).to("cuda", dtype=torch.bfloat16)
    opt = FusedAdamW(model.parameters(), lr=3e-4, weight_decay=5e-5)
    g = torch.Generator().manual_seed(0)
    xs = torch.randn(3, 32, 3, 64, 64, generator=g)
    ys = torch.randint(0, 10, (3, 32), generator=g)

    class Loader(list):
        dataset = range(96)
    loader = Loader(zip(xs, ys))
    crit = SoftTargetCrossEntropy()
    ops.KERNEL_LOG = []
    try:
        losses = [train_with_mixup_or_cutmix(model, loader, crit, opt, None, "cuda")[0] for _ in range(3)]
    finally:
        ran, ops.KERNEL_LOG = ops.KERNEL_LOG, None
    assert set(stream_names(192)) <= set(ran), sorted(set(ran))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    loss, acc = evaluate(model, loader, torch.nn.CrossEntropyLoss(), "cuda")
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0
