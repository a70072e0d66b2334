"""Attention maps (sfcvit_attention_probs) and attention-distance statistics (sfcvit_attention_stats) on the GPU, and
sfcvit.analysis.attention_report on whole models.

Reference: this file's own fp64 torch softmax of the SAME bf16 qkv on the CPU.  Error figures, one definition for every test:
    map        max over rows of  max_j |P - P_ref| / max_j P_ref           (relative to the row's largest probability)
    mass       |sum_j P - 1|
    distance   |d - d_ref| / the largest distance between two tokens       (sequence_distance: / (N - 1), entropy: / ln N;
               denominators at least 1)
Bounds: TOL_F32 is 4 x the worst figure measured over tests 1-3 on an MI355X (the margin is for other input
draws, not for kernel changes) and must stay <= 1e-3: a dropped or doubled key moves a row by ~1 / N of its mass, far above.
bf16 maps add one round-to-nearest-even step, 2^-8 of the value.  Every test prints its figure before asserting."""
import functools
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from oracle import formula, vit_oracle
from oracle.cases import MODEL_CASES
from test_host_cpu import build_model

pytestmark = pytest.mark.gpu

# worst figure of tests 1-3 measured on an MI355X: 2.45e-6 (random inputs, map, B 1 N 200 H 3 hd 256; uniform <= 1.9e-6 (mass,
# N = 577), one-hot <= 3.9e-8); profiles/probe/accuracy_figures.txt
TOL_F32 = 4 * 2.45e-6
TOL_BF16 = TOL_F32 + 2.0 ** -8      # bf16 keeps 8 significand bits: round-to-nearest-even moves a value by <= 2^-8 of itself
# attention_report (bf16 model path) against fp32 math on the same weights: worst measured 1.23e-3 (entropy, golden model)
TOL_MODEL = 4 * 1.23e-3
assert TOL_F32 <= 1e-3

# (B, N, H, hd): every N at hd 64, {65, 200} at the wider heads, N = 577 at hd 64, N = 130 at hd 256
SHAPES = [(1, 1, 1, 64), (2, 4, 3, 64), (1, 63, 3, 64), (2, 65, 1, 64), (1, 196, 3, 64), (2, 200, 1, 64),
          (1, 65, 3, 128), (2, 200, 1, 128), (2, 65, 1, 192), (1, 200, 3, 192), (1, 65, 1, 256), (1, 200, 3, 256),
          (1, 577, 1, 64), (1, 130, 3, 256)]
IDS = ["B%d-N%d-H%d-hd%d" % s for s in SHAPES]
GAP = 30.0


def positions(N):
    """Token centres of 16 x 16 patches on a grid ceil(sqrt(N)) wide, raster order."""
    w = math.isqrt(N - 1) + 1
    i = torch.arange(N)
    return torch.stack(((i // w) * 16 + 7.5, (i % w) * 16 + 7.5), dim=1).to(torch.float32)


def shift_of(N, b, h):
    """pi(i) = (i + shift) mod N: never the identity and never its own inverse for N > 2."""
    if N == 1:
        return 0
    s = (max(1, N // 3) + b + h) % N
    while s == 0 or (N > 2 and 2 * s % N == 0):
        s = (s + 1) % N
    return s


@functools.lru_cache(maxsize=None)
def make_qkv(kind, shape):
    """bf16 [B, N, 3 * H * hd] on the CPU.  uniform: q = 0; onehot: k_j = a +-1 code, q_i = alpha * code of pi(i), alpha a
    power of two chosen from the codes' smallest Hamming distance; random: N(0, 1), q scaled by 2 for peaked rows."""
    B, N, H, hd = shape
    g = torch.Generator().manual_seed(1000 * N + 10 * hd + H + B)
    qkv = torch.randn(B, N, 3, H, hd, generator=g)
    if kind == "uniform":
        qkv[:, :, 0] = 0
    elif kind == "onehot":
        codes = torch.randint(0, 2, (B, N, H, hd), generator=g).float() * 2 - 1
        alpha = torch.ones(B, H)
        for b in range(B):
            for h in range(H):
                c = codes[b, :, h]
                gram = c @ c.T
                gram.fill_diagonal_(-hd)
                worst = float(gram.max()) if N > 1 else -hd          # largest dot product of two different codes
                assert worst < hd, "codes are not distinct"
                alpha[b, h] = 2.0 ** math.ceil(math.log2(GAP * math.sqrt(hd) / (hd - worst)))
                qkv[b, :, 0, h] = alpha[b, h] * torch.roll(c, -shift_of(N, b, h), 0)
        qkv[:, :, 1] = codes
    else:
        qkv[:, :, 0] *= 2
    return qkv.reshape(B, N, 3 * H * hd).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def reference(kind, shape):
    """fp64 softmax of the bf16 qkv: P [B, H, N, N], and the four statistics [B, H, N]."""
    B, N, H, hd = shape
    t = make_qkv(kind, shape).double().reshape(B, N, 3, H, hd)
    q, k = t[:, :, 0].transpose(1, 2), t[:, :, 1].transpose(1, 2)
    s = (q @ k.transpose(2, 3)) / math.sqrt(hd)
    P = torch.softmax(s, dim=-1)
    pos = positions(N).double()
    dmat = (pos[:, None] - pos[None]).norm(dim=-1)
    idx = torch.arange(N, dtype=torch.float64)
    ent = -(P * torch.log(P.clamp_min(1e-300))).sum(-1)
    return {"P": P, "distance": (P * dmat).sum(-1),
            "sequence_distance": (P * (idx[:, None] - idx[None]).abs()).sum(-1), "entropy": ent,
            "scales": {"distance": max(float(dmat.max()), 1.0), "sequence_distance": max(N - 1.0, 1.0),
                       "entropy": max(math.log(N), 1.0)}, "s": s}


@functools.lru_cache(maxsize=None)
def run_gpu(kind, shape):
    """qkv, lse of the forward kernel, fp32 per-head map and the statistics, all on the device (computed once per case)."""
    from sfcvit import ops
    B, N, H, hd = shape
    qkv = make_qkv(kind, shape).cuda()
    _, lse = ops.attention_fwd(qkv, H, any_length=True)
    pos = positions(N).cuda()
    return {"qkv": qkv, "lse": lse, "pos": pos, "P": ops.attention_probs(qkv, lse, H),
            "stats": ops.attention_stats(qkv, lse, H, pos=pos)}


def map_err(got, ref):
    return float(((got.double().cpu() - ref).abs().amax(-1) / ref.amax(-1)).max())


def check_against(kind, shape, ref, tag):
    got = run_gpu(kind, shape)
    fig = {"map": map_err(got["P"], ref["P"]), "mass": float((got["stats"]["mass"].double().cpu() - 1).abs().max())}
    for name in ("distance", "sequence_distance", "entropy"):
        fig[name] = float((got["stats"][name].double().cpu() - ref[name]).abs().max()) / ref["scales"][name]
    print(f"FIGURE {tag} {shape}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    assert max(fig.values()) <= TOL_F32, fig
    return fig


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_uniform_scores(shape):
    """q = 0: P = 1 / N, entropy = ln N, distance = plain mean distance from token i, sequence distance = sum_j |i - j| / N."""
    B, N, H, hd = shape
    pos = positions(N).double()
    dmat = (pos[:, None] - pos[None]).norm(dim=-1)
    idx = torch.arange(N, dtype=torch.float64)
    ref = dict(reference("uniform", shape))
    assert float((ref["P"] - 1.0 / N).abs().max()) < 1e-15
    ones = torch.ones(B, H, N, dtype=torch.float64)
    ref.update(distance=ones * dmat.mean(1), sequence_distance=ones * (idx[:, None] - idx[None]).abs().mean(1),
               entropy=ones * math.log(N))
    check_against("uniform", shape, ref, "uniform")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_hot_rows(shape):
    """Every row's largest scaled score beats the others by >= 30 at pi(i) = i + shift: the map is that permutation matrix."""
    B, N, H, hd = shape
    exact = reference("onehot", shape)
    pos = positions(N).double()
    ref = {"P": torch.zeros(B, H, N, N, dtype=torch.float64), "scales": exact["scales"], "entropy": torch.zeros(B, H, N, dtype=torch.float64),
           "distance": torch.zeros(B, H, N, dtype=torch.float64), "sequence_distance": torch.zeros(B, H, N, dtype=torch.float64)}
    i = torch.arange(N)
    for b in range(B):
        for h in range(H):
            pi = (i + shift_of(N, b, h)) % N
            s = exact["s"][b, h]
            if N > 1:                                            # the construction has its gap at this shape (checked on the CPU)
                assert N < 3 or not torch.equal(pi[pi], i)
                rest = s.clone()
                rest[i, pi] = -math.inf
                assert float((s[i, pi] - rest.amax(-1)).min()) >= GAP
            ref["P"][b, h, i, pi] = 1.0
            ref["distance"][b, h] = (pos - pos[pi]).norm(dim=-1)
            ref["sequence_distance"][b, h] = (i - pi).abs().double()
    assert float((exact["P"] - ref["P"]).abs().max()) <= N * math.exp(-GAP)
    check_against("onehot", shape, ref, "onehot")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_inputs(shape):
    """fp32 and bf16 maps, per head and averaged over heads, and all four statistics against the fp64 reference."""
    from sfcvit import ops
    B, N, H, hd = shape
    ref = reference("random", shape)
    check_against("random", shape, ref, "random")
    got = run_gpu("random", shape)
    qkv, lse = got["qkv"], got["lse"]
    mean_ref = ref["P"].mean(1)
    figs = {"bf16": map_err(ops.attention_probs(qkv, lse, H, dtype=torch.bfloat16), ref["P"]),
            "mean_f32": map_err(ops.attention_probs(qkv, lse, H, head_mean=True), mean_ref),
            "mean_bf16": map_err(ops.attention_probs(qkv, lse, H, head_mean=True, dtype=torch.bfloat16), mean_ref)}
    print(f"FIGURE random-maps {shape}: " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()))
    assert figs["mean_f32"] <= TOL_F32 and figs["bf16"] <= TOL_BF16 and figs["mean_bf16"] <= TOL_BF16, figs
    # an explicit scale and skipped outputs: the same numbers
    st = ops.attention_stats(qkv, lse, H, scale=hd ** -0.5)
    assert set(st) == {"sequence_distance", "entropy", "mass"}
    assert all(torch.equal(st[k], got["stats"][k]) for k in st)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_sum_to_one_and_head_mean_is_the_mean_of_the_heads(shape):
    from sfcvit import ops
    B, N, H, hd = shape
    got = run_gpu("random", shape)
    P = got["P"]
    fig = float((P.double().sum(-1) - 1).abs().max())
    print(f"FIGURE rowsum {shape}: {fig:.3e}")
    assert tuple(P.shape) == (B, H, N, N) and fig <= TOL_F32
    pm = ops.attention_probs(got["qkv"], got["lse"], H, head_mean=True)
    acc = torch.zeros_like(P[:, 0])
    for h in range(H):                                           # the kernel's order: heads ascending, fp32 adds
        acc = acc + P[:, h]
    want = acc / H                                               # the kernel multiplies by fp32(1 / H): rounding of that step only
    assert tuple(pm.shape) == (B, N, N)
    assert torch.allclose(pm, want, rtol=3 * 2.0 ** -24, atol=1e-37), float((pm - want).abs().max())
    assert float((pm.double().sum(-1) - 1).abs().max()) <= TOL_F32


@pytest.mark.parametrize("shape", [(2, 200, 3, 64), (1, 130, 3, 256), (2, 65, 1, 192)], ids=lambda s: "B%d-N%d-H%d-hd%d" % s)
def test_two_runs_give_the_same_bits(shape):
    from sfcvit import ops
    B, N, H, hd = shape
    got = run_gpu("random", shape)
    qkv, lse, pos = got["qkv"], got["lse"], got["pos"]
    for kw in (dict(), dict(head_mean=True), dict(dtype=torch.bfloat16)):
        assert torch.equal(ops.attention_probs(qkv, lse, H, **kw), ops.attention_probs(qkv, lse, H, **kw)), kw
    assert torch.equal(ops.attention_probs(qkv, lse, H), got["P"])
    again = ops.attention_stats(qkv, lse, H, pos=pos)
    assert all(torch.equal(again[k], got["stats"][k]) for k in got["stats"])
    assert torch.equal(qkv.cpu(), make_qkv("random", shape))      # inputs are never written


GUARD = 256


def _guarded(shape, dtype):
    n = math.prod(shape)
    flat = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=dtype)
    return flat, flat[:n].view(shape)


@pytest.mark.parametrize("shape", [(2, 63, 3, 64), (1, 65, 3, 128), (2, 200, 1, 64), (1, 130, 3, 256), (1, 1, 1, 64)],
                         ids=lambda s: "B%d-N%d-H%d-hd%d" % s)
def test_nothing_is_written_past_the_outputs(shape):
    from sfcvit import ops
    B, N, H, hd = shape
    got = run_gpu("random", shape)
    qkv, lse, pos = got["qkv"], got["lse"], got["pos"]
    for dtype in (torch.float32, torch.bfloat16):
        for mean in (False, True):
            flat, out = _guarded((B, N, N) if mean else (B, H, N, N), dtype)
            ops.attention_probs(qkv, lse, H, head_mean=mean, dtype=dtype, out=out)
            assert bool(torch.isnan(flat[out.numel():]).all()) and bool(torch.isfinite(out).all()), (dtype, mean)
            if dtype == torch.float32 and not mean:
                assert torch.equal(out, got["P"])
    bufs = {k: _guarded((B, H, N), torch.float32) for k in ops.ATTENTION_STATS}
    ops.attention_stats(qkv, lse, H, pos=pos, out={k: v[1] for k, v in bufs.items()})
    for k, (flat, out) in bufs.items():
        assert bool(torch.isnan(flat[out.numel():]).all()) and torch.equal(out, got["stats"][k]), k


# ---- model level --------------------------------------------------------------------------------------------------------
def _golden_model():
    cfg, batch = MODEL_CASES["hilbert32_1d"]
    model = build_model(cfg)
    model.load_state_dict(vit_oracle.formula_state(cfg), strict=True)
    return model.to("cuda", dtype=torch.bfloat16), formula.image_batch(batch, cfg.in_channels, cfg.img_size, cfg.img_size).cuda()


def _padded_head_model():
    """D = 128, H = 4: head dim 32, run zero-padded on the head-dim-64 kernels; 64 tokens."""
    from sfcvit.models import VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    torch.manual_seed(7)
    model = VisionTransformer1D(HilbertEmbedding1D(32, 16, 3, 128), depth=2, n_heads=4, mlp_dim=256, num_classes=10)
    return model.to("cuda", dtype=torch.bfloat16), torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(8)).cuda()


def _fp32_layers(model, tokens, pos):
    """fp32 restatement of mixer + post-norm encoder layers on the model's own weights: per layer (distance, entropy) [B, H]."""
    ln = torch.nn.functional.layer_norm
    f = lambda t: t.detach().float().cpu()
    x = f(tokens)
    m = model.mlp_mixer
    x = x + torch.nn.functional.gelu(ln(x, x.shape[-1:], f(m.channel_mix_ln.weight), f(m.channel_mix_ln.bias)) @ f(m.channel_mix[0].weight).T
                                     + f(m.channel_mix[0].bias)) @ f(m.channel_mix[2].weight).T + f(m.channel_mix[2].bias)
    dmat = (pos[:, None] - pos[None]).norm(dim=-1)
    H, out = model.encoder.n_head, []
    for layer in model.encoder.transformer.layers:
        a = layer.self_attn
        B, N, D = x.shape
        qkv = (x @ f(a.in_proj_weight).T + f(a.in_proj_bias)).reshape(B, N, 3, H, D // H)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        P = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(D // H), dim=-1)
        out.append(((P * dmat).sum(-1).mean(-1), -(P * torch.log(P.clamp_min(1e-30))).sum(-1).mean(-1)))
        o = (P @ v).transpose(1, 2).reshape(B, N, D) @ f(a.out_proj.weight).T + f(a.out_proj.bias)
        x = ln(x + o, (D,), f(layer.norm1.weight), f(layer.norm1.bias))
        ff = torch.relu(x @ f(layer.linear1.weight).T + f(layer.linear1.bias)) @ f(layer.linear2.weight).T + f(layer.linear2.bias)
        x = ln(x + ff, (D,), f(layer.norm2.weight), f(layer.norm2.bias))
    return out


@pytest.mark.parametrize("which", ["golden_hilbert32_1d", "head_dim_32_padded"])
def test_attention_report_on_a_model(which):
    from sfcvit import ops
    from sfcvit.analysis import attention_report, token_positions
    model, x = _golden_model() if which.startswith("golden") else _padded_head_model()
    model.train()                                                # the report runs at dropout 0 whatever the mode says
    ops.KERNEL_LOG = log = []
    try:
        rep = attention_report(model, x, maps=True, head_mean=False, rows=True)
    finally:
        ops.KERNEL_LOG = None
    assert model.training and all(m.training for m in model.modules())
    with torch.no_grad():
        want = model.eval()(x)
    assert torch.equal(rep["logits"], want)
    B, N, H = x.shape[0], model.patch_embed.n_patches, model.encoder.n_head
    depth = len(model.encoder.transformer.layers)
    assert [e["layer"] for e in rep["layers"]] == list(range(depth))
    assert sum(k.startswith("attn_probe_stats_kernel<1>") for k in log) == depth
    assert sum(k.startswith("attn_probe_map_kernel<1, false>") for k in log) == depth
    pos = token_positions(model.patch_embed)
    assert torch.equal(rep["positions"].cpu(), pos)
    ref = _fp32_layers(model, model.patch_embed(x), pos)
    dscale, escale = float((pos[:, None] - pos[None]).norm(dim=-1).max()), max(math.log(N), 1.0)
    for e, (dref, eref) in zip(rep["layers"], ref):
        assert tuple(e["map"].shape) == (B, H, N, N) and tuple(e["distance"].shape) == (B, H)
        assert tuple(e["rows"]["entropy"].shape) == (B, H, N)
        assert float((e["map"].double().sum(-1) - 1).abs().max()) <= TOL_F32 and e["mass_error"] <= TOL_F32
        fd = float((e["distance"].cpu() - dref).abs().max()) / dscale
        fe = float((e["entropy"].cpu() - eref).abs().max()) / escale
        fs = float((e["sequence_distance"] - e["rows"]["sequence_distance"].mean(-1)).abs().max())
        print(f"FIGURE model {which} layer {e['layer']}: distance={fd:.3e} entropy={fe:.3e} mass={e['mass_error']:.3e}")
        assert fd <= TOL_MODEL and fe <= TOL_MODEL and fs == 0.0, (fd, fe, fs)
    only = attention_report(model, x, layers=[depth - 1])
    assert [e["layer"] for e in only["layers"]] == [depth - 1] and "map" not in only["layers"][0]
    assert torch.equal(only["logits"], want)
    assert torch.equal(only["layers"][0]["distance"], rep["layers"][-1]["distance"])


def test_attention_report_on_the_pooled_vits():
    """altvit's SimpleViT (head dim 32, padded on the activations) and HilbertViT: same logits, maps that sum to 1."""
    from sfcvit.analysis import attention_report
    from sfcvit.models.altvit import HilbertViT, SimpleViT
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(3)).cuda()
    for cls, dim_head in ((SimpleViT, 32), (HilbertViT, 64)):
        torch.manual_seed(5)
        model = cls(image_size=32, patch_size=8, num_classes=10, dim=64, depth=2, heads=2, mlp_dim=128, dim_head=dim_head)
        model = model.to("cuda", dtype=torch.bfloat16)
        rep = attention_report(model, x, maps=True)
        with torch.no_grad():
            assert torch.equal(rep["logits"], model(x))
        assert len(rep["layers"]) == 2 and tuple(rep["layers"][0]["map"].shape) == (2, 16, 16)
        assert all(e["mass_error"] <= TOL_F32 and tuple(e["entropy"].shape) == (2, 2) for e in rep["layers"])


def test_main_writes_the_attention_report(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "attention.json"
    cmd = [sys.executable, os.path.join(root, "space-filling-curves-for-vision-transformers_amd", "main.py"), "--synthetic",
           "--tokenizer", "hilbert", "--patch-size", "64", "--embed-dim", "128", "--depth", "3", "--heads", "2", "--mlp-dim", "256",
           "--batch-size", "8", "--train-size", "8", "--test-size", "8", "--epochs", "0", "--checkpoint-dir", str(tmp_path / "ck"),
           "--attention-report", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.loads(out.read_text())
    assert [e["layer"] for e in rep["layers"]] == [0, 1, 2] and rep["tokens"] == 16
    for e in rep["layers"]:
        assert len(e["distance"]) == len(e["sequence_distance"]) == len(e["entropy"]) == 2
        assert all(math.isfinite(v) and v >= 0 for v in e["distance"] + e["entropy"]) and e["mass_error"] <= TOL_F32
