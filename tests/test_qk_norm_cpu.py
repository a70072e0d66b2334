"""QK-norm without a GPU: the reference against torch's own LayerNorm + scaled_dot_product_attention, the state_dict surface
(`encoder.qk_norm.<l>`, no changed draw), the plans of the kernels through the library (geometry, workspace, every refusal
decided before any HIP call), the ABI surface, the sanitizer program, and the refusals of the constructors, F.* and main.py."""
import ctypes
import importlib.util
import math
import os
import re
import subprocess

import pytest
import torch

import drop_path_ref
import prenorm_ref
import qk_norm_ref
from oracle.cases import MODEL_CASES
from test_host_cpu import build_model
from token_pool_ref import build_with

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd")
EINVAL = 1
NEW_SYMBOLS = ("sfcvit_qk_norm_fwd", "sfcvit_qk_norm_bwd", "sfcvit_qk_norm_bwd_ws", "sfcvit_qk_norm_plan")
# (B, N, H, hd) of the GPU tests: M = B * N
SHAPES = [(2, 5, 4, 64), (2, 5, 3, 64), (2, 197, 12, 64), (2, 5, 4, 48), (2, 5, 4, 20), (1, 7, 2, 128), (1, 7, 2, 96), (1, 7, 1, 192),
          (1, 7, 1, 256)]


def _hp(hd):
    return next(s for s in (64, 128, 192, 256) if hd <= s)


def _layer_inputs(B, N, D, H, Fd, seed, pre):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc          # noqa: E731
    names = prenorm_ref.ORDER if pre else ["in_w", "in_b", "out_w", "out_b", "n1_w", "n1_b", "w1", "b1", "w2", "b2", "n2_w", "n2_b"]
    shapes = dict(in_w=(3 * D, D), in_b=(3 * D,), out_w=(D, D), out_b=(D,), w1=(Fd, D), b1=(Fd,), w2=(D, Fd), b2=(D,))
    P = {k: (r(*shapes[k], sc=0.2) if k in shapes else (1 + r(D, sc=0.1) if k.endswith("_w") else r(D, sc=0.1))) for k in names}
    qk = torch.stack([1 + r(D // H, sc=0.2), r(D // H, sc=0.2), 1 + r(D // H, sc=0.2), r(D // H, sc=0.2)])
    return r(B, N, D), P, qk


# ---- (a) the reference ---------------------------------------------------------------------------------------------------------
def test_reference_without_qk_norm_is_the_existing_references():
    B, N, D, H, Fd = 3, 9, 32, 4, 64
    x, P, _ = _layer_inputs(B, N, D, H, Fd, 3, pre=False)
    one = torch.ones(())
    ones = torch.ones(B)
    assert torch.equal(qk_norm_ref.encoder_layer(x, P, H, (one, one, one, one), ones, ones),
                       drop_path_ref.encoder_layer(x, P, H, (one, one, one, one), ones, ones))
    s, P, _ = _layer_inputs(B, N, D, H, Fd, 4, pre=True)
    n = torch.nn.functional.layer_norm(s, (D,))
    a, b = qk_norm_ref.pre_norm_layer(s, n, P, H, act="gelu"), prenorm_ref.pre_norm_layer(s, n, P, H, act="gelu")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("eps", [1e-6, 1e-5, 0.0])
def test_reference_equals_torch_layernorm_and_sdpa(eps):
    """fp32 on the CPU: nn.LayerNorm(hd) on [B, H, N, hd] followed by F.scaled_dot_product_attention, written independently."""
    from torch import nn
    B, N, D, H = 3, 9, 48, 4
    hd = D // H
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, N, 3 * D, generator=g) * 2 + 0.5
    qk = torch.stack([1 + 0.3 * torch.randn(hd, generator=g), 0.3 * torch.randn(hd, generator=g),
                      1 + 0.3 * torch.randn(hd, generator=g), 0.3 * torch.randn(hd, generator=g)])
    got, probs = qk_norm_ref.attention(qkv, H, qk, eps)
    qn, kn = nn.LayerNorm(hd, eps=eps), nn.LayerNorm(hd, eps=eps)
    with torch.no_grad():
        qn.weight.copy_(qk[0]); qn.bias.copy_(qk[1]); kn.weight.copy_(qk[2]); kn.bias.copy_(qk[3])
        q, k, v = (t.reshape(B, N, H, hd).permute(0, 2, 1, 3) for t in qkv.split(D, dim=-1))
        want = torch.nn.functional.scaled_dot_product_attention(qn(q), kn(k), v).permute(0, 2, 1, 3).reshape(B, N, D)
    err = float((got - want).abs().max())
    print(f"eps {eps}: max |qk_norm_ref - LayerNorm + sdpa| = {err:.2e}")
    assert err <= 1e-5 and float((probs.sum(-1) - 1).abs().max()) <= 1e-5
    # and inside both layers: the layer with parameters differs from the layer without exactly by that attention
    x, P, qkp = _layer_inputs(B, N, D, H, 64, 6, pre=False)
    one, ones = torch.ones(()), torch.ones(B)
    y0 = qk_norm_ref.encoder_layer(x, P, H, (one, one, one, one), ones, ones)
    y1 = qk_norm_ref.encoder_layer(x, P, H, (one, one, one, one), ones, ones, qk_norm=qkp, qk_eps=eps)
    assert float((y0 - y1).abs().max()) > 1e-3


def test_walsh_inputs_give_exact_answers_in_fp32():
    """The exact-answer claims of the GPU tests, on the CPU in fp32 with an rstd one ulp off either way: LN(x) = gamma * sign +
    beta and dx = 2^(m - k) * row survive the rounding to bf16 bit for bit."""
    BF16 = torch.bfloat16
    for hd in (64, 128, 256):
        x, gy, k, m, sx, sg, gamma, beta = qk_norm_ref.exact_inputs(12, 3, hd)
        assert torch.equal(x.to(BF16).float(), x) and bool((x.sum(-1) == 0).all()) and bool((gy.sum(-1) == 0).all())
        assert bool(((x * gy).sum(-1) == 0).all())
        want = (gamma * sx + beta).to(BF16)
        assert torch.equal(want.float(), gamma * sx + beta) and bool((want != 0).all())
        dy = gy / gamma
        assert torch.equal(dy.to(BF16).float(), dy)
        for eps in (0.0, 1e-6, 1e-5):
            var = (x * x).mean(-1, keepdim=True)
            for ulp in (-1, 0, 1):
                rstd = (var + eps).rsqrt()
                rstd = torch.nextafter(rstd, rstd * (2.0 if ulp > 0 else 0.5)) if ulp else rstd
                y = ((x * rstd) * gamma + beta).to(BF16)
                assert torch.equal(y, want), (hd, eps, ulp)
                xh = x * rstd
                c2 = (gy * xh).mean(-1, keepdim=True)
                dx = (rstd * (gy - xh * c2)).to(BF16)
                assert torch.equal(dx.float(), sg * torch.pow(2.0, (m - k).float())[..., None]), (hd, eps, ulp)


# ---- (b) the state_dict surface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["raster32_2d", "hilbert32_1d"])
def test_state_dict_surface(name):
    cfg, _ = MODEL_CASES[name]
    torch.manual_seed(7)
    base = build_model(cfg)
    torch.manual_seed(7)
    off = build_with(cfg, qk_norm=False)
    torch.manual_seed(7)
    on = build_with(cfg, qk_norm=True)
    torch.manual_seed(7)
    pre = build_with(cfg, qk_norm=True, qk_norm_eps=1e-5, norm_first=True, activation="gelu", layer_scale=1e-4)
    a, b, c, d = base.state_dict(), off.state_dict(), on.state_dict(), pre.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a) and not hasattr(off.encoder, "qk_norm")
    assert all(torch.equal(a[k], c[k]) and torch.equal(a[k], d[k]) for k in a)      # no draw: every other value as it was
    keys = [f"encoder.qk_norm.{l}" for l in range(cfg.depth)]
    assert set(c) - set(a) == set(keys), set(c) - set(a)
    assert {k for k in set(d) - set(a) if "qk_norm" in k} == set(keys)
    hd = cfg.embed_dim // cfg.n_heads
    want = torch.tensor([1.0, 0.0, 1.0, 0.0])[:, None].expand(4, hd)
    for k in keys:
        assert tuple(c[k].shape) == (4, hd) and torch.equal(c[k], want) and torch.equal(d[k], want), k
    assert isinstance(on.encoder.qk_norm, torch.nn.ParameterList) and on.encoder.qk_norm_eps == 1e-6 and pre.encoder.qk_norm_eps == 1e-5
    # the optimizer treats them as it treats the LayerNorm parameters: one group, a slot in the flat gradient buffer
    from sfcvit.training import FusedAdamW
    opt = FusedAdamW(on.parameters(), lr=1e-3)
    assert len(opt.param_groups) == 1
    ln = on.encoder.transformer.layers[0].norm1.weight
    for prm in on.encoder.qk_norm:
        assert any(prm is q for q in opt.params) and (getattr(prm, "_sfcvit_slot", None) is None) == (getattr(ln, "_sfcvit_slot", None) is None)


# ---- (c) the plans through the library -------------------------------------------------------------------------------------------
def _buffers():
    raw = ctypes.create_string_buffer(1 << 20)
    p = (ctypes.addressof(raw) + 15) // 16 * 16                # 16-byte aligned host addresses: never dereferenced
    return raw, p


@pytest.mark.parametrize("B,N,H,hd", SHAPES + [(256, 196, 12, 64), (64, 576, 16, 64)])
def test_plan_and_workspace(B, N, H, hd):
    from sfcvit import ops
    from sfcvit._lib import lib
    M, hp = B * N, _hp(hd)
    plan = ops.qk_norm_plan(M, H, hp)
    print((B, N, H, hd), plan)
    rows = plan["rows_per_wg"]
    assert plan["vpl"] == hp // 64 and plan["slot_groups"] == -(-2 * H // 8) and rows >= 1
    assert plan["blocks"] == plan["slot_groups"] * -(-M // rows)
    assert lib.sfcvit_qk_norm_bwd_ws(M, H, hp) == plan["blocks"] * 12 * hp * 4
    assert lib.sfcvit_qk_norm_bwd_ws(0, H, hp) == 0 and lib.sfcvit_qk_norm_bwd_ws(M, 0, hp) == 0 and lib.sfcvit_qk_norm_bwd_ws(M, H, 96) == 0
    out = (ctypes.c_int32 * 4)()
    assert lib.sfcvit_qk_norm_plan(M, H, 100, out) == EINVAL and lib.sfcvit_qk_norm_plan(M, H, hp, None) == EINVAL


def test_host_refusals_launch_nothing():
    """Every refusal is SFCVIT_EINVAL with a message, decided before any HIP call: without a GPU a launch attempt would come back
    as a launch error (status 2), not as status 1."""
    from sfcvit._lib import lib
    raw, p = _buffers()
    qkv, rw, P, dP, cs, vs, ws = (p + (i << 16) for i in range(7))         # [10, 3 * 4 * 64] bf16 = 15 360 bytes

    def fwd(qkv=qkv, raw=rw, params=P, M=10, H=4, hd=64, hp=64, eps=1e-6):
        return lib.sfcvit_qk_norm_fwd(qkv, raw, params, M, H, hd, hp, eps, None)

    def bwd(dqkv=qkv, raw=rw, params=P, dparams=dP, colsum=cs, vsum=vs, ws=ws, M=10, H=4, hd=64, hp=64, eps=1e-6):
        return lib.sfcvit_qk_norm_bwd(dqkv, raw, params, dparams, 0, colsum, 0, vsum, ws, M, H, hd, hp, eps, None)

    def refused(rc, word):
        msg = lib.sfcvit_last_error().decode()
        print(rc, msg)
        assert rc == EINVAL and word in msg, (rc, msg)

    for n in ("qkv", "raw", "params"):
        refused(fwd(**{n: None}), "null")
    for n in ("dqkv", "raw", "params", "dparams"):
        refused(bwd(**{n: None}), "null")
    refused(bwd(ws=None), "workspace")
    refused(bwd(colsum=None), "vsum without colsum")
    for n, addr in dict(qkv=qkv, raw=rw, params=P).items():
        refused(fwd(**{n: addr + 8}), "aligned")
    for n, addr in dict(dqkv=qkv, raw=rw, params=P, dparams=dP, colsum=cs, vsum=vs, ws=ws).items():
        refused(bwd(**{n: addr + 8}), "aligned")
    refused(fwd(raw=qkv + 1024), "overlaps")
    refused(bwd(raw=qkv + 1024), "overlaps")
    for f, what in ((fwd, "qk_norm_fwd"), (bwd, "qk_norm_bwd")):
        for hp in (0, 32, 96, 65, 512, -64):
            refused(f(hp=hp, hd=8), "not a kernel head dim")
        refused(f(hp=100, hd=8), what)
        for hd in (0, -1, 65, 1000):
            refused(f(hd=hd), f"hd={hd}")
        refused(f(hd=129, hp=128), "hd=129")
        for z in (0, -5):
            refused(f(M=z), f"M={z}")
            refused(f(H=z), f"H={z}")
        refused(f(H=11184811), "leaves int")                   # 3 * H * 64 = 2^31 + 64
        refused(f(H=2 ** 31 - 1, hp=256, hd=64), "leaves int")
        for eps in (-1e-6, float("nan"), float("inf"), -float("inf")):
            refused(f(eps=eps), "eps=")
    buf = ctypes.create_string_buffer(96)
    assert lib.sfcvit_last_rowwise_kernel(buf, 96) == 0 and b"qk_norm" not in buf.value      # nothing was launched


def test_abi_surface():
    """The header declares what _lib.py binds, with the argument counts of the declarations, and the version stays 1."""
    from sfcvit import _lib
    header = open(os.path.join(ROOT, "include", "sfcvit.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} is not declared in include/sfcvit.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define\s+SFCVIT_ABI_VERSION\s+1\b", header)
    assert _lib.lib.sfcvit_abi_version() == 1


def test_python_layers_refuse_cpu_tensors():
    from sfcvit import functional as F, ops
    from sfcvit._lib import SfcvitError
    z = torch.zeros(4, 3 * 2 * 64, dtype=torch.bfloat16)
    P = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        ops.qk_norm_fwd(z, P, 2, 64)
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        ops.qk_norm_bwd(z, z[:, :256].contiguous(), P, 2, 64)
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        F.qk_norm(z, 2, P)


# ---- (d) the sanitizer program ---------------------------------------------------------------------------------------------------
def test_sanitizer_program_drives_the_new_plans():
    """`make asan` builds and runs csrc/hostcheck/host_check.cpp with qk_norm.cpp compiled in under -fsanitize=address,undefined;
    check_qk_norm is part of it."""
    csrc = os.path.join(PKG, "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^ASAN_SRCS :=.*\bqk_norm\.cpp\b", mk, re.M)
    assert "check_qk_norm();" in open(os.path.join(csrc, "hostcheck", "host_check.cpp")).read()
    out = subprocess.run(["make", "-s", "-C", csrc, "asan"], capture_output=True, text=True, timeout=900)
    print(out.stdout[-500:], out.stderr[-2000:])
    assert out.returncode == 0 and "host_check ok" in out.stdout


# ---- (e) constructors, F.* and main.py -------------------------------------------------------------------------------------------
def test_constructor_and_functional_refusals():
    from sfcvit import functional as F
    from sfcvit.models import TransformerSeqEncoder, VisionTransformer, VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    for eps in (-1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="qk_norm_eps="):
            TransformerSeqEncoder(16, 4, 2, 32, None, qk_norm=True, qk_norm_eps=eps)
    with pytest.raises(ValueError, match="exceeds the largest supported"):
        TransformerSeqEncoder(1024, 4, 2, 32, None, qk_norm=True)
    enc = TransformerSeqEncoder(16, 4, 2, 32, None, n_layers=3, qk_norm=True, qk_norm_eps=0.0)
    assert len(enc.qk_norm) == 3 and tuple(enc.qk_norm[2].shape) == (4, 8) and enc.qk_norm_eps == 0.0
    assert not hasattr(TransformerSeqEncoder(16, 4, 2, 32, None), "qk_norm")
    for cls in (VisionTransformer, VisionTransformer1D):
        m = cls(HilbertEmbedding1D(32, 256, 3, 32), depth=2, n_heads=2, mlp_dim=32, norm_first=True, activation="gelu", layer_scale=0.1,
                drop_path_rate=0.1, pool="mean", pos_embed="learned", qk_norm=True)
        assert len(m.encoder.qk_norm) == 2 and tuple(m.encoder.qk_norm[0].shape) == (4, 16)
        m = cls(HilbertEmbedding1D(32, 256, 3, 32), depth=1, n_heads=2, mlp_dim=32, rel_pos_bias="curve", qk_norm=True)
        assert len(m.encoder.qk_norm) == 1 and len(m.encoder.rel_pos_bias) == 1
    D, H = 16, 2
    x = torch.zeros(1, 2, D)
    w = [torch.zeros(3 * D, D), torch.zeros(3 * D), torch.zeros(D, D)] + [torch.zeros(D)] * 3 + [torch.zeros(32, D), torch.zeros(32),
                                                                                                  torch.zeros(D, 32)] + [torch.zeros(D)] * 3
    for bad in (torch.zeros(4, D), torch.zeros(2, D // H), torch.zeros(4 * D // H), "yes"):
        with pytest.raises(ValueError, match="qk_norm must be a"):
            F.encoder_layer(x, *w, H, qk_norm=bad)
        with pytest.raises(ValueError, match="qk_norm must be a"):
            F.pre_norm_layer(x, x, *w, H, qk_norm=bad)
        with pytest.raises(ValueError, match="qk_norm must be a"):
            F.encoder_layer_probe(x, *w, H, qk_norm=bad)
        with pytest.raises(ValueError, match="qk_norm must be a"):
            F.pre_norm_layer_probe(x, x, *w, H, qk_norm=bad)
    for eps in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="qk_norm_eps="):
            F.encoder_layer(x, *w, H, qk_norm=torch.zeros(4, D // H), qk_norm_eps=eps)
    z = torch.zeros(3, 3 * 2 * 64)
    with pytest.raises(ValueError, match="qk_norm must be a"):
        F.qk_norm(z, 2, torch.zeros(4, 48))
    with pytest.raises(ValueError, match="params must be"):
        F.qk_norm(z, 2, None)
    with pytest.raises(ValueError, match="packed width"):
        F.qk_norm(torch.zeros(3, 100), 2, torch.zeros(4, 64))
    with pytest.raises(ValueError, match="head dim"):
        F.qk_norm(torch.zeros(3, 3 * 2 * 48), 2, torch.zeros(4, 48))          # a packed width of 48 is not a kernel head dim
    with pytest.raises(ValueError, match="head dim"):
        F.qk_norm(z, 2, torch.zeros(4, 64), head_dim=65)


@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_torch_compile_refuses_qk_norm(pre):
    """Decided while tracing, before any kernel: the encoder alone, on a machine without a GPU."""
    from sfcvit.models import TransformerSeqEncoder
    enc = TransformerSeqEncoder(128, 4, 2, 256, None, dropout_p=0.0, n_layers=1, qk_norm=True, norm_first=pre).to(torch.bfloat16).eval()
    want = "the pre-norm layer has no traced form" if pre else "qk_norm is not supported under torch.compile"
    try:
        with pytest.raises(NotImplementedError, match=want):
            torch.compile(enc)(torch.randn(2, 4, 128, dtype=torch.bfloat16))
    finally:
        torch._dynamo.reset()


def _main_module():
    spec = importlib.util.spec_from_file_location("sfcvit_main_py", os.path.join(PKG, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_main_py_options():
    main = _main_module()
    small = ["--tokenizer", "hilbert", "--img-size", "32", "--patch-size", "16", "--embed-dim", "64", "--depth", "3", "--heads", "2",
             "--mlp-dim", "128"]
    a = main.parse_args(small)
    assert a.qk_norm is None and not hasattr(main.build_model(a, main.build_tokenizer(a)).encoder, "qk_norm")
    a = main.parse_args(small + ["--qk-norm"])
    enc = main.build_model(a, main.build_tokenizer(a)).encoder
    assert a.qk_norm == 1e-6 and len(enc.qk_norm) == 3 and tuple(enc.qk_norm[0].shape) == (4, 32) and enc.qk_norm_eps == 1e-6
    assert not enc.norm_first
    a = main.parse_args(small + ["--qk-norm", "1e-5", "--pre-norm", "--activation", "gelu", "--layer-scale", "--drop-path", "0.1",
                                 "--rel-pos-bias", "curve", "--pool", "mean", "--pos-embed", "learned"])
    enc = main.build_model(a, main.build_tokenizer(a)).encoder
    assert enc.qk_norm_eps == 1e-5 and enc.norm_first and len(enc.layer_scale) == 3 and len(enc.rel_pos_bias) == 3 and len(enc.qk_norm) == 3
    for bad in (["--qk-norm", "-1"], ["--qk-norm", "nan"], ["--qk-norm", "inf"], ["--qk-norm", "x"]):
        with pytest.raises(SystemExit):
            main.parse_args(small + bad)
