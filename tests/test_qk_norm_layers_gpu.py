"""QK-norm in the layers and the models on the GPU: option off = the bits of a call without the argument; option on = the post-
and pre-norm layers against the fp32 reference (qk_norm_ref) with the same masks and flags at the bars the layer tests of the
project hold the same quantities to (outputs close(1/32, 1/24); every gradient cosine > 0.99 and norm within 5 %, the bar of the
LayerNorm gains for the new parameter; the in_proj bias gradient per third); the models: eval logits, training steps through the
flat gradient buffer, the captured step, main.py with --resume, and attention_report."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prenorm_ref
import qk_norm_ref
from oracle import formula
from oracle.cases import MODEL_CASES
from prenorm_ref import keep_flags
from token_pool_ref import build_with

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
POST = ["in_w", "in_b", "out_w", "out_b", "n1_w", "n1_b", "w1", "b1", "w2", "b2", "n2_w", "n2_b"]
GEOMETRIES = {"D128_H2": (3, 9, 128, 2), "D192_H4_padded": (3, 9, 192, 4)}          # (B, N, D, H), F = 2 D; hd 64 and 48
SEEDS = (11, 22, 33, 44)


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int16)


def _params(B, N, D, H, pre, seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, device="cuda", generator=g) * sc)     # noqa: E731
    Fd, hd = 2 * D, D // H
    shapes = dict(in_w=((3 * D, D), D ** -0.5), in_b=((3 * D,), 0.1), out_w=((D, D), D ** -0.5), out_b=((D,), 0.1),
                  w1=((Fd, D), D ** -0.5), b1=((Fd,), 0.1), w2=((D, Fd), Fd ** -0.5), b2=((D,), 0.1))
    names = prenorm_ref.ORDER if pre else POST
    P = {k: (r(*shapes[k][0], sc=shapes[k][1]) if k in shapes else (1 + r(D, sc=0.1) if k.endswith("_w") else r(D, sc=0.1))).to(BF16)
         for k in names}
    x = r(B, N, D).to(BF16)
    n = torch.nn.functional.layer_norm(x.float(), (D,), 1 + r(D, sc=0.1), r(D, sc=0.1)).to(BF16)
    qk = torch.stack([1 + r(hd, sc=0.2), r(hd, sc=0.2), 1 + r(hd, sc=0.2), r(hd, sc=0.2)]).to(BF16)
    lam = r(2, D, sc=0.1).to(BF16)
    return x, n, P, qk, lam, r(B, N, D).to(BF16), r(B, N, D).to(BF16)


def _path_seeds(B, rate):
    """Two path seeds whose flags keep some and drop some of the B images, differently at the two sites."""
    found = []
    for s in range(1, 400, 2):
        k = keep_flags(s, rate, B)
        if 0 < k.sum() < B and all(not np.array_equal(k, keep_flags(f, rate, B)) for f in found):
            found.append(s)
        if len(found) == 2:
            return tuple(found)
    raise AssertionError("no mixed flags")


# ---- option off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_option_off_is_the_call_without_the_argument(ops, pre, geometry):
    import sfcvit.functional as F
    B, N, D, H = GEOMETRIES[geometry]
    x, n, P, _, _, dy, dn = _params(B, N, D, H, pre)
    names = prenorm_ref.ORDER if pre else POST
    runs = []
    for kw in ({}, dict(qk_norm=None), dict(qk_norm=None, qk_norm_eps=1e-3)):
        leaves = [x.clone().requires_grad_(True)] + ([n.clone().requires_grad_(True)] if pre else []) + [P[k].clone().requires_grad_(True) for k in names]
        torch.manual_seed(9)
        ops.KERNEL_LOG = []
        try:
            if pre:
                out = F.pre_norm_layer(*leaves, H, dropout_p=0.1, drop_path=0.2, activation="gelu", **kw)
                torch.autograd.backward(list(out), [dy, dn])
            else:
                out = (F.encoder_layer(*leaves, H, dropout_p=0.1, drop_path=0.2, **kw),)
                out[0].backward(dy)
            log = list(ops.KERNEL_LOG)
        finally:
            ops.KERNEL_LOG = None
        torch.cuda.synchronize()
        runs.append(([bits(o.detach()) for o in out], [bits(t.grad) for t in leaves], log))
        assert not any("qk_norm" in k for k in log) and "qk_norm" not in ops.last_rowwise_kernel()
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0], other[0]))
        assert all(torch.equal(a, b) for a, b in zip(runs[0][1], other[1]))
        assert runs[0][2] == other[2]


# ---- option on: the layers against the fp32 reference --------------------------------------------------------------------------
def _run_layer(ops, geometry, pre, act="relu", with_lam=False, rate=0.0, p=0.0, masked=False, biased=False, qk_eps=1e-6):
    import sfcvit.functional as F
    from sfcvit import masks, relpos
    from attn_bias_ref import bias_term
    from test_dropout_gpu import close
    B, N, D, H = GEOMETRIES[geometry]
    Fd, M, hd = 2 * D, B * N, D // H
    hp = ops.padded_head_dim(hd)
    x, n, P, qk, lam, dy, dn = _params(B, N, D, H, pre)
    names = prenorm_ref.ORDER if pre else POST
    pseeds = _path_seeds(B, rate) if rate > 0 else (0, 0)
    k1, k2 = (keep_flags(s_, rate, B) for s_ in pseeds) if rate > 0 else (np.ones(B, bool), np.ones(B, bool))
    window = masks.curve_window(N, 3) if masked else None
    am = ops.as_attention_mask(window, N) if masked else None
    table = index = idx = None
    if biased:
        idx, T = relpos.curve_offsets(N, 4)
        index = ops.AttentionBiasIndex(idx, T)
        table = (0.5 * torch.randn(H, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))).requires_grad_(True)
    leaves = {k: P[k].clone().requires_grad_(True) for k in names}
    xl, nl = x.clone().requires_grad_(True), n.clone().requires_grad_(True)
    qkl = qk.clone().requires_grad_(True)
    lam_leaf = lam.clone().requires_grad_(True) if with_lam else None
    # the public path's own argument preparation (the per-head zero padding of in_proj / out_proj), then the Function with
    # explicit seeds so that the reference can draw the same masks and flags
    args, scale = F._encoder_layer_args(xl, *[leaves[k] for k in names], H)
    seeds = SEEDS if p > 0 else (0, 0, 0, 0)
    cfg = F._LayerCfg(H, 1e-5, p, seeds, scale, act, am, (rate, pseeds) if rate > 0 else None, index, qk_eps)
    ops.KERNEL_LOG = []
    try:
        if pre:
            out = F._PreNormLayer.apply(args[0], nl, *args[1:], lam_leaf, table, cfg, qkl)
            torch.autograd.backward(list(out), [dy, dn])
        else:
            out = (F._EncoderLayer.apply(*args, table, cfg, qkl),)
            out[0].backward(dy)
        ran = list(ops.KERNEL_LOG)
    finally:
        ops.KERNEL_LOG = None
    torch.cuda.synchronize()
    assert ran.count(f"qk_norm_fwd_kernel<{hp}>") == 1 and ran.count(f"qk_norm_bwd_kernel<{hp}>") == 1, ran
    assert masked == any("masked" in k for k in ran) and biased == any("attn_bias" in k for k in ran)

    one = torch.ones((), device="cuda")
    if p > 0:
        ms = (ops.dropout_mask(B * H * N, N, p, seeds[0]).float().view(B, H, N, N), ops.dropout_mask(M, D, p, seeds[1]).float().view(B, N, D),
              ops.dropout_mask(M, Fd, p, seeds[2]).float().view(B, N, Fd), ops.dropout_mask(M, D, p, seeds[3]).float().view(B, N, D))
    else:
        ms = (one, one, one, one)
    c1, c2 = (torch.from_numpy(k).cuda().float() / (1 - rate) for k in (k1, k2))
    xr, nr = x.float().requires_grad_(True), n.float().requires_grad_(True)
    R = {k: v.float().requires_grad_(True) for k, v in P.items()}
    qr = qk.float().requires_grad_(True)
    lr = lam.float().requires_grad_(True) if with_lam else None
    tr = table.detach().clone().requires_grad_(True) if biased else None
    rb = bias_term(tr, idx.cuda()) if biased else None
    wm = window.cuda() if masked else None
    if pre:
        ref = qk_norm_ref.pre_norm_layer(xr, nr, R, H, ms, c1, c2, (lr[0], lr[1]) if with_lam else None, act, attn_mask=wm, rel_bias=rb,
                                         qk_norm=qr, qk_eps=qk_eps)
        torch.autograd.backward(list(ref), [dy.float(), dn.float()])
    else:
        ref = (qk_norm_ref.encoder_layer(xr, R, H, ms, c1, c2, attn_mask=wm, qk_norm=qr, qk_eps=qk_eps, rel_bias=rb),)
        ref[0].backward(dy.float())
    tag = f"{geometry} {'pre' if pre else 'post'}-norm {act} lam={with_lam} drop_path={rate} p={p}" + (" masked" if masked else "") + (" rel_bias" if biased else "")
    for o, r_ in zip(out, ref):
        print(f"[{tag}] output max err {float((o.float() - r_.detach()).abs().max()):.3e}")
        close(o, r_.detach(), rel=1 / 32, abs_scale=1 / 24)
    pairs = [("x", xl, xr)] + ([("n", nl, nr)] if pre else []) + [(k, leaves[k], R[k]) for k in names] + [("qk_norm", qkl, qr)]
    if with_lam:
        pairs.append(("lam", lam_leaf, lr))
    if biased:
        pairs.append(("rel_table", table, tr))
    thirds = [(f"in_b[{name}]", leaves["in_b"].grad[i * D:(i + 1) * D], R["in_b"].grad[i * D:(i + 1) * D]) for i, name in enumerate("qkv")]
    # k_bias is left out of the row-wise bars: a bias on the keys moves every score of a query by the same amount, the softmax
    # cancels it, and its exact gradient is 0 (sum_j dS_ij = 0 per query).  What either side computes is rounding noise: the sum of
    # B * N * H rounded dk rows that cancel, each stored to 2^-9 of itself, next to q_bias's sum of as many dq rows of the same
    # size that do not cancel -- at most 2^-8 * sqrt(B * N * H) of it for independent roundings, 0.04 here; held to 0.1.
    rows = [(f"qk_norm[{name}]", qkl.grad[i], qr.grad[i]) for i, name in enumerate(("q_weight", "q_bias", "k_weight"))]
    kb = float(qkl.grad[3].float().norm() / qr.grad[1].norm())
    print(f"    dqk_norm[k_bias]: norm {float(qkl.grad[3].float().norm()):.3e} (reference {float(qr.grad[3].norm()):.3e}), {kb:.4f} of q_bias's")
    assert kb <= 0.1, (tag, "k_bias", kb)
    worst = []
    for name, got, ref_ in [(nm, a.grad, b.grad) for nm, a, b in pairs] + thirds + rows:
        gg, rr = got.float().flatten(), ref_.flatten()
        cos, ratio = float(torch.dot(gg, rr) / (gg.norm() * rr.norm() + 1e-30)), float(gg.norm() / rr.norm())
        print(f"    d{name}: cosine {cos:.5f}, norm ratio {ratio:.4f}")
        worst.append((name, cos, ratio))
    for name, cos, ratio in worst:
        assert cos > 0.99, (tag, name, cos)
        assert abs(ratio - 1) < 5e-2, (tag, name, ratio)


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_post_norm_layer(ops, geometry):
    _run_layer(ops, geometry, pre=False)
    _run_layer(ops, geometry, pre=False, p=0.1, rate=0.5)


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("act,with_lam", [("relu", False), ("gelu", True)], ids=["relu", "gelu_layer_scale"])
def test_pre_norm_layer(ops, geometry, act, with_lam):
    _run_layer(ops, geometry, pre=True, act=act, with_lam=with_lam)
    _run_layer(ops, geometry, pre=True, act=act, with_lam=with_lam, p=0.1, rate=0.5)


@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_layer_with_a_curve_window(ops, pre):
    _run_layer(ops, "D128_H2", pre, act="gelu" if pre else "relu", with_lam=pre, p=0.1, masked=True)
    _run_layer(ops, "D192_H4_padded", pre, masked=True)


@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_layer_with_a_relative_position_bias(ops, pre):
    _run_layer(ops, "D128_H2", pre, act="gelu" if pre else "relu", with_lam=pre, p=0.1, rate=0.5, biased=True)
    _run_layer(ops, "D192_H4_padded", pre, biased=True, qk_eps=1e-5)


def test_public_layer_calls_reach_the_kernels(ops):
    """F.encoder_layer / F.pre_norm_layer with qk_norm= run the QK-norm kernels once per direction and hand the parameter its
    gradient; the probes return the normalised q, k."""
    import sfcvit.functional as F
    B, N, D, H = GEOMETRIES["D192_H4_padded"]
    hd, hp = D // H, 64
    for pre in (False, True):
        x, n, P, qk, _, dy, dn = _params(B, N, D, H, pre)
        names = prenorm_ref.ORDER if pre else POST
        w = [P[k] for k in names]
        qkl = qk.clone().requires_grad_(True)
        ops.KERNEL_LOG = []
        try:
            if pre:
                out = F.pre_norm_layer(x, n, *w, H, qk_norm=qkl, qk_norm_eps=1e-5)
                torch.autograd.backward(list(out), [dy, dn])
                probe = F.pre_norm_layer_probe(x, n, *w, H, qk_norm=qk, qk_norm_eps=1e-5)
                y, qkv = probe[1], probe[2]
            else:
                out = (F.encoder_layer(x, *w, H, qk_norm=qkl, qk_norm_eps=1e-5),)
                out[0].backward(dy)
                y, qkv, _, _ = F.encoder_layer_probe(x, *w, H, qk_norm=qk, qk_norm_eps=1e-5)
            log = list(ops.KERNEL_LOG)
        finally:
            ops.KERNEL_LOG = None
        assert log.count("qk_norm_fwd_kernel<64>") == 2 and log.count("qk_norm_bwd_kernel<64>") == 1, log
        assert qkl.grad is not None and tuple(qkl.grad.shape) == (4, hd)
        assert all(float(qkl.grad[i].float().abs().max()) > 0 for i in range(3))
        assert torch.equal(bits(y), bits(out[-1].detach()))
        t = qkv.view(B * N, 3, H, hp)[:, :2, :, :hd].float()
        # the probe's q, k are LayerNorm outputs: per head row, (t - beta) / gamma has mean 0 and variance 1 up to bf16 rounding
        for i in range(2):
            z = (t[:, i] - qk[2 * i + 1].float()) / qk[2 * i].float()
            assert float(z.mean(-1).abs().max()) < 0.05 and float((z.var(-1, unbiased=False) - 1).abs().max()) < 0.1
        assert int((bits(qkv.view(B * N, 3, H, hp)[:, :2, :, hd:]) != 0).sum()) == 0


# ---- models --------------------------------------------------------------------------------------------------------------------
def _tiny_model(rate=0.0, dropout=0.0, seed=11, name="hilbert32_1d", **kw):
    cfg, batch = MODEL_CASES[name]
    torch.manual_seed(seed)
    model = build_with(cfg, dropout_p=dropout, head_dropout_p=dropout, drop_path_rate=rate, **kw)
    x = formula.image_batch(batch, 3, cfg.img_size, cfg.img_size).cuda()
    tgt = formula.soft_targets(batch, cfg.num_classes).cuda()
    return model.to("cuda", dtype=BF16), x, tgt, cfg


def _shake(model):
    """Norms, biases and the QK-norm rows away from their ones and zeros."""
    with torch.no_grad():
        for k, prm in model.encoder.named_parameters():
            if prm.dim() == 1 or "qk_norm" in k:
                prm.add_((0.2 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(len(k)))).to(prm))


def _encoder_ref(model, t, probs=None):
    """The encoder of a post- or pre-norm QK-norm model in fp32 on the CPU, on the weights of `model`."""
    f = lambda v: v.detach().float().cpu()                                         # noqa: E731
    enc, H = model.encoder, model.encoder.n_head
    B, N, D = t.shape
    one, ones = torch.ones(()), torch.ones(B)
    if not enc.norm_first:
        for l, L in enumerate(prenorm_ref.layers_of(_Layers(enc.transformer))[0]):
            Pd = {k: f(v) for k, v in L.items()}
            if probs is not None:
                probs.append(qk_norm_ref.attention(t @ Pd["in_w"].t() + Pd["in_b"], H, f(enc.qk_norm[l]), enc.qk_norm_eps)[1])
            t = qk_norm_ref.encoder_layer(t, Pd, H, (one, one, one, one), ones, ones, qk_norm=f(enc.qk_norm[l]), qk_eps=enc.qk_norm_eps)
        return t
    layers, final = prenorm_ref.layers_of(enc.transformer)
    s = t
    n = torch.nn.functional.layer_norm(s, (D,), f(layers[0]["n1_w"]), f(layers[0]["n1_b"]))
    scales = getattr(enc, "layer_scale", None)
    for l, L in enumerate(layers):
        nxt = (layers[l + 1]["n1_w"], layers[l + 1]["n1_b"]) if l + 1 < len(layers) else final
        Pf = {k_: f(v) for k_, v in dict(L, next_w=nxt[0], next_b=nxt[1]).items()}
        if probs is not None:
            probs.append(qk_norm_ref.attention(n @ Pf["in_w"].t() + Pf["in_b"], H, f(enc.qk_norm[l]), enc.qk_norm_eps)[1])
        s, n = qk_norm_ref.pre_norm_layer(s, n, Pf, H, lam=(f(scales[l][0]), f(scales[l][1])) if scales is not None else None,
                                          act=enc.activation, qk_norm=f(enc.qk_norm[l]), qk_eps=enc.qk_norm_eps)
    return n


class _Layers:
    """layers_of reads `.layers` and `.norm`; a post-norm encoder has no final norm."""

    def __init__(self, tr):
        self.layers = tr.layers
        self.norm = tr.layers[0].norm1


@pytest.mark.parametrize("kw", [dict(), dict(norm_first=True, activation="gelu", layer_scale=0.5)], ids=["post_norm", "pre_norm"])
def test_eval_logits_against_the_torch_reference(kw):
    from test_parity_gpu import LOGIT_TOL
    model, x, _, cfg = _tiny_model(qk_norm=True, **kw)
    _shake(model)
    model.eval()
    with torch.no_grad():
        got = model(x).float().cpu()
        t = model.mlp_mixer(model.patch_embed(x))
        want_tokens = _encoder_ref(model, t.float().cpu())
        want = model.mlp_head(want_tokens.to("cuda", dtype=BF16)).float().cpu()
        enc = model.encoder(t).float().cpu()
        model_off, _, _, _ = _tiny_model(**kw)
        model_off.load_state_dict({k: v for k, v in model.state_dict().items() if "qk_norm" not in k})
        off = model_off.eval()(x).float().cpu()
    scale = float(want.abs().max())
    err, tok_err = float((got - want).abs().max()), float((enc - want_tokens).abs().max() / want_tokens.abs().max())
    print(f"logits max err {err:.3e} of {scale:.3e}; encoder output max err {tok_err:.3e} of its largest value; "
          f"without qk_norm the logits move by {float((got - off).abs().max()):.3e}")
    assert err <= LOGIT_TOL * scale and tok_err <= LOGIT_TOL
    assert float((got - off).abs().max()) > err, "the norm changed nothing"


def _wide_model(seed=3, **kw):
    """embed_dim 128, 2 heads: head dim 64, so in_proj is not padded and its bias is a leaf with a gradient slot of its own."""
    from sfcvit.models import VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    torch.manual_seed(seed)
    model = VisionTransformer1D(HilbertEmbedding1D(32, 64, 3, 128), depth=2, n_heads=2, mlp_dim=256, num_classes=10, dropout_p=0.0,
                                head_dropout_p=0.0, qk_norm=True, **kw)
    x = formula.image_batch(4, 3, 32, 32).cuda()
    return model.to("cuda", dtype=BF16), x, formula.soft_targets(4, 10).cuda()


@pytest.mark.parametrize("wide", [False, True], ids=["padded_heads", "head_dim_64"])
def test_training_steps_write_the_gradients_into_their_slots(ops, wide):
    import sfcvit.functional as F
    from sfcvit.training import FusedAdamW, train_step
    make = (lambda: _wide_model()[:3]) if wide else (lambda: _tiny_model(qk_norm=True)[:3])
    plain, x, tgt = make()
    plain.train()
    F.soft_target_cross_entropy(plain(x), tgt).backward()
    model, _, _ = make()
    model.train()
    opt = FusedAdamW(model.parameters(), lr=0.0, weight_decay=0.0)
    train_step(model, x, tgt, opt)                              # builds the flat buffers; from now on gradients go into slots
    opt.zero_grad()
    ops.KERNEL_LOG = []
    try:
        F.soft_target_cross_entropy(model(x), tgt).backward()
        log = list(ops.KERNEL_LOG)
    finally:
        ops.KERNEL_LOG = None
    torch.cuda.synchronize()
    depth = len(model.encoder.qk_norm)
    assert sum(k.startswith("qk_norm_fwd") for k in log) == depth and sum(k.startswith("qk_norm_bwd") for k in log) == depth
    ref = dict(plain.named_parameters())
    for k, prm in model.named_parameters():
        if "qk_norm" in k or "in_proj_bias" in k:
            buf, off = prm._sfcvit_slot
            assert buf is opt
            a, b = ref[k].grad.float(), prm.grad.float()
            if "qk_norm" in k or wide:
                assert prm.grad.data_ptr() == buf.flat_grad.data_ptr() + 2 * off, f"{k}: the gradient is not its slot"
            print(f"{k}: max |slot - plain| {float((a - b).abs().max()):.3e} of {float(a.abs().max()):.3e}")
            assert float((a - b).abs().max()) <= 2.0 ** -7 * float(a.abs().max()) + 1e-12, k
            assert float(b.abs().max()) > 0, k
    # three real steps: finite loss, the parameters moved
    model2, _, _ = make()
    model2.train()
    before = [p.detach().clone() for p in model2.encoder.qk_norm]
    opt2 = FusedAdamW(model2.parameters(), lr=1e-2, weight_decay=5e-2)
    losses = [float(train_step(model2, x, tgt, opt2)) for _ in range(3)]
    print(losses)
    assert all(np.isfinite(losses))
    for p0, p1 in zip(before, model2.encoder.qk_norm):
        # (k_bias, row 3, has an exact gradient of 0 -- the softmax cancels a bias on the keys -- and is not asked to move)
        assert all(float((p0[i].float() - p1[i].float()).abs().max()) > 0 for i in range(3)), "a QK-norm row did not move"


@pytest.mark.parametrize("kw", [dict(), dict(norm_first=True, activation="gelu", layer_scale=0.5)], ids=["post_norm", "pre_norm"])
def test_graphed_train_step_takes_the_eager_steps(kw):
    """Replays of the captured step equal eager steps three to five (two warm-up steps first), at dropout 0: the loss bit for bit,
    every parameter bytewise."""
    from sfcvit import ops
    from sfcvit.training import FusedAdamW, GraphedTrainStep, train_step
    try:
        model_e, x, tgt, _ = _tiny_model(qk_norm=True, **kw)
        model_e.train()
        opt_e = FusedAdamW(model_e.parameters(), lr=1e-3, weight_decay=5e-2)
        opt_e.use_device_state(seed_base=4242)
        eager = [train_step(model_e, x, tgt, opt_e).float().cpu() for _ in range(5)]
        model_g, _, _, _ = _tiny_model(qk_norm=True, **kw)
        model_g.train()
        opt_g = FusedAdamW(model_g.parameters(), lr=1e-3, weight_decay=5e-2)
        opt_g.use_device_state(seed_base=4242)
        step = GraphedTrainStep(model_g, x.clone(), tgt.clone(), opt_g, warmup=2, preserve_state=False)
        graphed = [step().float().cpu() for _ in range(3)]
        print([float(v) for v in eager], [float(v) for v in graphed])
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(eager[2:], graphed))
        for (k, a), (_, b) in zip(model_e.state_dict().items(), model_g.state_dict().items()):
            assert torch.equal(bits(a) if a.dtype == BF16 else a, bits(b) if b.dtype == BF16 else b), k
        assert float((model_g.encoder.qk_norm[0][1].float()).abs().max()) > 0      # the zero bias row was trained
        step.close()
    finally:
        ops.STEP_STATE = None


def _main_py(tmp_path, *extra):
    main = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd", "main.py")
    return [sys.executable, main, "--synthetic", "--tokenizer", "hilbert", "--img-size", "32", "--patch-size", "16", "--embed-dim", "64",
            "--depth", "2", "--heads", "2", "--mlp-dim", "128", "--batch-size", "64", "--train-size", "256", "--test-size", "128",
            "--warmup-epochs", "0", "--qk-norm", "--checkpoint-dir", str(tmp_path), *extra]


@pytest.mark.parametrize("extra", [[], ["--pre-norm", "--activation", "gelu", "--layer-scale"]], ids=["post_norm", "pre_norm"])
def test_main_py_trains_and_resumes(tmp_path, extra):
    out = subprocess.run(_main_py(tmp_path, "--epochs", "1", *extra), capture_output=True, text=True, timeout=300)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stderr[-3000:]
    assert "Epoch 1/1" in out.stdout, out.stdout[-1000:]
    ck = os.path.join(str(tmp_path), "checkpoint_hilbert.pt")
    sd = torch.load(ck, map_location="cpu", weights_only=True)["model_state_dict"]
    assert {"encoder.qk_norm.0", "encoder.qk_norm.1"} <= set(sd) and tuple(sd["encoder.qk_norm.1"].shape) == (4, 32)
    init = torch.tensor([1.0, 0.0, 1.0, 0.0])[:, None].expand(4, 32)
    assert not torch.equal(sd["encoder.qk_norm.0"].float(), init), "training left the QK-norm rows at their initial values"
    out = subprocess.run(_main_py(tmp_path, "--epochs", "2", "--resume", ck, *extra), capture_output=True, text=True, timeout=300)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stderr[-3000:]
    assert "Epoch 2/2" in out.stdout and "Epoch 1/2" not in out.stdout, out.stdout[-1000:]
    # --resume restores the keys: a model built from the same arguments takes the checkpoint strictly
    sd2 = torch.load(ck, map_location="cpu", weights_only=True)["model_state_dict"]
    assert set(sd2) == set(sd)


@pytest.mark.parametrize("kw", [dict(), dict(norm_first=True, activation="gelu", layer_scale=0.5)], ids=["post_norm", "pre_norm"])
def test_attention_report_on_a_qk_norm_model(kw):
    """The report's maps are those of the NORMALISED q, k: rows sum to 1, distance and entropy agree with the fp32 reference at the
    bar of the report's model test, and the maps of every layer agree with the reference's softmax within the bound below."""
    from sfcvit.analysis import attention_report, token_positions
    from test_attention_probe_gpu import TOL_F32, TOL_MODEL
    model, x, _, cfg = _tiny_model(qk_norm=True, **kw)
    _shake(model)
    model.train()
    rep = attention_report(model, x, maps=True, head_mean=False)
    assert model.training
    with torch.no_grad():
        want = model.eval()(x)
        t = model.mlp_mixer(model.patch_embed(x)).float().cpu()
    assert torch.equal(rep["logits"], want)
    probs = []
    with torch.no_grad():
        _encoder_ref(model, t, probs)
    pos = token_positions(model.patch_embed)
    dmat = (pos[:, None] - pos[None]).norm(dim=-1)
    B, N, _ = t.shape
    H, hd = model.encoder.n_head, cfg.embed_dim // cfg.n_heads
    dscale, escale = float(dmat.max()), max(math.log(N), 1.0)
    assert len(rep["layers"]) == len(probs) == cfg.depth
    # q_hat and k_hat are bf16: each carries a relative rounding of 2^-9 from its own store and as much again from the rounded
    # projection it was normalised from, so a score moves by at most 4 * 2^-9 * sum_i |q_i k_i| / sqrt(hd) <= 2^-7 * |q| |k| /
    # sqrt(hd) =: delta (Cauchy-Schwarz), and a probability by at most (e^(2 delta) - 1) of itself (numerator and denominator
    # each by e^delta).  A LayerNorm output has |gamma * x_hat + beta| <= sqrt(hd) (max|gamma| + max|beta|).
    for e, P in zip(rep["layers"], probs):
        qk = model.encoder.qk_norm[e["layer"]].detach().float().cpu()
        qmax = math.sqrt(hd) * (float(qk[0].abs().max()) + float(qk[1].abs().max()))
        kmax = math.sqrt(hd) * (float(qk[2].abs().max()) + float(qk[3].abs().max()))
        delta = 2.0 ** -7 * qmax * kmax / math.sqrt(hd)
        m = e["map"].float().cpu()
        assert tuple(m.shape) == (B, H, N, N) and e["mass_error"] <= TOL_F32
        assert float((m.sum(-1) - 1).abs().max()) <= 1e-3
        worst = float(((m - P).abs() / (P * math.expm1(2 * delta) + 1e-6)).max())
        fd = float((e["distance"].cpu() - (P * dmat).sum(-1).mean(-1)).abs().max()) / dscale
        fe = float((e["entropy"].cpu() + (P * torch.log(P.clamp_min(1e-30))).sum(-1).mean(-1)).abs().max()) / escale
        print(f"FIGURE qk-norm model layer {e['layer']}: distance={fd:.3e} entropy={fe:.3e} mass={e['mass_error']:.3e} "
              f"map worst {worst:.3f} of its bound (delta {delta:.3f})")
        assert worst <= 1.0 and fd <= TOL_MODEL and fe <= TOL_MODEL, (worst, fd, fe)
