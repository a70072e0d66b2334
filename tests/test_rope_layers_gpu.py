"""Rotary position embeddings in the layers and the models on the GPU: option off = the bits of a call without the argument;
option on = the post- and pre-norm layers against the fp32 reference (rope_ref) with the same masks and flags at the bars
test_qk_norm_layers_gpu holds the same quantities to (outputs close(1/32, 1/24); every gradient cosine > 0.99 and norm within
5 %; the in_proj bias gradient per third -- the check that catches a wrong owner of the column sums); the models: eval logits,
gradient slots written whole, the captured step, main.py with --resume, and attention_report."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import prenorm_ref
import rope_ref
from prenorm_ref import keep_flags
from test_qk_norm_layers_gpu import GEOMETRIES, POST, SEEDS, _Layers, _params, _path_seeds, _shake, _tiny_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from sfcvit import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int16)


def _table(N, hd, kind="curve"):
    """A table whose angles differ visibly from token to token at N = 9: the curve table at a small base, or arbitrary angles."""
    from sfcvit import rope
    if kind == "curve":
        return rope.curve_table(N, hd, base=50.0)
    theta = torch.rand(N, hd // 2, generator=torch.Generator().manual_seed(N + hd), dtype=torch.float64) * (2 * math.pi)
    return torch.stack((theta.cos(), theta.sin()), -1).float()


# ---- option off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_option_off_is_the_call_without_the_argument(ops, pre, geometry):
    import sfcvit.functional as F
    B, N, D, H = GEOMETRIES[geometry]
    x, n, P, qk, _, dy, dn = _params(B, N, D, H, pre)
    names = prenorm_ref.ORDER if pre else POST
    for base in ({}, dict(qk_norm=qk)):
        runs = []
        for kw in ({}, dict(rope=None)):
            leaves = [x.clone().requires_grad_(True)] + ([n.clone().requires_grad_(True)] if pre else []) + [P[k].clone().requires_grad_(True) for k in names]
            torch.manual_seed(9)
            ops.KERNEL_LOG = []
            try:
                if pre:
                    out = F.pre_norm_layer(*leaves, H, dropout_p=0.1, drop_path=0.2, activation="gelu", **base, **kw)
                    torch.autograd.backward(list(out), [dy, dn])
                else:
                    out = (F.encoder_layer(*leaves, H, dropout_p=0.1, drop_path=0.2, **base, **kw),)
                    out[0].backward(dy)
                log = list(ops.KERNEL_LOG)
            finally:
                ops.KERNEL_LOG = None
            torch.cuda.synchronize()
            runs.append(([bits(o.detach()) for o in out], [bits(t.grad) for t in leaves], log))
            assert not any("rope" in k for k in log) and "rope" not in ops.last_rowwise_kernel()
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
        assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
        assert runs[0][2] == runs[1][2]


# ---- option on: the layers against the fp32 reference --------------------------------------------------------------------------
def _run_layer(ops, geometry, pre, act="relu", with_lam=False, rate=0.0, p=0.0, masked=False, biased=False, with_qk=False, kind="curve"):
    import sfcvit.functional as F
    from sfcvit import masks, relpos
    from attn_bias_ref import bias_term
    from test_dropout_gpu import close
    B, N, D, H = GEOMETRIES[geometry]
    Fd, M, hd = 2 * D, B * N, D // H
    hp = ops.padded_head_dim(hd)
    x, n, P, qk, lam, dy, dn = _params(B, N, D, H, pre)
    rope_cpu = _table(N, hd, kind)
    rt = ops.RopeTable(rope_cpu)
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
    qkl = qk.clone().requires_grad_(True) if with_qk else None
    lam_leaf = lam.clone().requires_grad_(True) if with_lam else None
    # the public path's own argument preparation (the per-head zero padding of in_proj / out_proj), then the Function with
    # explicit seeds so that the reference can draw the same masks and flags
    args, scale = F._encoder_layer_args(xl, *[leaves[k] for k in names], H)
    seeds = SEEDS if p > 0 else (0, 0, 0, 0)
    cfg = F._LayerCfg(H, 1e-5, p, seeds, scale, act, am, (rate, pseeds) if rate > 0 else None, index, 1e-6, rt)
    tail = (qkl,) if with_qk else ()
    ops.KERNEL_LOG = []
    try:
        if pre:
            out = F._PreNormLayer.apply(args[0], nl, *args[1:], lam_leaf, table, cfg, *tail)
            torch.autograd.backward(list(out), [dy, dn])
        else:
            out = (F._EncoderLayer.apply(*args, table, cfg, *tail),)
            out[0].backward(dy)
        ran = list(ops.KERNEL_LOG)
    finally:
        ops.KERNEL_LOG = None
    torch.cuda.synchronize()
    assert ran.count(f"rope_fwd_kernel<{hp}>") == 1 and ran.count(f"rope_bwd_kernel<{hp}>") == 1, ran
    assert ran.count(f"qk_norm_fwd_kernel<{hp}>") == int(with_qk) and ran.count(f"qk_norm_bwd_kernel<{hp}>") == int(with_qk), ran
    if with_qk:                                                 # forward: norm, then rotation; backward: the mirror
        assert ran.index(f"qk_norm_fwd_kernel<{hp}>") < ran.index(f"rope_fwd_kernel<{hp}>")
        assert ran.index(f"rope_bwd_kernel<{hp}>") < ran.index(f"qk_norm_bwd_kernel<{hp}>")
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
    qr = qk.float().requires_grad_(True) if with_qk else None
    lr = lam.float().requires_grad_(True) if with_lam else None
    tr = table.detach().clone().requires_grad_(True) if biased else None
    rb = bias_term(tr, idx.cuda()) if biased else None
    wm = window.cuda() if masked else None
    if pre:
        ref = rope_ref.pre_norm_layer(xr, nr, R, H, ms, c1, c2, (lr[0], lr[1]) if with_lam else None, act, attn_mask=wm, rel_bias=rb,
                                      qk_norm=qr, rope=rope_cpu.cuda())
        torch.autograd.backward(list(ref), [dy.float(), dn.float()])
    else:
        ref = (rope_ref.encoder_layer(xr, R, H, ms, c1, c2, attn_mask=wm, qk_norm=qr, rel_bias=rb, rope=rope_cpu.cuda()),)
        ref[0].backward(dy.float())
    tag = (f"{geometry} {'pre' if pre else 'post'}-norm {act} rope={kind} qk_norm={with_qk} lam={with_lam} drop_path={rate} p={p}"
           + (" masked" if masked else "") + (" rel_bias" if biased else ""))
    for o, r_ in zip(out, ref):
        print(f"[{tag}] output max err {float((o.float() - r_.detach()).abs().max()):.3e}")
        close(o, r_.detach(), rel=1 / 32, abs_scale=1 / 24)
    pairs = [("x", xl, xr)] + ([("n", nl, nr)] if pre else []) + [(k, leaves[k], R[k]) for k in names]
    if with_lam:
        pairs.append(("lam", lam_leaf, lr))
    if biased:
        pairs.append(("rel_table", table, tr))
    thirds = [(f"in_b[{name}]", leaves["in_b"].grad[i * D:(i + 1) * D], R["in_b"].grad[i * D:(i + 1) * D]) for i, name in enumerate("qkv")]
    # (with a rotation behind the norm the softmax no longer cancels a bias on the keys -- it is turned by a different angle per
    # token -- so k_bias, and the k third of in_b without QK-norm, have a gradient of their own and are held to the bars too)
    rows = [(f"qk_norm[{name}]", qkl.grad[i], qr.grad[i]) for i, name in enumerate(("q_weight", "q_bias", "k_weight", "k_bias"))] if with_qk else []
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
@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_layer_with_rope_alone(ops, pre, geometry):
    _run_layer(ops, geometry, pre)
    _run_layer(ops, geometry, pre, kind="angles")


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_layer_with_rope_and_qk_norm(ops, pre, geometry):
    _run_layer(ops, geometry, pre, with_qk=True)


@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_layer_with_rope_and_a_relative_position_bias(ops, pre):
    _run_layer(ops, "D128_H2", pre, biased=True)
    _run_layer(ops, "D192_H4_padded", pre, biased=True, with_qk=True)


@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_layer_with_rope_and_a_curve_window(ops, pre):
    _run_layer(ops, "D128_H2", pre, masked=True, with_qk=True)
    _run_layer(ops, "D192_H4_padded", pre, masked=True)


@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_layer_with_rope_dropout_and_drop_path(ops, pre):
    _run_layer(ops, "D128_H2", pre, p=0.1, rate=0.5)
    _run_layer(ops, "D192_H4_padded", pre, p=0.1, rate=0.5, with_qk=True)


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_pre_norm_layer_with_rope_layer_scale_and_gelu(ops, geometry):
    _run_layer(ops, geometry, pre=True, act="gelu", with_lam=True)
    _run_layer(ops, geometry, pre=True, act="gelu", with_lam=True, p=0.1, rate=0.5, with_qk=True)


def test_public_layer_calls_reach_the_kernels(ops):
    """F.encoder_layer / F.pre_norm_layer with rope= run the RoPE kernels once per direction; the probes return the rotated q, k:
    what the attention kernels consumed."""
    import sfcvit.functional as F
    from test_parity_gpu import _store_point
    B, N, D, H = GEOMETRIES["D192_H4_padded"]
    hd, hp = D // H, 64
    rt = ops.RopeTable(_table(N, hd))
    for pre in (False, True):
        x, n, P, _, _, dy, dn = _params(B, N, D, H, pre)
        names = prenorm_ref.ORDER if pre else POST
        w = [P[k] for k in names]
        ops.KERNEL_LOG = []
        try:
            if pre:
                out = F.pre_norm_layer(x.clone().requires_grad_(True), n, *w, H, rope=rt)
                torch.autograd.backward(list(out), [dy, dn])
                probe = F.pre_norm_layer_probe(x, n, *w, H, rope=rt.table)           # a CPU table is taken too
                plain = F.pre_norm_layer_probe(x, n, *w, H)
                y, qkv, qkv0 = probe[1], probe[2], plain[2]
            else:
                out = (F.encoder_layer(x.clone().requires_grad_(True), *w, H, rope=rt),)
                out[0].backward(dy)
                y, qkv, _, _ = F.encoder_layer_probe(x, *w, H, rope=rt.table)
                qkv0 = F.encoder_layer_probe(x, *w, H)[1]
            log = list(ops.KERNEL_LOG)
        finally:
            ops.KERNEL_LOG = None
        assert log.count("rope_fwd_kernel<64>") == 2 and log.count("rope_bwd_kernel<64>") == 1, log
        assert torch.equal(bits(y), bits(out[-1].detach()))
        # the probe's q, k are the rotation of the unrotated probe's
        want = rope_ref.forward64(qkv0.view(B * N, -1), rt.on("cuda"), H, hd, hp)
        got = rope_ref.heads(qkv.view(B * N, -1), H, hp, 3)
        _store_point("probe q | k", got[:, :2], want[:, :2].float().to(BF16).float().cpu(), [], 1e-3)
        assert torch.equal(bits(got[:, 2]), bits(rope_ref.heads(qkv0.view(B * N, -1), H, hp, 3)[:, 2]))
        assert not torch.equal(bits(got[:, :2]), bits(rope_ref.heads(qkv0.view(B * N, -1), H, hp, 3)[:, :2]))


# ---- models --------------------------------------------------------------------------------------------------------------------
def _encoder_ref(model, t, probs=None):
    """The encoder of a post- or pre-norm model with RoPE (and QK-norm, if it has it) in fp32 on the CPU, on the weights of `model`."""
    f = lambda v: v.detach().float().cpu()                                         # noqa: E731
    enc, H = model.encoder, model.encoder.n_head
    if hasattr(enc, "cls_token"):
        t = torch.cat((f(enc.cls_token).expand(t.shape[0], 1, -1), t), 1)
    B, N, D = t.shape
    one, ones = torch.ones(()), torch.ones(B)
    rope = enc.rope.table
    qks = getattr(enc, "qk_norm", None)
    qk = lambda l: dict(qk_norm=f(qks[l]), qk_eps=enc.qk_norm_eps) if qks is not None else {}      # noqa: E731
    if not enc.norm_first:
        for l, L in enumerate(prenorm_ref.layers_of(_Layers(enc.transformer))[0]):
            Pd = {k: f(v) for k, v in L.items()}
            if probs is not None:
                probs.append(rope_ref.attention(t @ Pd["in_w"].t() + Pd["in_b"], H, rope, f(qks[l]) if qks is not None else None,
                                                enc.qk_norm_eps)[1])
            t = rope_ref.encoder_layer(t, Pd, H, (one, one, one, one), ones, ones, rope=rope, **qk(l))
        return t
    layers, final = prenorm_ref.layers_of(enc.transformer)
    s = t
    n = torch.nn.functional.layer_norm(s, (D,), f(layers[0]["n1_w"]), f(layers[0]["n1_b"]))
    scales = getattr(enc, "layer_scale", None)
    for l, L in enumerate(layers):
        nxt = (layers[l + 1]["n1_w"], layers[l + 1]["n1_b"]) if l + 1 < len(layers) else final
        Pf = {k_: f(v) for k_, v in dict(L, next_w=nxt[0], next_b=nxt[1]).items()}
        if probs is not None:
            probs.append(rope_ref.attention(n @ Pf["in_w"].t() + Pf["in_b"], H, rope, f(qks[l]) if qks is not None else None,
                                            enc.qk_norm_eps)[1])
        s, n = rope_ref.pre_norm_layer(s, n, Pf, H, lam=(f(scales[l][0]), f(scales[l][1])) if scales is not None else None,
                                       act=enc.activation, rope=rope, **qk(l))
    return n


@pytest.mark.parametrize("kw", [dict(rope="curve"), dict(rope="image", pool="cls"),
                                dict(rope="image", rope_base=20.0, qk_norm=True, norm_first=True, activation="gelu", layer_scale=0.5)],
                         ids=["curve", "image_cls", "image_qk_norm_pre_norm"])
def test_eval_logits_against_the_torch_reference(kw):
    from test_parity_gpu import LOGIT_TOL
    model, x, _, cfg = _tiny_model(**kw)
    _shake(model)
    model.eval()
    with torch.no_grad():
        got = model(x).float().cpu()
        t = model.mlp_mixer(model.patch_embed(x))
        want_tokens = _encoder_ref(model, t.float().cpu())
        want = model.mlp_head(want_tokens.to("cuda", dtype=BF16)).float().cpu()
        enc = model.encoder(t).float().cpu()
        off_kw = {k: v for k, v in kw.items() if not k.startswith("rope")}
        model_off, _, _, _ = _tiny_model(**off_kw)
        model_off.load_state_dict(model.state_dict())          # no key of its own: the checkpoint loads strictly
        off = model_off.eval()(x).float().cpu()
    scale = float(want.abs().max())
    err, tok_err = float((got - want).abs().max()), float((enc - want_tokens).abs().max() / want_tokens.abs().max())
    print(f"logits max err {err:.3e} of {scale:.3e}; encoder output max err {tok_err:.3e} of its largest value; "
          f"without rope the logits move by {float((got - off).abs().max()):.3e}")
    assert err <= LOGIT_TOL * scale and tok_err <= LOGIT_TOL
    assert float((got - off).abs().max()) > err, "the rotation changed nothing"


@pytest.mark.parametrize("kw", [dict(rope="curve"), dict(rope="curve", qk_norm=True)], ids=["rope", "rope_qk_norm"])
def test_training_steps_write_the_in_proj_bias_slot_whole(ops, kw):
    """Head dim 64: in_proj is not padded, its bias is a leaf with a slot in the flat gradient buffer.  With RoPE alone the RoPE
    backward writes the slot (q | k sums, v sums carried over); with QK-norm behind it, ops.qk_norm_bwd does."""
    import sfcvit.functional as F
    from sfcvit.training import FusedAdamW, train_step
    make = lambda: _tiny_model(**kw)[:3]                        # noqa: E731
    plain, x, tgt = make()
    plain.train()
    F.soft_target_cross_entropy(plain(x), tgt).backward()
    model, _, _ = make()
    model.train()
    opt = FusedAdamW(model.parameters(), lr=0.0, weight_decay=0.0)
    train_step(model, x, tgt, opt)                              # builds the flat buffers; from now on gradients go into slots
    opt.zero_grad()
    opt.flat_grad.fill_(float("nan"))                          # a slot that is not written whole keeps a NaN
    ops.KERNEL_LOG = []
    try:
        F.soft_target_cross_entropy(model(x), tgt).backward()
        log = list(ops.KERNEL_LOG)
    finally:
        ops.KERNEL_LOG = None
    torch.cuda.synchronize()
    depth = len(model.encoder.transformer.layers)
    assert sum(k.startswith("rope_fwd") for k in log) == depth and sum(k.startswith("rope_bwd") for k in log) == depth
    ref = dict(plain.named_parameters())
    seen = 0
    for k, prm in model.named_parameters():
        if "in_proj_bias" in k:
            buf, off = prm._sfcvit_slot
            assert buf is opt and prm.grad.data_ptr() == buf.flat_grad.data_ptr() + 2 * off, f"{k}: the gradient is not its slot"
            a, b = ref[k].grad.float(), prm.grad.float()
            D = a.numel() // 3
            for i, third in enumerate("qkv"):
                ai, bi = a[i * D:(i + 1) * D], b[i * D:(i + 1) * D]
                print(f"{k}[{third}]: max |slot - plain| {float((ai - bi).abs().max()):.3e} of {float(ai.abs().max()):.3e}")
                assert bool(torch.isfinite(bi).all()), f"{k}[{third}] was not written"
                assert float((ai - bi).abs().max()) <= 2.0 ** -7 * float(ai.abs().max()) + 1e-12, (k, third)
                assert float(bi.abs().max()) > 0, (k, third)
            seen += 1
    assert seen == depth


@pytest.mark.parametrize("kw", [dict(rope="curve"), dict(rope="image", qk_norm=True, norm_first=True, activation="gelu", layer_scale=0.5)],
                         ids=["post_norm", "pre_norm_qk_norm"])
def test_graphed_train_step_takes_the_eager_steps(kw):
    """Replays of the captured step equal eager steps three to five (two warm-up steps first), at dropout 0: the loss bit for bit,
    every parameter bytewise.  Nothing in the RoPE launches depends on the host."""
    from sfcvit import ops
    from sfcvit.training import FusedAdamW, GraphedTrainStep, train_step
    try:
        model_e, x, tgt, _ = _tiny_model(**kw)
        model_e.train()
        opt_e = FusedAdamW(model_e.parameters(), lr=1e-3, weight_decay=5e-2)
        opt_e.use_device_state(seed_base=4242)
        eager = [train_step(model_e, x, tgt, opt_e).float().cpu() for _ in range(5)]
        model_g, _, _, _ = _tiny_model(**kw)
        model_g.train()
        opt_g = FusedAdamW(model_g.parameters(), lr=1e-3, weight_decay=5e-2)
        opt_g.use_device_state(seed_base=4242)
        step = GraphedTrainStep(model_g, x.clone(), tgt.clone(), opt_g, warmup=2, preserve_state=False)
        graphed = [step().float().cpu() for _ in range(3)]
        print([float(v) for v in eager], [float(v) for v in graphed])
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(eager[2:], graphed))
        for (k, a), (_, b) in zip(model_e.state_dict().items(), model_g.state_dict().items()):
            assert torch.equal(bits(a) if a.dtype == BF16 else a, bits(b) if b.dtype == BF16 else b), k
        step.close()
    finally:
        ops.STEP_STATE = None


def _main_py(ckdir, *extra):
    main = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd", "main.py")
    return [sys.executable, main, "--synthetic", "--tokenizer", "hilbert", "--img-size", "32", "--patch-size", "16", "--embed-dim", "64",
            "--depth", "2", "--heads", "2", "--mlp-dim", "128", "--batch-size", "64", "--train-size", "256", "--test-size", "128",
            "--warmup-epochs", "0", "--qk-norm", "--checkpoint-dir", str(ckdir), *extra]


def _epoch_line(stdout, epoch):
    m = re.search(rf"Epoch {epoch}/\d+ \| Train Loss: (\S+), Train Acc: \S+ \| Test Loss: (\S+),", stdout)
    assert m, stdout[-1000:]
    return m.group(1), m.group(2)


def test_main_py_trains_and_resumes_with_the_same_table(tmp_path):
    """--rope image --qk-norm: one epoch, then the second epoch twice from the same checkpoint -- once with --rope on the command
    line, once without (the checkpoint names the kind and the base) -- gives the same losses: --resume rebuilt the same table."""
    first = tmp_path / "first"
    out = subprocess.run(_main_py(first, "--epochs", "1", "--rope", "image", "--rope-base", "30"), capture_output=True, text=True, timeout=300)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stderr[-3000:]
    assert "Epoch 1/1" in out.stdout, out.stdout[-1000:]
    ck = os.path.join(str(first), "checkpoint_hilbert.pt")
    saved = torch.load(ck, map_location="cpu", weights_only=True)
    assert saved["rope"] == {"kind": "image", "base": 30.0}
    assert not any("rope" in k for k in saved["model_state_dict"]) and "encoder.qk_norm.1" in saved["model_state_dict"]
    lines = []
    for tag, extra in (("given", ["--rope", "image", "--rope-base", "30"]), ("from_checkpoint", [])):
        d = tmp_path / tag
        d.mkdir()
        mine = shutil.copy(ck, str(d / "start.pt"))
        out = subprocess.run(_main_py(d, "--epochs", "2", "--resume", mine, *extra), capture_output=True, text=True, timeout=300)
        print(out.stdout[-600:])
        assert out.returncode == 0, out.stderr[-3000:]
        assert "Epoch 2/2" in out.stdout and "Epoch 1/2" not in out.stdout, out.stdout[-1000:]
        assert ("taken from the checkpoint" in out.stdout) == (tag == "from_checkpoint")
        lines.append(_epoch_line(out.stdout, 2))
    print(lines)
    assert lines[0] == lines[1], "the resumed runs disagree: the table was not rebuilt as it was"


def test_attention_report_sees_rotated_q_and_k():
    """The report's maps are those of the ROTATED q, k: they agree with the reference's softmax of the rotated scores within the
    bound below, and they do not agree with the softmax of the unrotated ones."""
    from sfcvit.analysis import attention_report, token_positions
    from test_attention_probe_gpu import TOL_F32, TOL_MODEL
    import qk_norm_ref
    model, x, _, cfg = _tiny_model(rope="curve", rope_base=5.0, qk_norm=True)
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
    # test_qk_norm_layers_gpu's bound with one more bf16 store per operand: the normalised q and k each carry 2 * 2^-9 (their own
    # store and the rounded projection), the rotation stores them once more (2^-9; a rotation keeps |q| and |k|), so a score
    # moves by at most 6 * 2^-9 * |q| |k| / sqrt(hd) =: delta and a probability by at most (e^(2 delta) - 1) of itself.
    for e, P in zip(rep["layers"], probs):
        qk = model.encoder.qk_norm[e["layer"]].detach().float().cpu()
        qmax = math.sqrt(hd) * (float(qk[0].abs().max()) + float(qk[1].abs().max()))
        kmax = math.sqrt(hd) * (float(qk[2].abs().max()) + float(qk[3].abs().max()))
        delta = 6 * 2.0 ** -9 * qmax * kmax / math.sqrt(hd)
        m = e["map"].float().cpu()
        assert tuple(m.shape) == (B, H, N, N) and e["mass_error"] <= TOL_F32
        assert float((m.sum(-1) - 1).abs().max()) <= 1e-3
        worst = float(((m - P).abs() / (P * math.expm1(2 * delta) + 1e-6)).max())
        fd = float((e["distance"].cpu() - (P * dmat).sum(-1).mean(-1)).abs().max()) / dscale
        fe = float((e["entropy"].cpu() + (P * torch.log(P.clamp_min(1e-30))).sum(-1).mean(-1)).abs().max()) / escale
        print(f"FIGURE rope model layer {e['layer']}: distance={fd:.3e} entropy={fe:.3e} mass={e['mass_error']:.3e} "
              f"map worst {worst:.3f} of its bound (delta {delta:.3f})")
        assert worst <= 1.0 and fd <= TOL_MODEL and fe <= TOL_MODEL, (worst, fd, fe)
    # layer 0 without the rotation, on the same weights: a different map
    enc = model.encoder
    L0 = prenorm_ref.layers_of(_Layers(enc.transformer))[0][0]
    qkv0 = t @ L0["in_w"].detach().float().cpu().t() + L0["in_b"].detach().float().cpu()
    unrot = qk_norm_ref.attention(qkv0, H, enc.qk_norm[0].detach().float().cpu(), enc.qk_norm_eps)[1]
    m0 = rep["layers"][0]["map"].float().cpu()
    assert float((m0 - unrot).abs().max()) > 10 * float((m0 - probs[0]).abs().max()), "the report saw unrotated q and k"
