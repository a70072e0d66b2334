"""Device-side MixUp / CutMix on the GPU: the mixing gather and the one-pass image mixer against stock torch (exact), the
label-pair loss against an fp64 oracle, whole training steps, the epoch loop, the graphed step and main.py --device-mix."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.cases import MODEL_CASES
from test_host_cpu import build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- cases ------------------------------------------------------------------------------------------------------------
def _perms(B):
    """identity (all fixed points), one cycle through everything, a 3-cycle + fixed points, a seeded shuffle."""
    g = torch.Generator().manual_seed(B)
    out = [torch.arange(B), torch.roll(torch.arange(B), 1), torch.randperm(B, generator=g)]
    p = torch.arange(B)
    p[:3] = torch.tensor([1, 2, 0])
    return out + [p]


def _mix_cases(S):
    """(kind, lam or box) for an S x S image: lam of 1.0, beta(0.2, 0.2)-like draws next to 0 and 1, a middling one; boxes
    (bbx1, bby1, bbx2, bby2) that are empty, cover the image, touch each edge, and cut through 16 x 16 tiles."""
    return [("none", None), ("mixup", 1.0), ("mixup", 3.1e-5), ("mixup", 0.99996), ("mixup", 0.3717),
            ("cutmix", (5, 5, 5, 9)), ("cutmix", (0, 0, S, S)), ("cutmix", (0, 3, S // 3, S // 2 + 3)),
            ("cutmix", (max(0, S - 21), max(0, S - 9), S, S)), ("cutmix", (7, 0, 12, S)), ("cutmix", (0, max(0, S - 5), S, S)),
            ("cutmix", (7, 19, min(S, 57), min(S, 52))), ("cutmix", (17, 1, 18, 2))]


def _set(bm, case, idx, S):
    kind, arg = case
    idx = idx.to(bm.device)
    if kind == "none":
        bm.set_none()
        bm.perm.copy_(idx)                      # whatever the permutation holds, mode 0 ignores it
        bm.idx = idx
    elif kind == "mixup":
        bm.set_mixup(arg, idx)
    else:
        bm.set_cutmix(arg, idx, S, S)
    return bm


def _tables(tok):
    pix = tok._pix_table(torch.device("cuda"))
    return pix, tok._desc, tok._order


# ---- 5. the gather, exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,img,patch,path", [("HilbertEmbedding1D", 224, 256, "tiles"), ("MortonEmbedding1D", 224, 256, "tiles"),
                                                ("RasterScan1DEmbedding", 224, 256, "strips"),
                                                ("HilbertEmbedding1D", 32, 16, "pixel"), ("HilbertEmbedding1D", 32, 64, "pixel"),
                                                ("MortonEmbedding1D", 32, 512, "generic")])
def test_mixing_gather_equals_the_gather_of_the_torch_mixed_batch(cls, img, patch, path):
    import sfcvit.tokenizers as T
    from sfcvit import ops
    from sfcvit.training import BatchMix
    tok = getattr(T, cls)(img, patch, 3, 64).to("cuda")
    pix, desc, order = _tables(tok)
    if path == "tiles":
        assert desc is not None and desc.mode == 1                   # the 16 x 16-tile kernel is what runs
    torch.manual_seed(img + patch)
    n = 0
    for B in (5, 9, 8):
        x = torch.randn(B, 3, img, img, device="cuda")
        bm = BatchMix(B, "cuda")
        plain = ops.gather_tokens(x, pix, desc, order)
        for pi, idx in enumerate(_perms(B)):
            for case in _mix_cases(img):
                if B != 5 and pi not in (1, 2) and case[0] != "none":
                    continue                                         # the full cross product at one batch size is enough
                _set(bm, case, idx, img)
                mixed = bm.apply_torch(x)
                got = ops.gather_tokens(x, pix, desc, order, mix=bm)
                assert torch.equal(got, ops.gather_tokens(mixed, pix, desc, order)), (B, idx.tolist(), case)
                if case[0] == "none" or case == ("mixup", 1.0) or case == ("cutmix", (5, 5, 5, 9)):
                    assert torch.equal(got, plain), (B, case)        # mode 0 (and the do-nothing mixes) = the unmixed gather
                n += 1
    assert n > 60
    with pytest.raises(TypeError, match="fp32"):
        ops.gather_tokens(x.to(torch.bfloat16), pix, desc, order, mix=bm)
    with pytest.raises(ValueError, match="batch"):
        ops.gather_tokens(x, pix, desc, order, mix=BatchMix(3, "cuda"))


def test_partner_outside_the_batch_reads_nothing_outside_it():
    """perm entries outside [0, B) mean "no partner" (include/sfcvit.h): the image itself, in every kernel."""
    import sfcvit.tokenizers as T
    from sfcvit import ops
    from sfcvit.training import BatchMix
    for img, patch in ((224, 256), (32, 16)):
        tok = T.HilbertEmbedding1D(img, patch, 3, 64).to("cuda")
        pix, desc, order = _tables(tok)
        x = torch.randn(4, 3, img, img, device="cuda")
        bm = BatchMix(4, "cuda")
        bm.set_cutmix((0, 0, img, img), torch.tensor([1, 0, 3, 2], device="cuda"), img, img)
        bm.perm.copy_(torch.tensor([1, -1, 4, 2 ** 31 - 1], dtype=torch.int32))
        want = x.clone()
        want[0] = x[1]
        assert torch.equal(ops.gather_tokens(x, pix, desc, order, mix=bm), ops.gather_tokens(want, pix, desc, order))
        assert torch.equal(ops.mix_images(x, bm), want)


# ---- 6. the image mixer and the tokenizers behind it ------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3, 224, 224), (9, 3, 32, 32), (3, 2, 7, 9), (4, 1, 6, 10)])
def test_mix_images_equals_torch(shape):
    from sfcvit import ops
    from sfcvit.training import BatchMix
    B, C, H, W = shape
    torch.manual_seed(H)
    x = torch.randn(shape, device="cuda")
    bm = BatchMix(B, "cuda")
    S = min(H, W)
    for idx in _perms(B):
        for case in _mix_cases(S):
            if case[0] == "cutmix":
                bm.set_cutmix(case[1], idx.cuda(), H, W)
            else:
                _set(bm, case, idx, S)
            keep = x.clone()
            got = ops.mix_images(x, bm)
            assert torch.equal(got, bm.apply_torch(x)), (shape, idx.tolist(), case)
            assert torch.equal(x, keep) and got.data_ptr() != x.data_ptr()
    bm.set_cutmix((2, 1, H + 40, W + 40), _perms(B)[1].cuda(), H, W)    # a box that overhangs: clamped like torch's slices
    assert torch.equal(ops.mix_images(x, bm), bm.apply_torch(x))


def _families():
    import sfcvit.tokenizers as T
    from sfcvit.models.altvit import HilbertViT, SimpleViT
    return {
        "fused_small_patch_embed": lambda: T.HilbertEmbedding1D(32, 16, 3, 64),
        "hierarchical": lambda: T.HierarchicalMortonEmbedding(32, 3, [16, 4, 1], 256),
        "conv2d_zigzag": lambda: T.ZigzagEmbedding(32, 4, 3, 64),
        "conv2d_hilbert": lambda: T.HilbertEmbedding(32, 4, 3, 64),
        "altvit_simple": lambda: SimpleViT(image_size=32, patch_size=4, num_classes=10, dim=64, depth=1, heads=1, mlp_dim=128),
        "altvit_hilbert": lambda: HilbertViT(image_size=32, patch_size=4, num_classes=10, dim=64, depth=1, heads=1, mlp_dim=128),
    }


@pytest.mark.parametrize("family", sorted(_families()))
def test_tokenizers_without_a_gather_mix_through_mix_images(family, monkeypatch):
    from sfcvit import ops
    from sfcvit.training import BatchMix
    torch.manual_seed(3)
    model = _families()[family]().to("cuda", dtype=torch.bfloat16).eval()
    x = torch.randn(6, 3, 32, 32, device="cuda")
    bm = BatchMix(6, "cuda")
    calls = []
    real = ops.mix_images
    monkeypatch.setattr(ops, "mix_images", lambda *a: (calls.append(1), real(*a))[1])
    with torch.no_grad():
        for case in (("mixup", 0.3717), ("cutmix", (7, 3, 25, 30)), ("none", None)):
            _set(bm, case, _perms(6)[2], 32)
            n0 = len(calls)
            got = model(x, mix=bm)                                   # eval mode: a mix that is given is applied
            assert len(calls) == n0 + 1
            assert torch.equal(got, model(bm.apply_torch(x))), (family, case)
        assert torch.equal(model(x, mix=None), model(x)) and len(calls) == n0 + 1


# ---- 7. the label-pair loss -------------------------------------------------------------------------------------------
def _ordered(bf16):
    """bf16 tensor -> int32 keys in which neighbouring representable values differ by one (+0 and -0 coincide)."""
    b = bf16.view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


@pytest.mark.parametrize("C,ld", [(10, 10), (100, 100), (1000, 1000), (77, 77), (77, 80)])
@pytest.mark.parametrize("lam", [1.0, 0.3717, 3.1e-5, 0.99996])
def test_pair_loss_against_an_fp64_oracle(C, ld, lam):
    """Oracle: log-softmax of the bf16 logits in double on the CPU with the fp32 dense targets the loop builds.
    dlogits: the correctly rounded bf16 of the oracle or its neighbour.  loss_rows: the largest error over the rows may be
    at most twice the largest error of ops.soft_ce on dense_targets of the same rows (the two kernels share the lse loop and
    differ in a 2-term against a C-term sum) plus one fp32 ulp of max(|lse| + max|z|).  hit_rows exact."""
    from sfcvit import ops
    from sfcvit.training import BatchMix
    B = 37
    g = torch.Generator().manual_seed(C * 7 + ld)
    z = (torch.randn(B, ld, generator=g) * 3).clamp(-12, 12)
    top = torch.randint(0, C, (B,), generator=g)
    z[torch.arange(B), top] = 14.0 + torch.arange(B) % 3             # every row's maximum is unique
    logits = z.to(torch.bfloat16).cuda()
    y_a = torch.randint(0, C, (B,), generator=g)
    y_b = torch.randint(0, C, (B,), generator=g)
    y_b[::5] = y_a[::5]                                              # rows with y_a == y_b
    y_a[1::4] = top[1::4]                                            # hits on y_a, on y_b, on both, on neither
    y_b[2::4] = top[2::4]
    bm = BatchMix(B, "cuda")
    bm.set_mixup(lam, torch.randperm(B, generator=g).cuda())
    dense = bm.dense_targets(y_a, y_b, C)                            # fp32, CPU
    gscale = 1.0 / B
    rows, dl, hits = ops.soft_ce_pair(logits, y_a.cuda(), y_b.cuda(), bm, C, gscale)
    rows_d, dl_d = ops.soft_ce(logits, dense.cuda(), C, gscale)
    torch.cuda.synchronize()
    z64 = logits[:, :C].double().cpu()
    t64 = dense.double()
    lsm = torch.log_softmax(z64, dim=-1)
    loss64 = -(t64 * lsm).sum(-1)
    dl64 = (lsm.exp() * t64.sum(-1, keepdim=True) - t64) * gscale
    # hit_rows: what the loop computes from argmax
    preds = logits[:, :C].float().cpu().argmax(dim=1)
    assert torch.equal(preds, top)
    want_hits = lam * (preds == y_a).float() + (1 - lam) * (preds == y_b).float()
    assert torch.equal(hits.cpu(), want_hits)
    # dlogits
    ref_bf = dl64.to(torch.float32).to(torch.bfloat16)
    steps = (_ordered(dl[:, :C].cpu()) - _ordered(ref_bf)).abs()
    assert int(steps.max()) <= 1, int(steps.max())
    assert not dl[:, C:].any()                                       # padding columns are written 0
    # loss_rows
    err_pair = float((rows.cpu().double() - loss64).abs().max())
    err_dense = float((rows_d.cpu().double() - loss64).abs().max())
    lse = torch.logsumexp(z64, dim=-1)
    ulp = float(np.spacing(np.float32(float((lse.abs() + z64.abs().max(dim=-1).values).max()))))
    print(f"pair loss C={C} ld={ld} lam={lam}: max error {err_pair:.3e} (pair) {err_dense:.3e} (dense soft_ce), ulp {ulp:.3e}; "
          f"dlogits within {int(steps.max())} bf16 step(s)")
    assert err_pair <= 2 * err_dense + ulp, (err_pair, err_dense, ulp)
    # mode 0 is lam = 1
    bm.set_none()
    rows0, dl0, hits0 = ops.soft_ce_pair(logits, y_a.cuda(), y_b.cuda(), bm, C, gscale)
    bm.set_mixup(1.0, bm.idx)
    rows1, dl1, hits1 = ops.soft_ce_pair(logits, y_a.cuda(), y_b.cuda(), bm, C, gscale)
    assert torch.equal(rows0, rows1) and torch.equal(dl0, dl1) and torch.equal(hits0, hits1)


def test_pair_loss_with_labels_out_of_range():
    """A label outside [0, C) is a label without a target (include/sfcvit.h): nothing is read or written through it and
    the neighbouring rows do not change."""
    from sfcvit import ops
    from sfcvit.training import BatchMix
    B, C = 12, 10
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(B, C, generator=g).to(torch.bfloat16).cuda()
    y_a, y_b = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    bm = BatchMix(B, "cuda")
    bm.set_mixup(0.3, torch.arange(B).cuda())
    guard = torch.full((3, B), 7.0, device="cuda")                   # loss_rows / hit_rows sit in torch's pool between other tensors
    base = ops.soft_ce_pair(logits, y_a.cuda(), y_b.cuda(), bm, C, 1.0)
    bad_a, bad_b = y_a.clone(), y_b.clone()
    bad_a[1], bad_b[1] = -1, y_b[1]
    bad_a[4], bad_b[4] = y_a[4], C
    bad_a[7], bad_b[7] = 2 ** 40, -(2 ** 40)
    bad_a[9], bad_b[9] = C + 5, C + 5
    got = ops.soft_ce_pair(logits, bad_a.cuda(), bad_b.cuda(), bm, C, 1.0)
    torch.cuda.synchronize()
    ok = torch.ones(B, dtype=torch.bool)
    ok[[1, 4, 7, 9]] = False
    for a, b in zip(base, got):
        assert torch.equal(a[ok.cuda()], b[ok.cuda()])
        assert torch.isfinite(b.float()).all()
    rows, dl, hits = (t.cpu() for t in got)
    z = logits.double().cpu()
    lsm = torch.log_softmax(z, dim=-1)
    lam32, oml32 = float(np.float32(0.3)), float(np.float32(1.0 - 0.3))
    assert float(rows[1]) == pytest.approx(-oml32 * float(lsm[1, y_b[1]]), rel=1e-5, abs=1e-6)      # only y_b has a target
    assert float(rows[4]) == pytest.approx(-lam32 * float(lsm[4, y_a[4]]), rel=1e-5, abs=1e-6)      # only y_a
    assert float(rows[7]) == 0.0 and float(rows[9]) == 0.0 and not dl[7].any() and not dl[9].any()  # no target at all
    assert float(hits[7]) == 0.0 and float(hits[9]) == 0.0
    assert bool((guard == 7.0).all())


# ---- 8. whole model, exact ----------------------------------------------------------------------------------------------
def _vit(kind):
    from sfcvit.models import VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    if kind == "tiny32":                                             # ViT-Tiny-size Hilbert model on 32 px (per-pixel gather)
        pe = HilbertEmbedding1D(32, 16, 3, 192)
        return VisionTransformer1D(pe, depth=2, n_heads=3, mlp_dim=768, num_classes=10, dropout_p=0.0, head_dropout_p=0.0), 32, 8
    pe = HilbertEmbedding1D(224, 256, 3, 768)                        # ViT-B geometry at small depth (16 x 16-tile gather)
    return VisionTransformer1D(pe, depth=1, n_heads=12, mlp_dim=1024, num_classes=10, dropout_p=0.0, head_dropout_p=0.0), 224, 20


def _no_mix_images(*a):
    raise AssertionError("the batch was mixed outside the gather")


@pytest.mark.parametrize("kind", ["tiny32", "vitb224"])
def test_three_steps_with_the_mix_in_the_gather_equal_three_steps_on_torch_mixed_images(kind, monkeypatch):
    import sfcvit.functional as F
    from sfcvit import _lib, ops
    from sfcvit.training import BatchMix, FusedAdamW
    # the gather + GEMM form of patch_embed at both sizes (by default a launch-bound size takes the fused kernels, which mix
    # through mix_images: covered above)
    monkeypatch.setattr(F, "pe_two_stage", lambda x, pix, D: True)
    torch.manual_seed(17)
    proto, img, B = _vit(kind)
    state = {k: v.clone() for k, v in proto.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(B, 3, img, img, generator=g).cuda() for _ in range(3)]
    ys = [torch.randint(0, 10, (B,), generator=g).cuda() for _ in range(3)]

    def run(fused):
        model, _, _ = _vit(kind)
        model.load_state_dict(state)
        model = model.to("cuda", dtype=torch.bfloat16).train()
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2)
        bm = BatchMix(B, "cuda")
        np.random.seed(23)
        torch.manual_seed(23)
        calls = []
        losses = []
        with monkeypatch.context() as mp:
            if fused:
                real = _lib.lib.sfcvit_tokens_gather_mix
                mp.setattr(ops, "mix_images", _no_mix_images)
                mp.setattr(_lib.lib, "sfcvit_tokens_gather_mix", lambda *a: (calls.append(1), real(*a))[1])
            for step, (x, y) in enumerate(zip(xs, ys)):
                if step == 0:
                    bm.set_mixup(0.3717, torch.randperm(B, device="cuda"))
                elif step == 1:
                    bm.set_cutmix((7, 19, 7 + img // 2, 19 + img // 3), torch.randperm(B, device="cuda"), img, img)
                else:
                    bm.draw(img, img)
                y_a, y_b = y, y[bm.idx]
                opt.zero_grad()
                logits = model(x, mix=bm) if fused else model(bm.apply_torch(x))
                loss = F.soft_target_cross_entropy(logits, bm.dense_targets(y_a, y_b, 10))
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
        return losses, opt.master.clone(), len(calls)

    l_f, w_f, n_f = run(True)
    l_t, w_t, _ = run(False)
    assert n_f == 3                                                  # one mixing gather per forward, nothing else mixed
    assert l_f == l_t and torch.equal(w_f, w_t)
    assert l_f[0] == l_f[0] and not torch.equal(w_f, torch.zeros_like(w_f))


# ---- 9. the epoch loop --------------------------------------------------------------------------------------------------
def test_epoch_with_device_mix_draws_and_trains_like_the_default_loop(monkeypatch):
    from sfcvit.training import FusedAdamW, SoftTargetCrossEntropy
    from sfcvit.training.loops import train_with_mixup_or_cutmix
    from test_parity_gpu import load_formula
    cfg, _ = MODEL_CASES["hilbert32_1d"]
    g = torch.Generator().manual_seed(0)
    batches = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, cfg.num_classes, (8,), generator=g)) for _ in range(4)]

    class Loader(list):
        dataset = range(32)

    trace = []
    for mod, name in ((np.random, "rand"), (np.random, "beta"), (np.random, "randint"), (torch, "randperm")):
        real = getattr(mod, name)

        def rec(*a, _real=real, _name=name, **kw):
            out = _real(*a, **kw)
            trace.append((_name, out.tolist() if hasattr(out, "tolist") else out))
            return out
        monkeypatch.setattr(mod, name, rec)

    def epoch(device_mix):
        m = build_model(cfg)
        load_formula(m, cfg)
        m = m.to("cuda", dtype=torch.bfloat16).train()
        o = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=5e-5)
        torch.manual_seed(11)
        np.random.seed(11)
        del trace[:]
        out = train_with_mixup_or_cutmix(m, Loader(batches), SoftTargetCrossEntropy(), o, None, "cuda", device_mix=device_mix)
        return out, list(trace)

    (l0, a0), t0 = epoch(False)
    (l1, a1), t1 = epoch(True)
    assert t0 == t1 and len([t for t in t0 if t[0] == "randperm"]) == 4
    assert {"beta", "rand"} <= {t[0] for t in t0}
    print(f"epoch loss / accuracy: default {l0:.6f} / {a0:.6f}, device_mix {l1:.6f} / {a1:.6f}")
    assert abs(l1 - l0) <= 2e-3 * abs(l0) + 2e-3
    assert abs(a1 - a0) <= 2e-3 * abs(a0) + 2e-3


# ---- 10. the graphed step -----------------------------------------------------------------------------------------------
def test_graphed_step_with_a_mix_replays_the_eager_device_mix_steps_bit_for_bit():
    import sfcvit.functional as F
    from sfcvit import ops
    from sfcvit.training import BatchMix, FusedAdamW, GraphedTrainStep
    from test_parity_gpu import load_formula
    cfg, _ = MODEL_CASES["hilbert32_1d"]
    g = torch.Generator().manual_seed(0)
    B = 8
    batches = [(torch.randn(B, 3, 32, 32, generator=g).cuda(), torch.randint(0, cfg.num_classes, (B,), generator=g).cuda())
               for _ in range(4)]

    def fresh():
        m = build_model(cfg)
        load_formula(m, cfg)
        m = m.to("cuda", dtype=torch.bfloat16).train()               # dropout 0.1 / 0.5 on
        o = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=5e-2)
        o.use_device_state(torch.device("cuda"), seed_base=77)
        return m, o

    def seed():
        torch.manual_seed(5)
        np.random.seed(5)

    try:
        m_e, o_e = fresh()
        bm = BatchMix(B, "cuda")
        seed()
        eager = []
        for x, y in batches:
            bm.draw(32, 32)
            o_e.begin_step()
            o_e.zero_grad()
            loss, hits = F.mixed_target_cross_entropy(m_e(x, mix=bm), y, y[bm.idx], bm)
            loss.backward()
            o_e.step()
            eager.append((float(loss.detach()), hits.clone(), bm.mode, bm.lam))
        m_g, o_g = fresh()
        before = [p.detach().clone() for p in m_g.parameters()]
        labels = (torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda"))
        gs = GraphedTrainStep(m_g, torch.zeros(B, 3, 32, 32, device="cuda"), None, o_g, mix=BatchMix(B, "cuda"), labels=labels)
        assert all(torch.equal(a, b) for a, b in zip(before, m_g.parameters()))
        assert o_g.step_count == 0 and int(o_g.dev_state[1]) == 0 and not o_g.m.any() and not o_g.v.any()
        seed()
        graphed = []
        for x, y in batches:
            gs.mix.draw(32, 32)
            gs.images.copy_(x)
            gs.labels[0].copy_(y)
            gs.labels[1].copy_(y[gs.mix.idx])
            graphed.append((float(gs()), gs.hits.clone(), gs.mix.mode, gs.mix.lam))
        assert {e[2] for e in eager} == {1, 2}                       # both kinds of mix went through the one captured graph
        for e, r in zip(eager, graphed):
            assert e[0] == r[0] and torch.equal(e[1], r[1]) and e[2:] == r[2:], (e, r)
        assert torch.equal(o_e.master, o_g.master) and torch.equal(o_e.m, o_g.m) and torch.equal(o_e.v, o_g.v)
        assert o_g.step_count == 4 and int(o_g.dev_state[1]) == 4
        gs.close()
        with pytest.raises(ValueError):
            GraphedTrainStep(m_g, torch.zeros(B, 3, 32, 32, device="cuda"), None, o_g)
    finally:
        ops.STEP_STATE = None


# ---- 11. main.py --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_main_py_trains_with_device_mix(graph, tmp_path):
    """`main.py --synthetic --device-mix` (and with --graph): finishes and the training loss falls.  Three short epochs
    instead of one, so that there is a loss to fall from."""
    import re
    cmd = [sys.executable, os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd", "main.py"), "--synthetic",
           "--device-mix", "--epochs", "3", "--warmup-epochs", "1", "--train-size", "4096", "--test-size", "512", "--batch-size", "256",
           "--lr", "1e-3", "--checkpoint-dir", str(tmp_path)] + (["--graph"] if graph else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"Train Loss: ([0-9.]+)", out.stdout)]
    print(out.stdout[-600:])
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
