"""Device-side MixUp / CutMix, the parts that need no GPU: BatchMix's draws against the reference fixture
(tests/golden/mix.json, mix_batches.npz; tools/make_golden_mix.py) and against the existing loop helpers, the mix
semantics stated in numpy, the dense targets, and the argument checks of the three entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle import formula


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "mix.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(golden_dir, "mix_batches.npz"))


def _draw(seed, B, H, W, device="cpu"):
    from sfcvit.training import BatchMix
    np.random.seed(seed)
    torch.manual_seed(seed)
    return BatchMix(B, device).draw(H, W)


def numpy_mix(x, mode, lam, idx, rows, cols):
    """The mix semantics of include/sfcvit.h on a float32 array [B, C, H, W]: MixUp = two products and a sum, each
    rounded to fp32; CutMix = the partner's pixels inside [r0, r1) x [c0, c1) on dims 2 and 3, read from the un-mixed batch."""
    x = np.asarray(x, dtype=np.float32)
    if mode == 1:
        l32, o32 = np.float32(lam), np.float32(1.0 - lam)            # 1 - lam in double, rounded once
        return (l32 * x).astype(np.float32) + (o32 * x[idx]).astype(np.float32)
    out = x.copy()
    if mode == 2:
        out[:, :, rows[0]:rows[1], cols[0]:cols[1]] = x[idx][:, :, rows[0]:rows[1], cols[0]:cols[1]]
    return out


def test_draw_matches_the_reference_fixture(golden):
    meta, _ = golden
    B, _, H, W = meta["shape"]
    labels = torch.tensor(meta["labels"])
    kinds = set()
    for d in meta["draws"]:
        bm = _draw(d["seed"], B, H, W)
        kinds.add(d["kind"])
        assert bm.mode == {"mixup": 1, "cutmix": 2}[d["kind"]], d
        assert bm.idx.tolist() == d["idx"], d
        assert bm.perm.tolist() == d["idx"] and bm.perm.dtype == torch.int32
        assert bm.lam == d["lam"], d                                 # exact: the same double
        assert labels[bm.idx].tolist() == d["y_b"]
        rec = bm.rec.numpy()
        assert rec[0] == bm.mode and rec[7] == 0
        assert rec[5:7].view(np.float32).tolist() == [np.float32(d["lam"]), np.float32(1.0 - d["lam"])]
        if d["kind"] == "cutmix":
            assert list(bm.box) == d["box"], d
            bbx1, bby1, bbx2, bby2 = d["box"]
            assert rec[1:5].tolist() == [bbx1, bbx2, bby1, bby2]     # bbx on dim 2 (rows), bby on dim 3 (columns)
            assert d["lam"] == 1 - ((bbx2 - bbx1) * (bby2 - bby1) / (H * W))
    assert kinds == {"mixup", "cutmix"}


@pytest.mark.parametrize("seed", range(100, 124))
def test_draw_matches_the_loop_helpers(seed):
    """Same seeds, same consumption of np.random and torch's generator as train_with_mixup_or_cutmix."""
    from sfcvit.training import loops
    B, H, W = 6, 32, 32
    x0 = formula.image_batch(B, 3, H, W)
    y = torch.arange(B) % 4
    bm = _draw(seed, B, H, W)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if np.random.rand() < 0.5:
        mixed, y_a, y_b, lam = loops.mixup_data(x0.clone(), y, alpha=0.2)
        assert bm.mode == 1
    else:
        mixed, y_a, y_b, lam = loops.cutmix_data(x0.clone(), y, alpha=1.0)
        assert bm.mode == 2
    assert bm.lam == lam and torch.equal(y[bm.idx], y_b)
    assert torch.equal(bm.apply_torch(x0), mixed)
    rec = bm.rec.numpy()
    got = numpy_mix(x0.numpy(), int(rec[0]), bm.lam, bm.idx.numpy(), rec[1:3], rec[3:5])
    assert np.array_equal(got.view(np.int32), mixed.numpy().view(np.int32))
    # the generators are left where the loop leaves them
    a, b = np.random.rand(), torch.rand(1)
    _draw(seed, B, H, W)
    assert np.random.rand() == a and torch.equal(torch.rand(1), b)


def test_numpy_semantics_reproduce_the_fixture_batches_bit_for_bit(golden):
    meta, arrays = golden
    B, C, H, W = meta["shape"]
    x0 = formula.image_batch(B, C, H, W).numpy()
    for kind, seed in meta["mixed"].items():
        d = next(d for d in meta["draws"] if d["seed"] == seed)
        bm = _draw(seed, B, H, W)
        rec = bm.rec.numpy()
        got = numpy_mix(x0, int(rec[0]), bm.lam, np.array(d["idx"]), rec[1:3], rec[3:5])
        assert np.array_equal(got.view(np.int32), arrays[kind]), kind
    # separate rounding is what is pinned: a fused multiply-add of the same MixUp differs somewhere
    d = next(d for d in meta["draws"] if d["seed"] == meta["mixed"]["mixup"])
    l64, o64 = float(np.float32(d["lam"])), float(np.float32(1.0 - d["lam"]))
    x64 = x0.astype(np.float64)
    fused = ((l64 * x64).astype(np.float32).astype(np.float64) + o64 * x64[d["idx"]]).astype(np.float32)
    assert not np.array_equal(fused.view(np.int32), arrays["mixup"])
    # and the dim-2 / dim-3 quirk: the box applied the other way round is another batch (the fixture's box is not square-symmetric)
    d = next(d for d in meta["draws"] if d["seed"] == meta["mixed"]["cutmix"])
    bbx1, bby1, bbx2, bby2 = d["box"]
    swapped = numpy_mix(x0, 2, d["lam"], np.array(d["idx"]), (bby1, bby2), (bbx1, bbx2))
    assert not np.array_equal(swapped.view(np.int32), arrays["cutmix"])


def test_fixture_loss_and_dense_targets(golden):
    meta, _ = golden
    B, _, H, W = meta["shape"]
    labels, logits = torch.tensor(meta["labels"]), torch.tensor(meta["logits"])
    C = logits.shape[1]
    for d in meta["draws"]:
        bm = _draw(d["seed"], B, H, W)
        y_a, y_b = labels, labels[bm.idx]
        tgt = bm.dense_targets(y_a, y_b, C)
        loop = bm.lam * TF.one_hot(y_a, C).float() + (1 - bm.lam) * TF.one_hot(y_b, C).float()     # loops.py, train.py:160
        assert tgt.dtype == torch.float32 and torch.equal(tgt, loop)
        loss = float(torch.sum(-tgt * torch.log_softmax(logits, dim=-1), dim=-1).mean())
        assert loss == pytest.approx(d["loss"], rel=1e-6, abs=1e-7)
        same = (y_a == y_b)
        if same.any():                                               # where the labels coincide the row holds fadd(lam, 1 - lam)
            want = np.float32(np.float32(bm.lam) + np.float32(1.0 - bm.lam))
            assert all(float(tgt[int(b), int(y_a[b])]) == float(want) for b in torch.nonzero(same).flatten())
    assert any((labels == labels[torch.tensor(d["idx"])]).any() for d in meta["draws"])


def test_set_none_and_clamped_box():
    from sfcvit.training import BatchMix
    bm = BatchMix(3, "cpu")
    assert bm.rec.tolist() == [0] * 8 and bm.perm.tolist() == [0, 1, 2] and bm.mode == 0 and bm.lam == 1.0
    bm.set_cutmix((5, 30, 40, 70), torch.tensor([2, 0, 1]), 32, 64)          # slices clamp as torch's do
    assert bm.rec.tolist()[:5] == [2, 5, 32, 30, 64] and bm.box == (5, 30, 40, 70)
    assert bm.lam == 1 - (35 * 40 / (32 * 64))
    bm.set_none()
    assert bm.rec.tolist()[0] == 0 and bm.rec[5:7].numpy().view(np.float32).tolist() == [1.0, 0.0]
    with pytest.raises(ValueError):
        bm.set_mixup(0.5, torch.tensor([0, 1]))


def test_argument_checks_of_the_mix_entry_points_run_without_a_gpu():
    from sfcvit import _lib
    lib = _lib.lib
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)
    q = ctypes.c_void_p(base + 2048)

    def err():
        return lib.sfcvit_last_error().decode()

    # sfcvit_mix_images(x, perm, rec, out, B, C, H, W, stream)
    assert lib.sfcvit_mix_images(None, p, p, q, 1, 1, 4, 4, None) == 1 and "null" in err()
    assert lib.sfcvit_mix_images(p, None, p, q, 1, 1, 4, 4, None) == 1 and "null" in err()
    assert lib.sfcvit_mix_images(p, p, None, q, 1, 1, 4, 4, None) == 1 and "null" in err()
    assert lib.sfcvit_mix_images(p, p, p, None, 1, 1, 4, 4, None) == 1 and "null" in err()
    assert lib.sfcvit_mix_images(p, p, p, q, 0, 1, 4, 4, None) == 1 and "B=0" in err()
    assert lib.sfcvit_mix_images(p, p, p, q, 1, 1, 0, 4, None) == 1
    assert lib.sfcvit_mix_images(p, p, p, p, 1, 1, 4, 4, None) == 1 and "alias" in err()
    assert lib.sfcvit_mix_images(p, p, p, ctypes.c_void_p(base + 32), 1, 1, 4, 4, None) == 1 and "alias" in err()   # overlap
    assert lib.sfcvit_mix_images(p, p, p, ctypes.c_void_p(base + 2052), 1, 1, 4, 4, None) == 1 and "aligned" in err()
    # sfcvit_soft_ce_pair(logits, y_a, y_b, rec, loss_rows, dlogits, hit_rows, B, C, ld, gscale, stream)
    assert lib.sfcvit_soft_ce_pair(None, p, p, p, p, p, p, 1, 10, 16, 1.0, None) == 1 and "null" in err()
    assert lib.sfcvit_soft_ce_pair(p, None, p, p, p, p, p, 1, 10, 16, 1.0, None) == 1 and "null" in err()
    assert lib.sfcvit_soft_ce_pair(p, p, p, None, p, p, p, 1, 10, 16, 1.0, None) == 1 and "null" in err()
    assert lib.sfcvit_soft_ce_pair(p, p, p, p, None, p, p, 1, 10, 16, 1.0, None) == 1 and "null" in err()
    assert lib.sfcvit_soft_ce_pair(p, p, p, p, p, p, p, 0, 10, 16, 1.0, None) == 1 and "B=0" in err()
    assert lib.sfcvit_soft_ce_pair(p, p, p, p, p, p, p, 1, 10, 8, 1.0, None) == 1 and "ld=8" in err()
    # sfcvit_tokens_gather_mix(x, pix, order, origin, perm, rec, B, C, H, W, N, P, tokens, ld, stream)
    g = lib.sfcvit_tokens_gather_mix
    assert g(p, p, None, None, None, p, 1, 3, 32, 32, 64, 16, q, 48, None) == 1 and "perm" in err()
    assert g(p, p, None, None, p, None, 1, 3, 32, 32, 64, 16, q, 48, None) == 1 and "rec" in err()
    assert g(None, p, None, None, p, p, 1, 3, 32, 32, 64, 16, q, 48, None) == 1 and "null" in err()
    assert g(p, p, None, None, p, p, 1, 3, 32, 32, 64, 16, None, 48, None) == 1 and "null" in err()
    assert g(p, p, None, None, p, p, 0, 3, 32, 32, 64, 16, q, 48, None) == 1 and "B=0" in err()
    assert g(p, p, None, None, p, p, 1, 3, 32, 32, 64, 15, q, 48, None) == 1 and "N * P" in err()
    assert g(p, p, None, None, p, p, 1, 3, 32, 32, 64, 16, q, 40, None) == 1 and "ld=40" in err()
    assert g(p, p, None, None, p, p, 1, 3, 0, 32, 64, 16, q, 48, None) == 1
    # with a tile origin table: the tile kernel's envelope
    assert g(p, p, None, p, p, p, 1, 3, 32, 32, 64, 16, q, 48, None) == 1 and "P=16" in err()
    assert g(p, p, None, p, p, p, 1, 3, 32, 32, 4, 256, q, 512, None) == 1 and "ld=512" in err()
    assert g(p, p, None, p, p, p, 1, 5, 32, 32, 4, 256, q, 1280, None) == 1 and "C=5" in err()
    # the existing entry points keep their messages
    assert lib.sfcvit_tokens_gather(None, 0, p, None, 1, 3, 1024, 64, 16, q, 48, None) == 1 and err().startswith("tokens_gather: null")
    assert lib.sfcvit_tokens_gather_tiles(p, p, None, None, 1, 3, 32, 32, 4, q, 768, None) == 1 and err().startswith("tokens_gather_tiles: null")


def test_mix_on_cpu_tensors_is_rejected_like_every_other_cpu_tensor():
    from sfcvit import _lib, ops
    from sfcvit import functional as F
    from sfcvit.training import BatchMix
    from sfcvit.tokenizers import HilbertEmbedding1D
    bm = BatchMix(2, "cpu").draw(32, 32)
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(_lib.SfcvitError):
        ops.mix_images(x, bm)
    with pytest.raises(_lib.SfcvitError):
        ops.gather_tokens(x, torch.zeros(64, 16, dtype=torch.int32), mix=bm)
    with pytest.raises(_lib.SfcvitError):
        HilbertEmbedding1D(32, 16, 3, 64)(x, mix=bm)
    with pytest.raises(_lib.SfcvitError):
        F.mixed_target_cross_entropy(torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), bm)
    assert F.mix_images(x, None) is x                                # mix=None is today's code


def test_public_surface():
    import inspect
    import sfcvit.training as tr
    from sfcvit import functional as F, ops
    from sfcvit.models import VisionTransformer, VisionTransformer1D
    from sfcvit.models.altvit import HilbertViT, SimpleViT
    from sfcvit.training import loops
    import sfcvit.tokenizers as T
    assert tr.BatchMix is not None
    for fn in (ops.gather_tokens, F.patch_embed, VisionTransformer.forward, VisionTransformer1D.forward, SimpleViT.forward,
               HilbertViT.forward, T.HilbertEmbedding1D.forward, T.ZigzagEmbedding.forward, T.RandomEmbedding.forward,
               T.HierarchicalHilbertEmbedding.forward):
        assert inspect.signature(fn).parameters["mix"].default is None, fn
    assert inspect.signature(loops.train_with_mixup_or_cutmix).parameters["device_mix"].default is False
    sig = inspect.signature(tr.GraphedTrainStep.__init__).parameters
    assert sig["mix"].default is None and sig["labels"].default is None
    for name in ("mix_images", "soft_ce_pair"):
        assert callable(getattr(ops, name))
    assert callable(F.mixed_target_cross_entropy)
