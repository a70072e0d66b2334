"""Device image transforms, the parts that need no GPU: the host parameter draw (csrc/augment.cpp) against a pure-Python
restatement, its counter property and statistics, the numpy statement of the apply pipeline against Pillow, and the
argument checks of the apply entry point."""
import ctypes
import math

import numpy as np
import pytest
import torch

import augment_ref as R

CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


def _draw(B, H, W, S, seed, step, sample_base=0, **kw):
    from sfcvit import ops
    from sfcvit.training.augment import make_cfg
    rec = torch.zeros((B, 16), dtype=torch.int32)
    ops.augment_draw(rec, H, W, make_cfg(S, **kw), seed, step, sample_base)
    return rec.numpy().view(np.uint32).copy()


def _ulps(a, b):
    a, b = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    flip = lambda v: np.where(v < 0, -(v & 0x7FFFFFFF), v)      # noqa: E731  sign-magnitude -> ordered integers
    return np.abs(flip(a) - flip(b))


def _same(got, ref):
    ints = [i for i in range(16) if not R.FACTORS <= i < R.FACTORS + 4]
    fl = slice(R.FACTORS, R.FACTORS + 4)
    return np.array_equal(got[:, ints], ref[:, ints]) and _ulps(got[:, fl], ref[:, fl]).max() <= 1


def test_layout_constants_agree_with_the_header_and_the_package():
    import os
    import re
    from sfcvit.training import augment as A
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sfcvit.h")).read()
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define SFCVIT_AUG_(\w+) (\w+)", header)}
    want = {"WORDS": R.WORDS, "FLAGS": R.FLAGS, "CROP": R.CROP, "ORDER": R.ORDER, "FACTORS": R.FACTORS, "ERASE": R.ERASE,
            "FLIP_BIT": R.FLIP_BIT, "ERASE_BIT": R.ERASE_BIT, "JITTER_SHIFT": R.JITTER_SHIFT, "ORDER_IDENTITY": R.ORDER_IDENTITY}
    assert defs == want
    assert (A.WORDS, A.FLAGS, A.CROP, A.ORDER, A.FACTORS, A.ERASE, A.FLIP_BIT, A.ERASE_BIT, A.JITTER_SHIFT, A.ORDER_IDENTITY) == \
        tuple(want.values())


@pytest.mark.parametrize("H,W,S", [(32, 32, 32), (224, 224, 224), (24, 40, 40), (17, 9, 20)])
@pytest.mark.parametrize("seed,step,base", [(0, 0, 0), (42, 7, 1000), (2 ** 40 + 3, 2 ** 33 + 1, 2 ** 35)])
def test_draw_matches_the_python_restatement(H, W, S, seed, step, base):
    B = 192
    got = _draw(B, H, W, S, seed, step, base)
    ref = R.draw_ref(B, H, W, S, seed, step, base)
    assert _same(got, ref)


def test_draw_with_other_ranges_and_switches_matches_too():
    kw = dict(scale=(0.3, 0.6), ratio=(0.5, 2.0), brightness=0.9, contrast=1.5, saturation=0.0, hue=0.5, erase_p=0.7, flip=False)
    got, ref = _draw(256, 48, 64, 64, 5, 11, 0, **kw), R.draw_ref(256, 48, 64, 64, 5, 11, 0, **kw)
    assert np.array_equal(got[:, :6], ref[:, :6]) and np.array_equal(got[:, 10:], ref[:, 10:])
    assert _ulps(got[:, 6:10], ref[:, 6:10]).max() <= 1
    assert not (got[:, R.FLAGS] & R.FLIP_BIT).any()
    assert not (got[:, R.FLAGS] >> (R.JITTER_SHIFT + 2) & 1).any()          # saturation range 0: op off, factor neutral
    assert (got[:, R.FACTORS + 2].view(np.float32) == 1.0).all()
    # every switch off: the test transform's record
    off = _draw(8, 24, 40, 40, 1, 2, 3, crop=False, flip=False, brightness=0, contrast=0, saturation=0, hue=0, erase_p=0)
    want = R.make_rec(24, 40)
    assert all(np.array_equal(row, want) for row in off)


def test_counter_property():
    big = _draw(512, 32, 32, 32, 9, 4, 0)
    for k in (0, 1, 77, 511):
        assert np.array_equal(_draw(1, 32, 32, 32, 9, 4, k)[0], big[k])
    assert np.array_equal(_draw(100, 32, 32, 32, 9, 4, 300), big[300:400])
    assert not np.array_equal(_draw(512, 32, 32, 32, 10, 4, 0), big)
    assert not np.array_equal(_draw(512, 32, 32, 32, 9, 5, 0), big)
    changed = lambda other: np.mean(np.any(other != big, axis=1))            # noqa: E731
    assert changed(_draw(512, 32, 32, 32, 10, 4, 0)) > 0.99 and changed(_draw(512, 32, 32, 32, 9, 5, 0)) > 0.99


@pytest.mark.parametrize("H,W,S", [(32, 32, 32), (224, 224, 224), (24, 40, 40)])
def test_draws_are_valid_and_their_rates_binomial(H, W, S):
    n = 65536
    rec = _draw(n, H, W, S, 123, 5, 0)
    flags = rec[:, R.FLAGS]
    top, left, h, w = (rec[:, R.CROP + i].astype(np.int64) for i in range(4))
    assert (top >= 0).all() and (left >= 0).all() and (h >= 1).all() and (w >= 1).all()
    assert (top + h <= H).all() and (left + w <= W).all()
    er = (flags & R.ERASE_BIT) != 0
    et, el, eh, ew = (rec[:, R.ERASE + i].astype(np.int64) for i in range(4))
    assert (eh[er] < S).all() and (ew[er] < S).all() and (et[er] + eh[er] <= S).all() and (el[er] + ew[er] <= S).all()
    assert (rec[~er, R.ERASE:R.ERASE + 4] == 0).all()
    fac = rec[:, R.FACTORS:R.FACTORS + 4].view(np.float32)
    f32 = np.float32
    for op, x in enumerate((0.4, 0.4, 0.4)):
        assert (fac[:, op] >= f32(1 - x)).all() and (fac[:, op] <= f32(1 + x)).all()
    assert (fac[:, 3] >= f32(-0.1)).all() and (fac[:, 3] <= f32(0.1)).all()
    assert ((flags >> R.JITTER_SHIFT) & 0xF == 0xF).all()
    order = rec[:, R.ORDER]
    assert (order < 256).all()
    fields = np.stack([(order >> (2 * i)) & 3 for i in range(4)], axis=1)
    assert (np.sort(fields, axis=1) == np.arange(4)).all()

    def within(count, p):
        return abs(count / n - p) <= 5 * math.sqrt(p * (1 - p) / n)
    assert within(int((flags & R.FLIP_BIT != 0).sum()), 0.5)
    # an erase that was decided can only be lost when ten tries in a row miss h, w < S; at these sizes a single try misses
    # with probability < 0.2 (the aspect has to push one side past S), so the loss is < 1e-7 and the rate is p = 0.2
    assert within(int(er.sum()), 0.2)
    words = [sum(op << (2 * i) for i, op in enumerate(o)) for o in R.ALL_ORDERS]
    assert len(set(words)) == 24
    for wd in words:
        assert within(int((order == wd).sum()), 1 / 24), hex(wd)
    # the factors fill their ranges evenly: mean of U(a, b) within 5 sigma, sigma = (b - a) / sqrt(12 n)
    for op, (a, b) in enumerate(((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1))):
        assert abs(fac[:, op].astype(np.float64).mean() - (a + b) / 2) <= 5 * (b - a) / math.sqrt(12 * n)


@pytest.mark.parametrize("H,W,ratio,want", [
    (32, 32, (0.75, 4 / 3), (0, 0, 32, 32)),                       # ratio inside the range: the whole image
    (40, 20, (0.75, 4 / 3), (6, 0, 27, 20)),                       # W / H = 0.5 < r0: w = W, h = round(20 / 0.75) = 27
    (20, 50, (0.75, 4 / 3), (0, 11, 20, 27)),                      # W / H = 2.5 > r1: h = H, w = round(20 * 4 / 3) = 27
])
def test_fallback_crop_is_the_central_crop_rule(H, W, ratio, want):
    rec = _draw(64, H, W, max(H, W), 3, 0, 0, scale=(4.0, 5.0), ratio=ratio)     # area > H * W on every try
    assert (rec[:, R.CROP:R.CROP + 4] == np.array(want, dtype=np.uint32)).all()
    assert _same(rec, R.draw_ref(64, H, W, max(H, W), 3, 0, 0, scale=(4.0, 5.0), ratio=ratio))


def test_numpy_statement_against_pillow():
    """The fp64 numpy statement of the apply pipeline (augment_ref.apply_image, the yardstick of the GPU test) against
    Pillow, which is what torchvision's PIL backend calls: crop + Image.resize(box=, resample=BILINEAR) for the
    upsampling crop (the box is cut out first, as torchvision's resized_crop does, so the taps stay inside it) and
    ImageEnhance.Brightness / Contrast / Color.  Pillow works in uint8: its resize rounds after each of its two passes
    and uses 22-bit fixed-point weights, Image.blend truncates instead of rounding, its gray is an integer approximation
    and its contrast mean is rounded to a whole level.  Measured maxima |255 * statement - Pillow| on the inputs below,
    in uint8 levels: resize 0.9990, brightness 0.9900, contrast 1.0405, saturation 1.1790 (printed by this test).  Each
    bound is that measurement plus one level; a formula error (tap geometry, blend direction) shows as tens of levels."""
    from PIL import Image, ImageEnhance
    rng = np.random.default_rng(0)
    H, W = 48, 40
    # smooth structure + noise: a pure-noise image would hide a geometry error less well than it hides nothing at all
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([127 + 100 * np.sin(xx / 5.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)])
    img = np.clip(base + rng.normal(0, 20, base.shape), 0, 255).astype(np.uint8)
    pil = Image.fromarray(img.transpose(1, 2, 0), "RGB")

    def levels(rec, S):
        return 255.0 * R.apply_image(img, rec, S, np.float64).transpose(1, 2, 0)

    measured = {"resize": 0.0, "brightness": 0.0, "contrast": 0.0, "saturation": 0.0}
    for S, crop in ((64, (5, 7, 30, 22)), (48, (0, 0, 48, 40)), (96, (10, 3, 13, 29)), (50, (47, 39, 1, 1)), (56, (3, 2, 40, 38))):
        top, left, h, w = crop
        want = np.asarray(pil.crop((left, top, left + w, top + h)).resize((S, S), resample=Image.BILINEAR, box=(0, 0, w, h)), dtype=np.float64)
        measured["resize"] = max(measured["resize"], np.abs(levels(R.make_rec(H, W, crop=crop), S) - want).max())
        flipped = levels(R.make_rec(H, W, crop=crop, flip=True), S)
        assert np.array_equal(flipped, levels(R.make_rec(H, W, crop=crop), S)[:, ::-1])
    # the jitter ops on the un-resized image (S = H = W would need a square; use the square top of it)
    sq = img[:, :40, :40]
    psq = Image.fromarray(sq.transpose(1, 2, 0), "RGB")
    for f in (0.6, 0.85, 1.0, 1.23, 1.4):
        for name, enh, kw in (("brightness", ImageEnhance.Brightness, {"brightness": f}), ("contrast", ImageEnhance.Contrast, {"contrast": f}),
                              ("saturation", ImageEnhance.Color, {"saturation": f})):
            want = np.asarray(enh(psq).enhance(float(np.float32(f))), dtype=np.float64)
            got = 255.0 * R.apply_image(sq, R.make_rec(40, 40, **kw), 40, np.float64).transpose(1, 2, 0)
            measured[name] = max(measured[name], np.abs(got - want).max())
    print("max |255 * numpy statement - Pillow| in uint8 levels:", {k: round(float(v), 4) for k, v in measured.items()})
    bound = {"resize": 0.9990 + 1, "brightness": 0.9900 + 1, "contrast": 1.0405 + 1, "saturation": 1.1790 + 1}
    for k, v in measured.items():
        assert v <= bound[k], (k, v)


def test_fp32_statement_is_close_to_the_fp64_one():
    # the two dtypes of the shared helper evaluate the same formulas: a slip in one of them would show here, on the CPU
    rng = np.random.default_rng(1)
    u8 = rng.integers(0, 256, (24, 3, 32, 32), dtype=np.uint8)
    rec = R.draw_ref(24, 32, 32, 32, 0, 0)
    a, b = R.apply_ref(u8, rec, 32, CIFAR_MEAN, CIFAR_STD, np.float64), R.apply_ref(u8, rec, 32, CIFAR_MEAN, CIFAR_STD, np.float32)
    assert b.dtype == np.float32 and np.abs(a - b).max() < 1e-4


def test_apply_argument_checks_return_einval_without_a_launch():
    from sfcvit import _lib
    from sfcvit.training.augment import make_cfg
    lib = _lib.lib
    buf = (ctypes.c_uint8 * 4096)()                       # never dereferenced: every call below is refused first
    p = ctypes.cast(buf, ctypes.c_void_p)
    p = ctypes.c_void_p((p.value + 15) & ~15)

    def call(x=p, rec=p, out=p, B=1, C=3, H=32, W=32, cfg=None, **kw):
        cfg = cfg if cfg is not None else make_cfg(32, **kw)
        return lib.sfcvit_augment_apply(x, rec, out, B, C, H, W, ctypes.byref(cfg) if cfg != "null" else None, None)

    for null in ("x", "rec", "out"):
        assert call(**{null: None}) == 1 and b"null" in lib.sfcvit_last_error()
    assert call(cfg="null") == 1 and b"null" in lib.sfcvit_last_error()
    assert call(H=33) == 1 and b"smaller" in lib.sfcvit_last_error()             # S < H
    assert call(W=48) == 1 and b"smaller" in lib.sfcvit_last_error()             # S < W
    assert call(C=1) == 1 and b"C == 3" in lib.sfcvit_last_error()               # colour ops on a gray batch
    assert call(C=4, brightness=0, contrast=0, saturation=0, hue=0) == 1
    assert call(std=(0.2, 0.0, 0.2)) == 1 and b"std" in lib.sfcvit_last_error()
    assert call(B=0) == 1
    assert call(out=ctypes.c_void_p(p.value + 4)) == 1 and b"aligned" in lib.sfcvit_last_error()
    # the draw's own checks
    rec = (ctypes.c_uint32 * 16)()
    assert lib.sfcvit_augment_draw(None, 1, 32, 32, ctypes.byref(make_cfg(32)), 0, 0, 0) == 1
    assert lib.sfcvit_augment_draw(rec, 1, 32, 32, None, 0, 0, 0) == 1
    assert lib.sfcvit_augment_draw(rec, 1, 32, 32, ctypes.byref(make_cfg(32, scale=(0.5, 0.1))), 0, 0, 0) == 1
    assert lib.sfcvit_augment_draw(rec, 1, 32, 32, ctypes.byref(make_cfg(32, hue=0.7)), 0, 0, 0) == 1
    assert lib.sfcvit_augment_draw(rec, 1, 0, 32, ctypes.byref(make_cfg(32)), 0, 0, 0) == 1


def test_device_augment_host_side_state():
    from sfcvit.training import DeviceAugment
    a = DeviceAugment(16, 32, 32, seed=7, device="cpu")
    first = a.draw().host.copy()
    second = a.draw().host.copy()
    assert a.step == 2 and not np.array_equal(first, second)
    assert _same(first, R.draw_ref(16, 32, 32, 32, 7, 0)) and _same(second, R.draw_ref(16, 32, 32, 32, 7, 1))
    assert np.array_equal(a.rec.numpy().view(np.uint32), second)
    b = DeviceAugment(16, 32, 32, seed=0, device="cpu")
    b.load_state_dict({"seed": 7, "step": 1})
    assert np.array_equal(b.draw().host, second) and b.state_dict() == {"seed": 7, "step": 2}
    assert np.array_equal(a.draw(step=0).host, first) and a.step == 2                    # an explicit step leaves the counter
    a.sample_base = 4
    assert np.array_equal(a.draw(step=0).host[:12], first[4:])
    t = DeviceAugment.test_transform(4, 24, 40, size=40, device="cpu")
    want = R.make_rec(24, 40)
    assert all(np.array_equal(row, want) for row in t.draw().host) and t.step == 0
