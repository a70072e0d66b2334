"""Reference statements of the device image transforms, shared by test_augment_cpu.py and test_augment_gpu.py:

  * draw_ref      a pure-Python restatement of the parameter draw (csrc/augment.cpp): same hash, math.log / exp / sqrt,
                  Python's round() (half to even)
  * apply_ref     the numpy statement of the apply pipeline (csrc/augment.hip) in a chosen dtype: float64 is the
                  yardstick, float32 evaluates the same formulas in the kernel's operation order (geometry-only records
                  must then agree with the kernel bit for bit)
  * make_rec      hand-written records

Layout constants are restated here from include/sfcvit.h on purpose: a test that imported them from the package could
not notice the package and the header drifting apart together."""
import math

import numpy as np

WORDS, FLAGS, CROP, ORDER, FACTORS, ERASE = 16, 0, 1, 5, 6, 10
FLIP_BIT, ERASE_BIT, JITTER_SHIFT, ORDER_IDENTITY = 1, 2, 2, 0xE4
M32 = 0xFFFFFFFF


# ---- the draw -----------------------------------------------------------------------------------------------------------
def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


class Stream:
    def __init__(self, seed, step, sample):
        seed, step, sample = seed & (2 ** 64 - 1), step & (2 ** 64 - 1), sample & (2 ** 64 - 1)
        key = mix32((seed & M32) + 0x9E3779B1)
        for w in (seed >> 32, step & M32, step >> 32, sample & M32, sample >> 32):
            key = mix32(key ^ w)
        self.key = key

    def u(self, i, a=None, b=None):
        v = (mix32(self.key ^ ((i * 0x9E3779B1 + 0x7FEB352D) & M32)) >> 8) * (1.0 / 16777216.0)
        return v if a is None else a + (b - a) * v

    def randint(self, i, n):
        return int(math.floor(self.u(i) * n))


def order_word(k):
    items, word = [0, 1, 2, 3], 0
    for i, f in enumerate((6, 2, 1, 1)):
        j, k = divmod(k, f)
        word |= items.pop(j) << (2 * i)
    return word


def f32_bits(v):
    return int(np.array([v], dtype=np.float64).astype(np.float32).view(np.uint32)[0])


def draw_ref(B, H, W, S, seed, step, sample_base=0, crop=True, flip=True, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0),
             brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, erase_p=0.2):
    """[B, 16] uint32 records, by the rules of the issue (torchvision v2's get_params)."""
    rec = np.zeros((B, WORDS), dtype=np.uint32)
    jit = (brightness, contrast, saturation, hue)
    for b in range(B):
        st = Stream(seed, step, sample_base + b)
        flags, top, left, h, w = 0, 0, 0, H, W
        if crop:
            l0, l1 = math.log(ratio[0]), math.log(ratio[1])
            for t in range(10):
                area = float(H) * float(W) * st.u(4 * t, scale[0], scale[1])
                aspect = math.exp(st.u(4 * t + 1, l0, l1))
                cw, ch = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                if 0 < cw <= W and 0 < ch <= H:
                    w, h = cw, ch
                    top, left = st.randint(4 * t + 2, H - h + 1), st.randint(4 * t + 3, W - w + 1)
                    break
            else:
                in_ratio = float(W) / float(H)
                if in_ratio < ratio[0]:
                    w = W
                    h = int(round(w / ratio[0]))
                elif in_ratio > ratio[1]:
                    h = H
                    w = int(round(h * ratio[1]))
                else:
                    w, h = W, H
                top, left = (H - h) // 2, (W - w) // 2
        rec[b, CROP:CROP + 4] = (top, left, h, w)
        if flip and st.u(40) < 0.5:
            flags |= FLIP_BIT
        rec[b, ORDER] = order_word(st.randint(41, 24)) if any(x > 0 for x in jit) else ORDER_IDENTITY
        for op in range(4):
            f = 0.0 if op == 3 else 1.0
            if jit[op] > 0:
                flags |= 1 << (JITTER_SHIFT + op)
                f = st.u(42 + op, -jit[op], jit[op]) if op == 3 else st.u(42 + op, max(0.0, 1.0 - jit[op]), 1.0 + jit[op])
            rec[b, FACTORS + op] = f32_bits(f)
        if erase_p > 0 and st.u(46) < erase_p:
            l0, l1 = math.log(0.3), math.log(3.3)
            for t in range(10):
                area = float(S) * float(S) * st.u(48 + 4 * t, 0.02, 0.33)
                aspect = math.exp(st.u(49 + 4 * t, l0, l1))
                eh, ew = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                if eh < S and ew < S:
                    flags |= ERASE_BIT
                    rec[b, ERASE:ERASE + 4] = (st.randint(50 + 4 * t, S - eh + 1), st.randint(51 + 4 * t, S - ew + 1), eh, ew)
                    break
        rec[b, FLAGS] = flags
    return rec


# ---- hand-written records -----------------------------------------------------------------------------------------------
def make_rec(H, W, crop=None, flip=False, order=(0, 1, 2, 3), brightness=None, contrast=None, saturation=None, hue=None,
             erase=None):
    """One record: crop = (top, left, h, w) or None for the whole image; a jitter factor of None leaves the op off."""
    r = np.zeros(WORDS, dtype=np.uint32)
    flags = FLIP_BIT if flip else 0
    r[CROP:CROP + 4] = crop if crop is not None else (0, 0, H, W)
    r[ORDER] = sum(int(op) << (2 * i) for i, op in enumerate(order))
    for op, (f, neutral) in enumerate(((brightness, 1.0), (contrast, 1.0), (saturation, 1.0), (hue, 0.0))):
        if f is not None:
            flags |= 1 << (JITTER_SHIFT + op)
        r[FACTORS + op] = f32_bits(neutral if f is None else f)
    if erase is not None:
        flags |= ERASE_BIT
        r[ERASE:ERASE + 4] = erase
    r[FLAGS] = flags
    return r


# ---- the apply ----------------------------------------------------------------------------------------------------------
def _taps(S, crop, T):
    """Per output index along one axis: lower tap, upper tap, weight of the upper tap -- in dtype T, the kernel's order."""
    scale = T(crop) / T(S)
    src = (np.arange(S).astype(T) + T(0.5)) * scale
    src = src - T(0.5)
    src = np.where(src < 0, T(0), src).astype(T)
    i0 = np.minimum(src.astype(np.int64), crop - 1)
    i1 = np.minimum(i0 + 1, crop - 1)
    return i0, i1, (src - i0.astype(T)).astype(T)


def _clamp01(x):
    return np.minimum(np.maximum(x, 0), 1)


def _gray(r, g, b, T):
    return T(0.2989) * r + T(0.587) * g + T(0.114) * b


def _hue(r, g, b, hue, T):
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    eqc = maxc == minc
    cr = maxc - minc
    one = T(1)
    s = cr / np.where(eqc, one, maxc)
    div = np.where(eqc, one, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = np.where(maxc == r, bc - gc, T(0))
    hg = np.where((maxc == g) & (maxc != r), T(2) + rc - bc, T(0))
    hb = np.where((maxc != g) & (maxc != r), T(4) + gc - rc, T(0))
    h = np.fmod((hr + hg + hb) / T(6) + one, one)
    h = np.fmod(h + hue + one, one)
    v = maxc
    h6 = h * T(6)
    fi = np.floor(h6)
    f = h6 - fi
    i = fi.astype(np.int64) % 6
    p = _clamp01(v * (one - s))
    q = _clamp01(v * (one - s * f))
    t = _clamp01(v * (one - s * (one - f)))
    pick = lambda choices: np.choose(i, choices).astype(T)      # noqa: E731
    return pick([v, q, p, p, t, v]), pick([t, v, v, q, p, p]), pick([p, p, t, v, v, q])


def apply_image(img, r, S, T):
    """img uint8 [C, H, W], r one record -> [C, S, S] in dtype T on [0, 1]: crop + resize + flip, jitter ops, erase (no
    normalize)."""
    T = np.dtype(T).type
    flags = int(r[FLAGS])
    top, left, ch, cw = (int(v) for v in r[CROP:CROP + 4])
    y0, y1, wy1 = _taps(S, ch, T)
    x0, x1, wx1 = _taps(S, cw, T)
    if flags & FLIP_BIT:
        x0, x1, wx1 = x0[::-1], x1[::-1], wx1[::-1]
    box = img[:, top:top + ch, left:left + cw].astype(T) / T(255)
    wx0, wy0 = (T(1) - wx1)[None, None, :], (T(1) - wy1)[None, :, None]
    wx1b, wy1b = wx1[None, None, :], wy1[None, :, None]
    r0, r1 = box[:, y0, :], box[:, y1, :]
    a = wx0 * r0[:, :, x0] + wx1b * r0[:, :, x1]
    b = wx0 * r1[:, :, x0] + wx1b * r1[:, :, x1]
    out = (wy0 * a + wy1b * b).astype(T)
    fac = r[FACTORS:FACTORS + 4].view(np.float32).astype(T)
    if flags & (0xF << JITTER_SHIFT):
        R, G, B = out[0], out[1], out[2]
        for pos in range(4):
            op = (int(r[ORDER]) >> (2 * pos)) & 3
            if not (flags >> (JITTER_SHIFT + op)) & 1:
                continue
            f = fac[op]
            if op == 0:
                R, G, B = (_clamp01(f * c) for c in (R, G, B))
            elif op == 1:
                k = (T(1) - f) * _gray(R, G, B, T).mean(dtype=T)
                R, G, B = (_clamp01(f * c + k) for c in (R, G, B))
            elif op == 2:
                k = (T(1) - f) * _gray(R, G, B, T)
                R, G, B = (_clamp01(f * c + k) for c in (R, G, B))
            else:
                R, G, B = _hue(R, G, B, f, T)
        out = np.stack([R, G, B]).astype(T)
    if flags & ERASE_BIT:
        et, el, eh, ew = (int(v) for v in r[ERASE:ERASE + 4])
        out[:, et:et + eh, el:el + ew] = 0
    return out


def apply_ref(u8, rec, S, mean, std, dtype=np.float64):
    """u8 uint8 [B, C, H, W], rec uint32 [B, 16] -> [B, C, S, S] in `dtype`: the whole pipeline, (x - mean) / std included
    (mean / std are the fp32 values the kernel holds, widened)."""
    T = np.dtype(dtype).type
    C = u8.shape[1]
    m = np.asarray(mean, dtype=np.float32)[:C].astype(T)[:, None, None]
    s = np.asarray(std, dtype=np.float32)[:C].astype(T)[:, None, None]
    out = np.empty((u8.shape[0], C, S, S), dtype=T)
    for b in range(u8.shape[0]):
        out[b] = (apply_image(u8[b], rec[b], S, T) - m) / s
    return out


ALL_ORDERS = [(a, b, c, d) for a in range(4) for b in range(4) for c in range(4) for d in range(4)
              if len({a, b, c, d}) == 4]
