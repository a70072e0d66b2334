"""Rotary position embeddings without a GPU: the reference against a complex-multiply statement, relativity along the curve and
in the image, the CLS row, the adjoint identity on the exact-answer inputs, the table builders' refusals, the plans of the kernels
through the library (geometry, workspace, every refusal decided before any HIP call), the ABI surface, the sanitizer program's
coverage, the state_dict surface, the refusals of the constructors, F.* and main.py, and the store-point cap of the GPU test held
by the reference alone."""
import ctypes
import importlib.util
import math
import os
import re

import pytest
import torch

import qk_norm_ref
import rope_ref
from oracle.cases import MODEL_CASES
from test_host_cpu import build_model
from token_pool_ref import build_with

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd")
EINVAL = 1
BF16 = torch.bfloat16
NEW_SYMBOLS = ("sfcvit_rope_fwd", "sfcvit_rope_bwd", "sfcvit_rope_bwd_ws", "sfcvit_rope_plan")
# (B, N, H, hd) of the GPU tests: a full slot group, 6 of 8 slots, the CLS token count with three groups and an odd N, m mod N
# wrapping many times (a long batch walk), B = 1, N = 1, padding (also one that is no multiple of 8), a single pair, and the
# other kernel head dims
SHAPES = [(2, 5, 4, 64), (2, 5, 3, 64), (2, 197, 12, 64), (67, 3, 1, 64), (1, 9, 2, 64), (3, 1, 2, 64), (2, 5, 4, 48), (2, 5, 4, 20),
          (1, 3, 1, 2), (1, 7, 2, 128), (1, 7, 2, 96), (1, 7, 1, 192), (1, 7, 1, 256)]
STORE_CAP = 1e-3                                                # the fraction cap of the GPU test (test_parity_gpu._store_point)


def _hp(hd):
    return next(s for s in (64, 128, 192, 256) if hd <= s)


def general(B, N, H, hd, seed=0):
    """randn, offset and scaled per head slot, a table of arbitrary angles -> (qkv [M, 3 H hp] bf16, table [N, hd / 2, 2] fp32, dy
    [M, 3 H hp] bf16) on the CPU, padded columns zero."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + N + 31 * H + hd)
    M, hp = B * N, _hp(hd)
    slots = torch.arange(2 * H).float()
    x = torch.randn(M, 2 * H, hd, generator=g) * (0.5 + 0.25 * slots)[None, :, None] + (slots - H)[None, :, None] * 0.7
    t = torch.zeros(M, 3, H, hp)
    t[:, :2, :, :hd] = x.reshape(M, 2, H, hd)
    t[:, 2, :, :hd] = torch.randn(M, H, hd, generator=g)
    theta = torch.rand(N, hd // 2, generator=g, dtype=torch.float64) * (2 * math.pi)
    table = torch.stack((torch.cos(theta), torch.sin(theta)), dim=-1).float().contiguous()
    dy = torch.zeros(M, 3, H, hp)
    dy[..., :hd] = torch.randn(M, 3, H, hd, generator=g)
    return t.reshape(M, 3 * H * hp).to(BF16), table, dy.reshape(M, 3 * H * hp).to(BF16)


# ---- (a) the reference ---------------------------------------------------------------------------------------------------------
def test_reference_without_rope_is_the_existing_references():
    from test_qk_norm_cpu import _layer_inputs
    B, N, D, H, Fd = 3, 9, 32, 4, 64
    x, P, qk = _layer_inputs(B, N, D, H, Fd, 3, pre=False)
    one, ones = torch.ones(()), torch.ones(B)
    for kw in ({}, dict(qk_norm=qk)):
        assert torch.equal(rope_ref.encoder_layer(x, P, H, (one, one, one, one), ones, ones, **kw),
                           qk_norm_ref.encoder_layer(x, P, H, (one, one, one, one), ones, ones, **kw))
    s, Pp, qk = _layer_inputs(B, N, D, H, Fd, 4, pre=True)
    n = torch.nn.functional.layer_norm(s, (D,))
    for kw in ({}, dict(qk_norm=qk)):
        a, b = rope_ref.pre_norm_layer(s, n, Pp, H, act="gelu", **kw), qk_norm_ref.pre_norm_layer(s, n, Pp, H, act="gelu", **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and with a table the layers change
    from sfcvit import rope
    table = rope.curve_table(N, D // H)
    y0 = rope_ref.encoder_layer(x, P, H, (one, one, one, one), ones, ones)
    y1 = rope_ref.encoder_layer(x, P, H, (one, one, one, one), ones, ones, rope=table)
    assert float((y0 - y1).abs().max()) > 1e-3
    # an identity table is the layer without one, up to the rounding of x * 1 - x * 0
    ident = torch.zeros(N, D // H // 2, 2)
    ident[..., 0] = 1
    assert torch.equal(rope_ref.encoder_layer(x, P, H, (one, one, one, one), ones, ones, rope=ident), y0)


def test_reference_is_the_complex_multiplication():
    """view_as_complex of the pairs times c + i s, RoPE-ViT's own statement, in fp64; and the packed-buffer forward agrees."""
    from sfcvit import rope
    g = torch.Generator().manual_seed(1)
    B, H, N, hd = 2, 3, 7, 12
    t = torch.randn(B, H, N, hd, generator=g, dtype=torch.float64)
    for table in (rope.curve_table(N, hd).double(), rope.image_table(torch.rand(N, 2, generator=g) * 32, 8.0, hd).double(),
                  torch.randn(N, hd // 2, 2, generator=g, dtype=torch.float64)):
        a, b = rope_ref.rotate(t, table), rope_ref.rotate_complex(t, table)
        assert float((a - b).abs().max()) <= 1e-15 * float(a.abs().max()) * 8
        # the transposed map is the multiplication by the conjugate
        conj = table * torch.tensor([1.0, -1.0], dtype=torch.float64)
        assert float((rope_ref.rotate_t(t, table) - rope_ref.rotate_complex(t, conj)).abs().max()) <= 1e-14
    for B_, N_, H_, hd_ in ((2, 5, 3, 64), (2, 5, 4, 20)):
        qkv, table, _ = general(B_, N_, H_, hd_)
        hp = _hp(hd_)
        got = rope_ref.forward64(qkv, table, H_, hd_, hp)
        src = rope_ref.heads(qkv.double(), H_, hp, 3)
        for i in range(2):
            want = rope_ref.rotate(src[:, i, :, :hd_].reshape(B_, N_, H_, hd_).transpose(1, 2), table.double()).transpose(1, 2)
            assert torch.equal(got[:, i, :, :hd_], want.reshape(B_ * N_, H_, hd_))
        assert torch.equal(got[:, 2], src[:, 2]) and not bool(got[:, :2, :, hd_:].any())


def _hilbert_d2xy(order, d):
    x = y = 0
    t, s = d, 1
    while s < order:
        rx = 1 & (t // 2)
        ry = 1 & (t ^ rx)
        if ry == 0:
            if rx == 1:
                x, y = s - 1 - x, s - 1 - y
            x, y = y, x
        x, y = x + s * rx, y + s * ry
        t //= 4
        s *= 2
    return x, y


# The table is the fp32 rounding of (cos, sin): each entry is off by at most 2^-25, a 2 x 2 block by at most 2^-24 in norm, and a
# score q^T R_i^T R_j k by at most 2 * 2^-24 |q| |k| (one perturbed factor at a time) -- so two scores that are equal with an
# exact table differ by at most 2^-22 |q| |k| with this one.
REL_TOL = 2.0 ** -22


def test_curve_table_scores_depend_on_the_offset_along_the_sequence():
    from sfcvit import rope
    N, hd = 16, 8
    g = torch.Generator().manual_seed(2)
    q, k = torch.randn(hd, generator=g, dtype=torch.float64), torch.randn(hd, generator=g, dtype=torch.float64)
    table = rope.curve_table(N, hd).double()
    sc = rope_ref.rotate(q.expand(N, hd), table) @ rope_ref.rotate(k.expand(N, hd), table).t()       # [i, j]
    tol = REL_TOL * float(q.norm() * k.norm())
    spread = []
    for d in range(-(N - 1), N):
        diag = torch.diagonal(sc, d)
        assert float(diag.max() - diag.min()) <= tol, (d, float(diag.max() - diag.min()))
        spread.append(float(diag[0]))
    assert max(spread) - min(spread) > 1e3 * tol, "the score does not depend on the offset at all"
    # theta[n, p] = n * base^(-2 p / hd)
    want = torch.arange(N, dtype=torch.float64)[:, None] * 10000.0 ** (-2 * torch.arange(hd // 2, dtype=torch.float64) / hd)
    assert torch.equal(rope.curve_table(N, hd), torch.stack((want.cos(), want.sin()), -1).float())
    assert not torch.equal(rope.curve_table(N, hd, base=100.0), rope.curve_table(N, hd))


def test_image_table_scores_depend_on_the_cell_displacement_whatever_the_order():
    """A 4 x 4 grid of 8-pixel cells in Hilbert and in raster order: the same image displacement gives the same score in both."""
    from sfcvit import rope
    side, cell, hd = 4, 8.0, 16
    g = torch.Generator().manual_seed(3)
    q, k = torch.randn(hd, generator=g, dtype=torch.float64), torch.randn(hd, generator=g, dtype=torch.float64)
    tol = REL_TOL * float(q.norm() * k.norm())
    orders = {"raster": [(n // side, n % side) for n in range(side * side)],
              "hilbert": [_hilbert_d2xy(side, n)[::-1] for n in range(side * side)]}
    assert sorted(orders["hilbert"]) == sorted(orders["raster"]) and orders["hilbert"] != orders["raster"]
    by_disp = {}
    for name, cells in orders.items():
        pos = torch.tensor([[(r + 0.5) * cell, (c + 0.5) * cell] for r, c in cells])
        table = rope.image_table(pos, cell, hd).double()
        sc = rope_ref.rotate(q.expand(len(cells), hd), table) @ rope_ref.rotate(k.expand(len(cells), hd), table).t()
        for i, (ri, ci) in enumerate(cells):
            for j, (rj, cj) in enumerate(cells):
                by_disp.setdefault((rj - ri, cj - ci), []).append(float(sc[i, j]))
    assert len(by_disp) == (2 * side - 1) ** 2
    for d, vals in by_disp.items():
        assert max(vals) - min(vals) <= tol, (d, max(vals) - min(vals))
    means = sorted(sum(v) / len(v) for v in by_disp.values())
    assert means[-1] - means[0] > 1e3 * tol
    # the row and the column turn different pairs: a step down is not a step right
    assert abs(by_disp[(1, 0)][0] - by_disp[(0, 1)][0]) > 1e3 * tol
    # pairs 0 .. hd/4 - 1 turn with col / cell * f_j, pairs hd/4 .. hd/2 - 1 with row / cell * f_j, f_j = base^(-4 j / hd)
    pos = torch.tensor([[20.0, 4.0], [12.0, 28.0]])
    f = 100.0 ** (-4 * torch.arange(hd // 4, dtype=torch.float64) / hd)
    theta = torch.cat((pos[:, 1:2].double() / cell * f, pos[:, 0:1].double() / cell * f), 1)
    assert torch.equal(rope.image_table(pos, cell, hd), torch.stack((theta.cos(), theta.sin()), -1).float())


def test_cls_row_is_the_identity():
    from sfcvit import rope
    table = rope.curve_table(5, 8)
    with_cls = rope.with_cls_token(table)
    assert tuple(with_cls.shape) == (6, 4, 2) and with_cls.dtype == torch.float32
    assert torch.equal(with_cls[1:], table) and bool((with_cls[0, :, 0] == 1).all()) and bool((with_cls[0, :, 1] == 0).all())
    t = torch.randn(2, 3, 6, 8, dtype=torch.float64)
    assert torch.equal(rope_ref.rotate(t, with_cls.double())[:, :, 0], t[:, :, 0])
    # token 0 of a curve table is an identity row too; the others are not
    assert torch.equal(table[0], with_cls[0]) and not torch.equal(table[1], with_cls[0])


@pytest.mark.parametrize("B,N,H,hd", [s for s in SHAPES if _hp(s[3]) == s[3]])
def test_adjoint_identity_is_exact_on_the_exact_answer_inputs(B, N, H, hd):
    """<R x, y> = <x, R^T y>, every term exact; and every answer is a multiple of 1/2 that bf16 holds."""
    x, dy, table = rope_ref.exact_inputs(B, N, H, hd)
    y, dx = rope_ref.exact_answers(x, dy, table)
    assert float((y * dy).sum(dtype=torch.float64)) == float((x * dx).sum(dtype=torch.float64))
    for t in (x, dy, y, dx):
        assert torch.equal(t.to(BF16).float(), t) and torch.equal(t * 2, (t * 2).round()) and float(t.abs().max()) <= 16
    assert float(y.abs().max()) > 4 and float((table[..., 0] ** 2 + table[..., 1] ** 2 - 1).abs().max()) > 1, "these are rotations"
    M = B * N
    hp = hd
    pack = torch.zeros(M, 3, H, hp)
    pack[:, :2] = x.reshape(M, 2, H, hd)
    assert torch.equal(rope_ref.forward64(pack.reshape(M, -1).to(BF16), table, H, hd, hp)[:, :2].float(), y.reshape(M, 2, H, hd))
    pack[:, :2] = dy.reshape(M, 2, H, hd)
    assert torch.equal(rope_ref.backward64(pack.reshape(M, -1).to(BF16), table, H, hd, hp).float(), dx.reshape(M, 2, H, hd))


def test_builder_refusals():
    from sfcvit import ops, rope
    pos = torch.tensor([[4.0, 4.0], [4.0, 12.0]])
    for hd in (0, 1, 3, 7, -2):
        with pytest.raises(ValueError, match="head_dim="):
            rope.curve_table(4, hd)
    for hd in (0, 2, 6, 10, 7):
        with pytest.raises(ValueError, match="multiple of 4"):
            rope.image_table(pos, 8.0, hd)
    for base in (float("nan"), float("inf"), -float("inf"), 0.0, -3.0):
        with pytest.raises(ValueError, match="base="):
            rope.curve_table(4, 8, base)
        with pytest.raises(ValueError, match="base="):
            rope.image_table(pos, 8.0, 8, base)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell="):
            rope.image_table(pos, cell, 8)
    with pytest.raises(ValueError, match="n_tokens="):
        rope.curve_table(0, 8)
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        rope.image_table(torch.zeros(3), 8.0, 8)
    with pytest.raises(ValueError, match="non-finite"):
        rope.image_table(torch.tensor([[0.0, float("nan")]]), 8.0, 8)
    with pytest.raises(ValueError, match="with_cls_token"):
        rope.with_cls_token(torch.zeros(3, 4))
    # ops.RopeTable: shape, dtype, finiteness
    good = rope.curve_table(4, 8)
    t = ops.RopeTable(good)
    assert t.n_tokens == 4 and t.head_dim == 8 and torch.equal(t.table, good) and "N=4" in repr(t)
    bad = good.clone()
    bad[2, 1, 0] = float("inf")
    for wrong in (good.double(), good[:, :, 0], good.reshape(4, 8), torch.zeros(0, 4, 2), "curve", bad):
        with pytest.raises(ValueError, match="RopeTable"):
            ops.RopeTable(wrong)


# ---- (b) the plans through the library -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,H,hd", SHAPES + [(256, 196, 12, 64), (256, 197, 12, 64), (64, 576, 16, 64)])
def test_plan_and_workspace(B, N, H, hd):
    from sfcvit import ops
    from sfcvit._lib import lib
    hp = _hp(hd)
    plan = ops.rope_plan(B, N, H, hp)
    print((B, N, H, hd), plan)
    tok, img = plan["tokens_per_wg"], plan["batch_per_wg"]
    assert plan["vpl"] == hp // 64 and plan["slot_groups"] == -(-2 * H // 8) and tok >= 1 and img >= 1 and plan["rows_per_wg"] == tok * img
    assert plan["blocks"] == plan["slot_groups"] * -(-N // tok) * -(-B // img)
    assert lib.sfcvit_rope_bwd_ws(B, N, H, hp) == plan["blocks"] * 8 * hp * 4
    assert lib.sfcvit_rope_bwd_ws(0, N, H, hp) == 0 and lib.sfcvit_rope_bwd_ws(B, 0, H, hp) == 0
    assert lib.sfcvit_rope_bwd_ws(B, N, 0, hp) == 0 and lib.sfcvit_rope_bwd_ws(B, N, H, 96) == 0
    out = (ctypes.c_int32 * 5)()
    assert lib.sfcvit_rope_plan(B, N, H, 100, out) == EINVAL and lib.sfcvit_rope_plan(B, N, H, hp, None) == EINVAL
    if B * N >= 64 * 576:
        assert plan["blocks"] >= 4 * 256, "the ViT-B / ViT-L grids fill 256 CUs several times over"


def test_host_refusals_launch_nothing():
    """Every refusal is SFCVIT_EINVAL with a message, decided before any HIP call: without a GPU a launch attempt would come back
    as a launch error (status 2), not as status 1."""
    from sfcvit._lib import lib
    raw = ctypes.create_string_buffer(1 << 20)
    p = (ctypes.addressof(raw) + 15) // 16 * 16                # 16-byte aligned host addresses: never dereferenced
    qkv, tab, cs, vs, ws = (p + (i << 16) for i in range(5))

    def fwd(qkv=qkv, table=tab, B=2, N=5, H=4, hd=64, hp=64):
        return lib.sfcvit_rope_fwd(qkv, table, B, N, H, hd, hp, None)

    def bwd(dqkv=qkv, table=tab, colsum=cs, vsum=vs, ws=ws, B=2, N=5, H=4, hd=64, hp=64):
        return lib.sfcvit_rope_bwd(dqkv, table, colsum, 0, vsum, ws, B, N, H, hd, hp, None)

    def refused(rc, word):
        msg = lib.sfcvit_last_error().decode()
        print(rc, msg)
        assert rc == EINVAL and word in msg, (rc, msg)

    for n in ("qkv", "table"):
        refused(fwd(**{n: None}), "null")
    for n in ("dqkv", "table"):
        refused(bwd(**{n: None}), "null")
    refused(bwd(ws=None), "colsum without a workspace")
    refused(bwd(ws=None, vsum=None), "colsum without a workspace")
    refused(bwd(colsum=None), "vsum without colsum")
    for n, addr in dict(qkv=qkv, table=tab).items():
        refused(fwd(**{n: addr + 8}), "aligned")
    for n, addr in dict(dqkv=qkv, table=tab, colsum=cs, vsum=vs, ws=ws).items():
        refused(bwd(**{n: addr + 8}), "aligned")
    for f, what in ((fwd, "rope_fwd"), (bwd, "rope_bwd")):
        for hp in (0, 32, 96, 65, 512, -64):
            refused(f(hp=hp, hd=8), "not a kernel head dim")
        refused(f(hp=100, hd=8), what)
        for hd in (0, -2, 1, 3, 63, 66, 1000):                  # odd, < 2, > hp
            refused(f(hd=hd), f"hd={hd}")
        refused(f(hd=130, hp=128), "hd=130")
        for z in (0, -5):
            refused(f(B=z), f"B={z}")
            refused(f(N=z), f"N={z}")
            refused(f(H=z), f"H={z}")
        refused(f(H=11184811), "leaves int")                   # 3 * H * 64 = 2^31 + 64
        refused(f(H=2 ** 31 - 1, hp=256, hd=64), "leaves int")
        refused(f(B=65536, N=32768), "leaves int")             # B * N = 2^31
        refused(f(B=1, N=2 ** 31 - 1, H=64), "leaves int")     # 16 slot groups * 2^29 token blocks
    buf = ctypes.create_string_buffer(96)
    assert lib.sfcvit_last_rowwise_kernel(buf, 96) == 0 and b"rope" not in buf.value      # nothing was launched


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
    from sfcvit import functional as F, ops, rope
    from sfcvit._lib import SfcvitError
    z = torch.zeros(4, 3 * 2 * 64, dtype=BF16)
    table = ops.RopeTable(rope.curve_table(4, 64))
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        ops.rope_fwd(z, table, 2)
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        ops.rope_bwd(z, table, 2)
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        F.rope(z, table, 2)


def test_sanitizer_program_covers_the_new_plans():
    """rope.cpp is compiled into the sanitizer program and check_rope is part of it; tests/test_host_cpu.py builds and runs it
    (`make asan`) on every CPU test run."""
    csrc = os.path.join(PKG, "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^ASAN_SRCS :=.*\brope\.cpp\b", mk, re.M)
    src = open(os.path.join(csrc, "hostcheck", "host_check.cpp")).read()
    assert "static void check_rope()" in src and "\n    check_rope();" in src


# ---- (c) constructors, F.* and main.py -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["raster32_2d", "hilbert32_1d"])
def test_state_dict_surface(name):
    cfg, _ = MODEL_CASES[name]
    hd = cfg.embed_dim // cfg.n_heads
    models = {}
    for tag, kw in dict(base=None, off=dict(rope=None), curve=dict(rope="curve"), image=dict(rope="image", rope_base=50.0),
                        cls=dict(rope="image", pool="cls"), plain_cls=dict(pool="cls"),
                        pre=dict(rope="curve", qk_norm=True, norm_first=True, activation="gelu", layer_scale=1e-4),
                        plain_pre=dict(qk_norm=True, norm_first=True, activation="gelu", layer_scale=1e-4)).items():
        torch.manual_seed(7)
        models[tag] = build_model(cfg) if kw is None else build_with(cfg, **kw)
    sd = {k: m.state_dict() for k, m in models.items()}
    for a, b in (("base", "off"), ("base", "curve"), ("base", "image"), ("plain_cls", "cls"), ("plain_pre", "pre")):
        assert list(sd[a]) == list(sd[b]) and all(torch.equal(sd[a][k], sd[b][k]) for k in sd[a]), (a, b)
    assert not hasattr(models["off"].encoder, "rope") and not hasattr(models["base"].encoder, "rope_table")
    N = models["base"].patch_embed.n_patches
    for tag, n, base in (("curve", N, 10000.0), ("image", N, 50.0), ("cls", N + 1, 100.0), ("pre", N, 10000.0)):
        enc = models[tag].encoder
        assert tuple(enc.rope_table.shape) == (n, hd // 2, 2) and enc.rope_base == base and enc.rope.n_tokens == n
        assert "rope_table" in dict(enc.named_buffers()) and "rope_table" not in enc.state_dict()
        assert torch.equal(enc.rope.table, enc.rope_table)
    from sfcvit import rope
    assert torch.equal(models["curve"].encoder.rope_table, rope.curve_table(N, hd))
    cls = models["cls"].encoder.rope_table
    assert bool((cls[0, :, 0] == 1).all()) and bool((cls[0, :, 1] == 0).all())
    assert torch.equal(cls[1:], rope.image_table(__import__("sfcvit.analysis").analysis.token_positions(models["cls"].patch_embed),
                                                 math.sqrt(cfg.img_size ** 2 / N), hd))
    # checkpoints move both ways
    models["base"].load_state_dict(sd["curve"], strict=True)
    models["image"].load_state_dict(sd["base"], strict=True)
    # the bf16 cast of a training run leaves the kernels' table alone
    enc = models["curve"].to(BF16).encoder
    assert enc.rope.table.dtype == torch.float32 and enc.rope_table.dtype == BF16


def test_constructor_and_functional_refusals():
    from sfcvit import functional as F, ops, rope
    from sfcvit.models import TransformerSeqEncoder, VisionTransformer, VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    with pytest.raises(ValueError, match="must be even"):
        TransformerSeqEncoder(18, 4, 2, 32, None, rope="curve")                 # head dim 9
    with pytest.raises(ValueError, match="multiple of 4"):
        TransformerSeqEncoder(12, 4, 2, 32, None, rope="image")                 # head dim 6
    with pytest.raises(ValueError, match="exceeds the largest supported"):
        TransformerSeqEncoder(1024, 4, 2, 32, None, rope="curve")
    with pytest.raises(ValueError, match="rope="):
        TransformerSeqEncoder(16, 4, 2, 32, None, rope="spiral")
    for base in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rope_base="):
            TransformerSeqEncoder(16, 4, 2, 32, None, rope="curve", rope_base=base)
    enc = TransformerSeqEncoder(16, 4, 2, 32, None, n_layers=3, rope="curve", rope_base=500.0)
    assert enc.rope.n_tokens == 4 and enc.rope.head_dim == 8 and enc.rope_base == 500.0
    assert torch.equal(enc.rope.table, rope.curve_table(4, 8, 500.0))
    assert not hasattr(TransformerSeqEncoder(16, 4, 2, 32, None), "rope")
    for cls in (VisionTransformer, VisionTransformer1D):
        m = cls(HilbertEmbedding1D(32, 256, 3, 32), depth=2, n_heads=2, mlp_dim=32, norm_first=True, activation="gelu", layer_scale=0.1,
                drop_path_rate=0.1, pool="cls", pos_embed="learned", qk_norm=True, rope="image")
        assert m.encoder.rope.n_tokens == m.patch_embed.n_patches + 1 and m.encoder.rope_kind == "image" and m.encoder.rope_base == 100.0
        m = cls(HilbertEmbedding1D(32, 256, 3, 32), depth=1, n_heads=2, mlp_dim=32, rel_pos_bias="curve", rope="curve")
        assert m.encoder.rope.n_tokens == m.patch_embed.n_patches and len(m.encoder.rel_pos_bias) == 1
        with pytest.raises(ValueError, match="rope_base needs rope"):
            cls(HilbertEmbedding1D(32, 256, 3, 32), depth=1, n_heads=2, mlp_dim=32, rope_base=10.0)
        with pytest.raises(ValueError, match="multiple of 4"):
            cls(HilbertEmbedding1D(32, 256, 3, 12), depth=1, n_heads=2, mlp_dim=32, rope="image")
    D, H, N = 16, 2, 2
    x = torch.zeros(1, N, D)
    w = [torch.zeros(3 * D, D), torch.zeros(3 * D), torch.zeros(D, D)] + [torch.zeros(D)] * 3 + [torch.zeros(32, D), torch.zeros(32),
                                                                                                  torch.zeros(D, 32)] + [torch.zeros(D)] * 3
    good = rope.curve_table(N, D // H)
    for bad, word in ((rope.curve_table(N + 1, D // H), "rope table for"), (rope.curve_table(N, D // H + 2), "rope table for"),
                      (ops.RopeTable(rope.curve_table(N, 4)), "rope table for"), ("curve", "rope must be"),
                      (good.double(), "RopeTable"), (good[..., 0], "RopeTable")):
        for call in (lambda: F.encoder_layer(x, *w, H, rope=bad), lambda: F.pre_norm_layer(x, x, *w, H, rope=bad),
                     lambda: F.encoder_layer_probe(x, *w, H, rope=bad), lambda: F.pre_norm_layer_probe(x, x, *w, H, rope=bad)):
            with pytest.raises(ValueError, match=word):
                call()
    D = 6                                                       # head dim 3
    x3 = torch.zeros(1, N, D)
    w3 = [torch.zeros(3 * D, D), torch.zeros(3 * D), torch.zeros(D, D)] + [torch.zeros(D)] * 3 + [torch.zeros(32, D), torch.zeros(32),
                                                                                                   torch.zeros(D, 32)] + [torch.zeros(D)] * 3
    with pytest.raises(ValueError, match="even head dim"):
        F.encoder_layer(x3, *w3, 2, rope=rope.curve_table(N, 2))
    z = torch.zeros(2, 3, 3 * 2 * 64)
    with pytest.raises(ValueError, match="table must be"):
        F.rope(z, None, 2)
    with pytest.raises(ValueError, match="packed width"):
        F.rope(torch.zeros(3, 100), good, 2)
    with pytest.raises(ValueError, match="packed head width"):
        F.rope(torch.zeros(2, 3, 3 * 2 * 48), rope.curve_table(3, 48), 2)       # 48 is not a kernel head dim
    with pytest.raises(ValueError, match="rope table for"):
        F.rope(z, rope.curve_table(4, 64), 2)                                  # a table for 4 tokens on a sequence of 3


@pytest.mark.parametrize("pre", [False, True], ids=["post_norm", "pre_norm"])
def test_torch_compile_refuses_rope(pre):
    """Decided while tracing, before any kernel: the encoder alone, on a machine without a GPU."""
    from sfcvit.models import TransformerSeqEncoder
    enc = TransformerSeqEncoder(128, 4, 2, 256, None, dropout_p=0.0, n_layers=1, rope="curve", norm_first=pre).to(BF16).eval()
    want = "the pre-norm layer has no traced form" if pre else "rope is not supported under torch.compile"
    try:
        with pytest.raises(NotImplementedError, match=want):
            torch.compile(enc)(torch.randn(2, 4, 128, dtype=BF16))
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
    assert a.rope is None and a.rope_base is None and not hasattr(main.build_model(a, main.build_tokenizer(a)).encoder, "rope")
    a = main.parse_args(small + ["--rope", "curve"])
    enc = main.build_model(a, main.build_tokenizer(a)).encoder
    assert enc.rope_kind == "curve" and enc.rope_base == 10000.0 and enc.rope.head_dim == 32 and not enc.norm_first
    a = main.parse_args(small + ["--rope", "image", "--rope-base", "50", "--qk-norm", "--pre-norm", "--activation", "gelu", "--layer-scale",
                                 "--drop-path", "0.1", "--rel-pos-bias", "curve", "--pool", "cls", "--pos-embed", "sincos2d"])
    enc = main.build_model(a, main.build_tokenizer(a)).encoder
    assert enc.rope_kind == "image" and enc.rope_base == 50.0 and enc.norm_first and len(enc.qk_norm) == 3 and len(enc.rel_pos_bias) == 3
    assert enc.rope.n_tokens == enc.max_len + 1
    for bad in (["--rope", "spiral"], ["--rope"], ["--rope-base", "10"], ["--rope", "curve", "--rope-base", "0"],
                ["--rope", "curve", "--rope-base", "nan"], ["--rope", "curve", "--rope-base", "inf"], ["--rope", "curve", "--rope-base", "x"]):
        with pytest.raises(SystemExit):
            main.parse_args(small + bad)


# ---- (d) the store-point cap, held by the reference alone --------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,H,hd", SHAPES)
def test_fp32_restatements_stay_within_a_quarter_of_the_store_point_cap(B, N, H, hd):
    """On the general inputs of the GPU test: the forward and the backward evaluated in fp32 -- two products and a sum, or one product
    and a fused multiply-add (either product fused) -- and rounded to bf16 differ from the bf16-rounded fp64 result on at most a
    quarter of what the GPU test allows the kernel (test_parity_gpu._store_point: 1e-3 of the elements + 8)."""
    qkv, table, dy = general(B, N, H, hd)
    hp, M = _hp(hd), B * N
    cs = table[torch.arange(M) % N][:, None, None]             # [M, 1, 1, hd / 2, 2] fp32
    c, s = cs[..., 0], cs[..., 1]
    fused = lambda a, b, d: (a.double() * b.double() + d.double()).float()       # noqa: E731  (a * b is exact in fp64: 8 + 24 bits)
    for name, buf, ref, sign in (("forward", qkv, rope_ref.forward64(qkv, table, H, hd, hp)[:, :2, :, :hd], 1.0),
                                 ("backward", dy, rope_ref.backward64(dy, table, H, hd, hp)[..., :hd], -1.0)):
        t = rope_ref.heads(buf.float(), H, hp, 3)[:, :2, :, :hd]
        x0, x1 = t[..., 0::2], t[..., 1::2]
        ss = s * sign                                           # forward: (x0 c - x1 s, x0 s + x1 c); backward: s -> -s
        forms = {"two products": (x0 * c - x1 * ss, x0 * ss + x1 * c),
                 "fma on the first": (fused(x0, c, -(x1 * ss)), fused(x0, ss, x1 * c)),
                 "fma on the second": (fused(-x1, ss, x0 * c), fused(x1, c, x0 * ss))}
        want = ref.float().to(BF16)
        allowed = 0.25 * (STORE_CAP * want.numel() + 8)
        for form, (y0, y1) in forms.items():
            got = torch.stack((y0, y1), -1).flatten(-2).to(BF16)
            differ = int((got.view(torch.int16) != want.view(torch.int16)).sum())
            print(f"{(B, N, H, hd)} {name}, {form}: {differ} of {want.numel()} differ (allowed {allowed:.1f})")
            assert differ <= allowed, (name, form, differ)
            assert float((got.float() - want.float()).abs().max()) <= 2.0 ** -7 * float(want.float().abs().max())
