"""CLS token and pooled heads without a GPU: the fixture against an fp64 restatement, the host-side plans and refusals of
sfcvit_cls_prepend_* / sfcvit_token_pool_* (decided before any HIP call), the ABI surface, masks.with_cls_token, the
models' `pool` keyword, and which attention kernels the N + 1 sequences plan onto."""
import ctypes
import json
import os
import re

import pytest
import torch

from oracle.cases import MODEL_CASES
from test_host_cpu import build_model
from token_pool_ref import build_with, load_fixture, model_ref, pooled_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
CASES = ["raster32_2d", "hilbert32_1d"]
POOLS = ["cls", "mean"]
NEW_SYMBOLS = ("sfcvit_cls_prepend_fwd", "sfcvit_cls_prepend_bwd", "sfcvit_cls_prepend_bwd_workspace", "sfcvit_token_pool_fwd",
               "sfcvit_token_pool_bwd", "sfcvit_last_token_pool_kernel")


def _rel(got, ref):
    return float((got.double().flatten() - ref.double().flatten()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("name", CASES)
def test_fixture_equals_the_fp64_statement(name, pool):
    """The reference modules' fp32 logits, loss and gradients with a CLS token / a pooled head (tests/golden/token_pool.json)
    against the same forward in fp64 (token_pool_ref.model_ref): 1e-5 relative to max |value|, the positional-embedding
    fixture's bar."""
    case, ref = load_fixture()["cases"][name][pool], model_ref(name, pool)
    figures = {"logits": _rel(torch.tensor(case["logits"]), ref["logits"]),
               "loss": abs(case["loss"] - ref["loss"]) / abs(ref["loss"])}
    if pool == "cls":
        figures["dcls"] = _rel(torch.tensor(case["dcls"]), ref["dcls"])
    norms = {k: v for k, v in case["grad_l2"].items() if v is not None}
    top = max(ref["grad_l2"][k] for k in norms)
    figures["grad_l2"] = max(abs(v - ref["grad_l2"][k]) for k, v in norms.items()) / top
    print(name, pool, figures)
    assert set(norms) == {k for k, v in ref["grad_l2"].items() if v is not None}
    assert ("encoder.cls_token" in norms) == (pool == "cls")
    assert all(v <= 1e-5 for v in figures.values()), figures


def test_host_refusals_launch_nothing():
    """Every refusal is SFCVIT_EINVAL with a message, decided before any HIP call: this machine has no GPU, so a launch
    attempt would come back as a launch error (status 2), not as status 1."""
    from sfcvit._lib import lib
    raw = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(raw) + 15) // 16 * 16                # 16-byte aligned host addresses: never dereferenced
    q = p + (1 << 15)                                          # a second buffer, far enough for every shape below
    big = 1 << 30

    def pre(x=p, cls=p, y=q, B=2, N=5, D=16):
        return lib.sfcvit_cls_prepend_fwd(x, cls, y, B, N, D, None)

    def preb(dy=p, dx=q, dcls=q, B=4096, N=1, D=8, ws=p, ws_bytes=big, bf16=0):
        return lib.sfcvit_cls_prepend_bwd(dy, dx, dcls, bf16, B, N, D, ws, ws_bytes, None)

    def pool(x=p, y=q, B=2, N=5, D=16, first=0, count=5):
        return lib.sfcvit_token_pool_fwd(x, y, B, N, D, first, count, None)

    def poolb(dy=p, dx=q, B=2, N=5, D=16, first=0, count=5):
        return lib.sfcvit_token_pool_bwd(dy, dx, B, N, D, first, count, None)

    def refused(rc, word):
        msg = lib.sfcvit_last_error().decode()
        print(rc, msg)
        assert rc == EINVAL and word in msg, (rc, msg)

    for f, names in ((pre, ("x", "cls", "y")), (preb, ("dy", "dcls")), (pool, ("x", "y")), (poolb, ("dy", "dx"))):
        for n in names:
            refused(f(**{n: None}), "null")
        refused(f(D=4), "D=4")
        refused(f(D=12), "D=12")
        refused(f(D=0), "D=0")
        refused(f(B=0), "B=0")
        refused(f(N=0), "=0")
        refused(f(B=2 ** 31 - 1, N=2 ** 31 - 1, D=2 ** 31 - 8), "int64")
    refused(pre(x=p + 2), "aligned")
    refused(pre(cls=p + 8), "aligned")
    refused(pre(y=q + 8), "aligned")
    refused(pre(y=p), "overlaps")                              # y must not be x ...
    refused(pre(x=q + 16), "overlaps")                         # ... nor hold it: [q + 16, q + 16 + 320) inside [q, q + 384)
    refused(pre(y=p + 2 * 5 * 16 * 2 - 16), "overlaps")        # ... nor start inside it
    refused(preb(dy=p + 2), "aligned")
    refused(preb(dx=q + 8), "aligned")
    refused(preb(ws=p + 4), "aligned")
    refused(pool(x=p + 2), "aligned")
    refused(poolb(dx=q + 4), "aligned")
    for f in (pool, poolb):                                    # 0 <= first, count >= 1, first + count <= T
        for first, count in ((-1, 1), (0, 0), (0, -1), (0, 6), (5, 1), (3, 3), (2 ** 31 - 1, 2 ** 31 - 1)):
            refused(f(first=first, count=count), "range")
    # the workspace: none up to 2048 images, whole fp32 rows of D above
    need = lib.sfcvit_cls_prepend_bwd_workspace(4096, 1, 8)
    assert need == 2 * 8 * 4
    refused(preb(ws_bytes=need - 1), "workspace")
    refused(preb(ws=None), "workspace")
    assert lib.sfcvit_cls_prepend_bwd_workspace(67, 3, 12) == 0 and lib.sfcvit_cls_prepend_bwd_workspace(0, 3, 8) == 0
    for shape in ((256, 196, 768), (64, 576, 1024), (3, 5, 72), (1, 1, 8), (67, 3, 8), (2048, 1, 8)):
        assert lib.sfcvit_cls_prepend_bwd_workspace(*shape) == 0, shape
    for B in (2049, 4096, 4097, 100000):
        assert lib.sfcvit_cls_prepend_bwd_workspace(B, 2, 24) == -(-B // 2048) * 24 * 4, B
    buf = ctypes.create_string_buffer(96)
    assert lib.sfcvit_last_token_pool_kernel(buf, 96) == 0 and buf.value == b"none"     # nothing was launched
    assert lib.sfcvit_last_token_pool_kernel(None, 96) == EINVAL


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


def test_with_cls_token_against_a_hand_built_mask():
    from sfcvit import masks
    ninf = float("-inf")
    window = masks.curve_window(3, 0)                          # the diagonal alone
    want = torch.tensor([[0.0, 0.0, 0.0, 0.0],
                         [0.0, 0.0, ninf, ninf],
                         [0.0, ninf, 0.0, ninf],
                         [0.0, ninf, ninf, 0.0]])
    got = masks.with_cls_token(window)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(masks.with_cls_token(~torch.eye(3, dtype=torch.bool)), want)        # bool: True = blocked
    soft = torch.tensor([[0.0, -1.5], [2.0, 0.0]])
    assert torch.equal(masks.with_cls_token(soft), torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, -1.5], [0.0, 2.0, 0.0]]))
    with pytest.raises(ValueError, match="square"):
        masks.with_cls_token(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="float additive or a bool"):
        masks.with_cls_token(torch.zeros(3, 3, dtype=torch.int32))


@pytest.mark.parametrize("name", CASES)
def test_pool_keyword_surface(name, golden_dir):
    """pool=None: the parent's manifest, key for key, and the parent's seeded values.  "cls" / "mean": the factorised head's
    four tensors leave, the pooled head's two arrive (mlp_head.0.* keep their keys), "cls" adds encoder.cls_token [1, 1, D]
    of zeros; everything in front of the head draws what it draws today."""
    cfg, _ = MODEL_CASES[name]
    with open(os.path.join(golden_dir, "state_manifest.json")) as f:
        manifest = json.load(f)[name]
    torch.manual_seed(7)
    base = build_model(cfg).state_dict()
    torch.manual_seed(7)
    none = build_with(cfg, pool=None)
    sd = none.state_dict()
    assert sorted(sd) == sorted(manifest)
    assert all(list(v.shape) == manifest[k][0] and str(v.dtype).replace("torch.", "") == manifest[k][1] for k, v in sd.items())
    assert list(sd) == list(base) and all(torch.equal(sd[k], base[k]) for k in sd)
    assert not hasattr(none.encoder, "cls_token") and type(none.mlp_head).__name__ == "MultiLayerPredictor"
    for pool in POOLS:
        torch.manual_seed(7)
        model = build_with(cfg, pool=pool)
        sd = model.state_dict()
        gone = {"mlp_head.1.W_emb", "mlp_head.1.W_seq", "mlp_head.4.weight", "mlp_head.4.bias"}
        new = {"mlp_head.1.weight", "mlp_head.1.bias"} | ({"encoder.cls_token"} if pool == "cls" else set())
        assert set(base) - set(sd) == gone and set(sd) - set(base) == new
        assert all(torch.equal(sd[k], base[k]) for k in sd if k in base and not k.startswith("mlp_head.")), "another initial value changed"
        assert type(model.mlp_head).__name__ == "PooledHead" and isinstance(model.mlp_head, torch.nn.Sequential)
        assert list(sd["mlp_head.1.weight"].shape) == [cfg.num_classes, cfg.embed_dim]
        assert set(sd) == set(pooled_state(cfg, pool))         # what the fixture's state loads into
        model.load_state_dict(pooled_state(cfg, pool))
        if pool == "cls":
            tok = model.encoder.cls_token
            assert isinstance(tok, torch.nn.Parameter) and tok.requires_grad and list(tok.shape) == [1, 1, cfg.embed_dim]
            assert [k for k, _ in model.encoder.named_parameters(recurse=False)] == ["cls_token"]
            torch.manual_seed(7)
            assert float(build_with(cfg, pool=pool).encoder.cls_token.detach().abs().max()) == 0.0
        else:
            assert not hasattr(model.encoder, "cls_token")


def test_pool_value_errors():
    from sfcvit import masks
    from sfcvit.models import TransformerSeqEncoder, VisionTransformer, VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    for cls in (VisionTransformer, VisionTransformer1D):
        pe = HilbertEmbedding1D(32, 256, 3, 32)
        for bad in ("max", "CLS", True, 0):
            with pytest.raises(ValueError, match="'cls', 'mean'"):
                cls(pe, depth=1, n_heads=2, mlp_dim=32, pool=bad)
        for pool in POOLS:
            with pytest.raises(ValueError, match="multiple of 8"):
                cls(HilbertEmbedding1D(32, 256, 3, 36), depth=1, n_heads=2, mlp_dim=32, pool=pool)
        n = pe.n_patches
        with pytest.raises(ValueError, match="with_cls_token"):
            cls(pe, depth=1, n_heads=2, mlp_dim=32, pool="cls", attn_mask=masks.curve_window(n, 1))
        with pytest.raises(ValueError, match=f"{n + 1} tokens"):
            cls(pe, depth=1, n_heads=2, mlp_dim=32, pool="mean", attn_mask=masks.with_cls_token(masks.curve_window(n, 1)))
    with pytest.raises(ValueError, match="multiple of 8"):
        TransformerSeqEncoder(36, 4, 2, 32, None, cls_token=True)


def test_cpu_tensors_and_wrong_shapes_are_refused_by_the_python_layers():
    from sfcvit import functional as F
    from sfcvit._lib import SfcvitError
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        F.cls_prepend(torch.zeros(2, 5, 16), torch.zeros(1, 1, 16))
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        F.token_pool(torch.zeros(2, 5, 16))
    with pytest.raises(ValueError, match="token"):
        F.cls_prepend(torch.zeros(2, 5, 16), torch.zeros(1, 1, 8))
    with pytest.raises(ValueError, match="token"):
        F.cls_prepend(torch.zeros(2, 5, 16), torch.zeros(1, 16))
    for first, count in ((0, 0), (3, 3), (-1, 2), (5, None)):
        with pytest.raises(ValueError, match="range"):
            F.token_pool(torch.zeros(2, 5, 16), first, count)


@pytest.mark.parametrize("N,H", [(4, 3), (196, 12), (576, 16)])
def test_attention_plans_accept_the_cls_sequence(N, H):
    """sfcvit_attention_plan (host only) takes N + 1 tokens at head dim 64, forward and backward: 5 and 197 tokens stay on the
    whole-sequence forward and the one-pass backward (<= 224), 577 on the sequence-resident kernels (<= 608)."""
    from test_attention_stream_cpu import plan
    for bwd in (False, True):
        rc, with_cls = plan(8, N + 1, H, 64, bwd, False)
        rc0, without = plan(8, N, H, 64, bwd, False)
        print(f"N + 1 = {N + 1} H = {H} {'backward' if bwd else 'forward'}: {with_cls}   (N = {N}: {without})")
        assert rc == 0 and rc0 == 0, (with_cls, without)
        assert ("long" in with_cls) == (N + 1 > 224), with_cls
