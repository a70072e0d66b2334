"""Positional embeddings without a GPU: the fixture against an fp64 restatement, the host-side refusals of
sfcvit_pos_embed_* (decided before any HIP call), the module / state_dict surface of the models' `pos_embed` keyword, the
fixed tables and permute_pos_embed."""
import ctypes

import pytest
import torch

from oracle.cases import MODEL_CASES
from pos_embed_ref import build_with, load_fixture, model_ref, sincos1d_ref, sincos2d_ref
from test_host_cpu import build_model

EINVAL = 1
CASES = ["raster32_2d", "hilbert32_1d"]


def _rel(got, ref):
    return float((got.double().flatten() - ref.double().flatten()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize("name", CASES)
def test_fixture_equals_the_fp64_statement(name):
    """The reference models' fp32 logits, loss and gradients with the table added after the tokenizer
    (tests/golden/pos_embed.json) against the same forward in fp64 (pos_embed_ref.model_ref): 1e-5 relative to max |value|."""
    case, ref = load_fixture()["cases"][name], model_ref(name)
    figures = {"logits": _rel(torch.tensor(case["logits"]), ref["logits"]),
               "loss": abs(case["loss"] - ref["loss"]) / abs(ref["loss"]),
               "table_grad": _rel(torch.tensor(case["table_grad"]), ref["table_grad"])}
    norms = {k: v for k, v in case["grad_l2"].items() if v is not None}
    top = max(ref["grad_l2"][k] for k in norms)
    figures["grad_l2"] = max(abs(v - ref["grad_l2"][k]) for k, v in norms.items()) / top
    print(name, figures)
    assert set(norms) == {k for k, v in ref["grad_l2"].items() if v is not None}
    assert all(v <= 1e-5 for v in figures.values()), figures


def test_host_refusals_launch_nothing():
    """Every refusal is SFCVIT_EINVAL with a message, decided before any HIP call: this machine has no GPU, so a launch
    attempt would come back as a launch error (status 2), not as status 1."""
    from sfcvit import _lib
    from sfcvit._lib import lib
    raw = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(raw) + 15) // 16 * 16                # a 16-byte aligned host address: never dereferenced
    big = 1 << 30
    split = (67, 3, 8)                                         # a shape whose plan splits the batch: workspace > 0

    def fwd(x=p, pos=p, y=p, B=2, N=5, D=16):
        return lib.sfcvit_pos_embed_fwd(x, pos, y, B, N, D, None)

    def bwd(dy=p, dpos=p, B=67, N=3, D=8, ws=p, ws_bytes=big, bf16=0):
        return lib.sfcvit_pos_embed_bwd(dy, dpos, bf16, B, N, D, ws, ws_bytes, None)

    def refused(rc, word):
        msg = lib.sfcvit_last_error().decode()
        print(rc, msg)
        assert rc == EINVAL and word in msg, (rc, msg)

    refused(fwd(x=None), "null")
    refused(fwd(pos=None), "null")
    refused(fwd(y=None), "null")
    refused(bwd(dy=None), "null")
    refused(bwd(dpos=None), "null")
    for f in (fwd, bwd):
        refused(f(D=4), "D=4")
        refused(f(D=12), "D=12")
        refused(f(D=0), "D=0")
        refused(f(B=0), "B=0")
        refused(f(N=0), "N=0")
    refused(fwd(x=p + 2), "aligned")
    refused(fwd(y=p + 8), "aligned")
    refused(bwd(dy=p + 2), "aligned")
    refused(bwd(ws=p + 4), "aligned")
    refused(fwd(B=2 ** 31 - 1, N=2 ** 31 - 1, D=2 ** 31 - 8), "int64")
    need = lib.sfcvit_pos_embed_bwd_workspace(*split)
    assert need > 0 and need % (4 * split[1] * split[2]) == 0          # whole fp32 partial rows of the [N D] table
    refused(bwd(ws_bytes=need - 1), "workspace")
    refused(bwd(ws=None), "workspace")
    # consistent with the plan: refused shapes need nothing, and a shape whose table alone fills the GPU needs nothing
    assert lib.sfcvit_pos_embed_bwd_workspace(67, 3, 12) == 0 and lib.sfcvit_pos_embed_bwd_workspace(0, 3, 8) == 0
    for shape in ((256, 196, 768), (64, 576, 1024), (3, 5, 72), (1, 1, 8)):
        assert lib.sfcvit_pos_embed_bwd_workspace(*shape) == 0, shape
    for B in (31, 32, 63, 64, 67, 512, 4096):                  # the split keeps >= 32 images per range and 8 | rows
        need = lib.sfcvit_pos_embed_bwd_workspace(B, 3, 8)
        splits = need // (4 * 24)
        assert need == splits * 4 * 24 and splits != 1 and splits <= max(B // 32, 1), (B, need)
        assert (splits == 0) == (B < 64), (B, need)
    for name in ("sfcvit_pos_embed_fwd", "sfcvit_pos_embed_bwd", "sfcvit_pos_embed_bwd_workspace", "sfcvit_last_pos_embed_kernel"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    buf = ctypes.create_string_buffer(96)
    assert lib.sfcvit_last_pos_embed_kernel(buf, 96) == 0 and buf.value == b"none"     # nothing was launched
    assert lib.sfcvit_abi_version() == 1


def test_cpu_tensors_and_wrong_tables_are_refused_by_the_python_layers():
    from sfcvit import functional as F
    from sfcvit._lib import SfcvitError
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        F.pos_embed(torch.zeros(2, 5, 16), torch.zeros(1, 5, 16))
    with pytest.raises(ValueError, match="5 tokens.*table 4"):
        F.pos_embed(torch.zeros(2, 5, 16), torch.zeros(1, 4, 16))
    with pytest.raises(ValueError, match="expected"):
        F.pos_embed(torch.zeros(2, 5, 16), torch.zeros(2, 5, 16))


@pytest.mark.parametrize("name", CASES)
def test_module_surface(name):
    """Default: today's keys and seeded values.  "learned": exactly one more key, a Parameter [1, N, D] drawn LAST (the
    fixture's head and sum of torch.randn after the reference model's construction).  "sincos*": a persistent buffer
    under that key, no parameter.  Every other initial value is the same with and without the option."""
    cfg, _ = MODEL_CASES[name]
    init = load_fixture()["init"][name]
    n, d = cfg.n_patches, cfg.embed_dim
    torch.manual_seed(init["seed"])
    base = build_model(cfg)
    base_sd = base.state_dict()
    assert "pos_embed" not in base_sd and not hasattr(base, "pos_embed")
    for off in (None, False):
        torch.manual_seed(init["seed"])
        sd = build_with(cfg, pos_embed=off).state_dict()
        assert list(sd) == list(base_sd) and all(torch.equal(sd[k], base_sd[k]) for k in sd)
    for kind in ("learned", "sincos1d", "sincos2d"):
        torch.manual_seed(init["seed"])
        model = build_with(cfg, pos_embed=kind)
        sd = model.state_dict()
        assert sorted(set(sd) - set(base_sd)) == ["pos_embed"] and set(base_sd) <= set(sd)
        assert all(torch.equal(sd[k], base_sd[k]) for k in base_sd), "the option changed another parameter's initial value"
        assert list(sd["pos_embed"].shape) == [1, n, d] and sd["pos_embed"].dtype == torch.float32
        params = dict(model.named_parameters())
        if kind == "learned":
            assert isinstance(model.pos_embed, torch.nn.Parameter) and params["pos_embed"].requires_grad
            print(kind, sd["pos_embed"].flatten()[:8].tolist(), float(sd["pos_embed"].double().sum()))
            assert sd["pos_embed"].flatten()[:8].tolist() == init["head"]
            assert float(sd["pos_embed"].double().sum()) == init["sum"]
        else:
            assert "pos_embed" not in params and "pos_embed" in dict(model.named_buffers())
            assert not model.pos_embed.requires_grad
            fresh = build_model(cfg)                            # a checkpoint of the fixed table loads where the keyword is set
            with pytest.raises(RuntimeError, match="pos_embed"):
                fresh.load_state_dict(sd)
            other = build_with(cfg, pos_embed=kind)
            other.pos_embed.zero_()
            other.load_state_dict(sd)
            assert torch.equal(other.pos_embed, model.pos_embed)
    torch.manual_seed(init["seed"])
    half = build_with(cfg, pos_embed="learned", pos_embed_std=0.5).state_dict()["pos_embed"]
    torch.manual_seed(init["seed"])
    assert torch.equal(half, build_with(cfg, pos_embed="learned").state_dict()["pos_embed"] * 0.5)
    with pytest.raises(ValueError, match="learned"):
        build_with(cfg, pos_embed="rope")


def test_learned_table_follows_the_aggregator():
    """Constructed last, after `ta`: with both options the aggregator draws what it draws alone."""
    cfg, _ = MODEL_CASES["hilbert32_1d"]
    torch.manual_seed(3)
    ta = build_with(cfg, token_aggregator=True).state_dict()
    torch.manual_seed(3)
    both = build_with(cfg, token_aggregator=True, pos_embed="learned").state_dict()
    assert sorted(set(both) - set(ta)) == ["pos_embed"] and set(ta) <= set(both)
    assert all(torch.equal(both[k], ta[k]) for k in ta)


def _grid_tokenizers(d=16):
    from sfcvit.curves import hilbert_curve, z_curve
    from sfcvit.tokenizers import RasterScan1DGroupedEmbedding, SFCEmbedding1D
    return (SFCEmbedding1D(32, 4, 1, 3, d, hilbert_curve), SFCEmbedding1D(32, 4, 1, 3, d, z_curve),
            RasterScan1DGroupedEmbedding(32, 4, 1, 3, d))


def test_sincos_tables():
    """sincos1d: the fixture's values (the reference's own function, whose fp32 angles p * w <= 4 carry ~2^-24 relative
    error each: 2e-6 absolute is eight such steps) and the fp64 formula rounded once (exact).  sincos2d: the fp64
    formula of the token centres rounded once (exact); the Hilbert tokenizer's table is the raster tokenizer's permuted
    by the curve's token order (exact), and it is not the 1-D table."""
    from sfcvit.models import VisionTransformer
    from sfcvit.models.altvit import posemb_sincos_1d
    gold = torch.tensor(load_fixture()["sincos1d_5_16"]).reshape(5, 16)
    ours = posemb_sincos_1d(5, 16)
    print("sincos1d vs the reference", float((ours - gold).abs().max()))
    assert float((ours - gold).abs().max()) <= 2e-6
    hil, _, ras = _grid_tokenizers(16)
    models = {k: {kind: VisionTransformer(pe, depth=1, n_heads=2, mlp_dim=32, pos_embed=kind) for kind in ("sincos1d", "sincos2d")}
              for k, pe in (("hilbert", hil), ("raster", ras))}
    n = hil.n_patches
    for k in models:
        assert torch.equal(models[k]["sincos1d"].pos_embed[0], sincos1d_ref(n, 16).float())
    grid = 32 // 4
    raster_pos = torch.tensor([[(t // grid) * 4 + 1.5, (t % grid) * 4 + 1.5] for t in range(n)])
    t_ras, t_hil = models["raster"]["sincos2d"].pos_embed[0], models["hilbert"]["sincos2d"].pos_embed[0]
    assert torch.equal(t_ras, sincos2d_ref(raster_pos, 16).float())
    order = hil.sfc_indices                                     # token t of the Hilbert tokenizer is raster patch order[t]
    assert not torch.equal(order, torch.arange(n))
    assert torch.equal(t_hil, t_ras[order])
    assert not torch.equal(t_hil, models["hilbert"]["sincos1d"].pos_embed[0])
    assert not torch.equal(t_hil, t_ras)


def test_sincos2d_needs_fixed_positions():
    from sfcvit.models import VisionTransformer
    from sfcvit.tokenizers import RandomEmbedding
    with pytest.raises(ValueError, match="new token order"):
        VisionTransformer(RandomEmbedding(32, 8, 3, 32), depth=1, n_heads=2, mlp_dim=32, pos_embed="sincos2d")


def test_width_rule_is_checked_at_construction():
    from sfcvit.models import VisionTransformer, VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    for cls in (VisionTransformer, VisionTransformer1D):
        for kind in ("learned", "sincos1d", "sincos2d"):
            with pytest.raises(ValueError, match="multiple of 8"):
                cls(HilbertEmbedding1D(32, 256, 3, 36), depth=1, n_heads=2, mlp_dim=32, pos_embed=kind)
        cls(HilbertEmbedding1D(32, 256, 3, 36), depth=1, n_heads=2, mlp_dim=32)          # without the option any width goes


def test_permute_pos_embed():
    from sfcvit.models import permute_pos_embed
    from sfcvit.tokenizers import RasterScan1DEmbedding, SFCEmbedding1D
    hil, z, ras = _grid_tokenizers(8)
    n = hil.n_patches
    table = torch.arange(n * 8, dtype=torch.float32).reshape(1, n, 8)
    to_z = permute_pos_embed(table, hil, z)
    assert to_z.shape == table.shape and not torch.equal(to_z, table)
    assert torch.equal(permute_pos_embed(to_z, z, hil), table)
    to_ras = permute_pos_embed(to_z, z, ras)
    assert torch.equal(to_ras[0][hil.sfc_indices], table[0])    # raster row of the patch Hilbert token t covers = row t
    assert torch.equal(permute_pos_embed(to_ras, ras, hil), table)
    assert torch.equal(permute_pos_embed(table[0], hil, z), to_z[0])      # [N, D] as well
    with pytest.raises(ValueError, match="tokens"):
        permute_pos_embed(table, hil, SFCEmbedding1D(32, 8, 1, 3, 8))     # 16 tokens against 64
    with pytest.raises(ValueError, match="centres"):
        permute_pos_embed(table, hil, RasterScan1DEmbedding(32, 16, 3, 8))      # 64 tokens, but strips of 16 pixels of a row
    with pytest.raises(ValueError, match="rows"):
        permute_pos_embed(table[:, :5], hil, z)
