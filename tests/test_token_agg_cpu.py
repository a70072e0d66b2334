"""TokenAggregator without a GPU: the fixture against an fp64 restatement, the module / state_dict surface, and the
host-side refusals of sfcvit_dwconv1d_* (decided before any HIP call)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from oracle.cases import MODEL_CASES
from test_host_cpu import build_model
from token_agg_ref import aggregator_ref, case_inputs, load_fixture

EINVAL = 1


def _rel(got, ref):
    return float((got.double().flatten() - ref.double().flatten()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize("idx", [0, 1])
def test_fixture_equals_the_fp64_statement(idx):
    """The reference module's fp32 outputs and gradients (tests/golden/token_aggregator.json) against conv1d on the
    transposed input -> linear -> erf-GELU -> layer_norm in fp64, written here: 1e-5 relative to max |value|."""
    case = load_fixture()["cases"][idx]
    B, N, D, k = case["B"], case["N"], case["D"], case["k"]
    x, cot, sd = case_inputs(B, N, D, k)
    y, dx, grads = aggregator_ref(x, sd, cot)
    figures = {"y": _rel(torch.tensor(case["y"]), y), "dx": _rel(torch.tensor(case["dx"]), dx)}
    for key, g in grads.items():
        figures[key] = _rel(torch.tensor(case["grads"][key]), g)
    print(figures)
    assert set(case["grads"]) == set(grads)
    assert all(v <= 1e-5 for v in figures.values()), figures


def test_module_surface_matches_the_manifest():
    import sfcvit.models.vit as vit
    import src.models.vit as refpath
    assert refpath.TokenAggregator is vit.TokenAggregator
    init = load_fixture()["init"]
    torch.manual_seed(init["seed"])
    mod = vit.TokenAggregator(init["dim"])
    sd = mod.state_dict()
    assert {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()} == init["keys"]
    for k, v in sd.items():                                   # same constructors in the same order: same seeded values
        assert v.flatten()[:8].tolist() == init["head"][k], k
        assert float(v.double().sum()) == init["sum"][k], k
    mod = vit.TokenAggregator(16, 5, 2)                       # the reference's constructor (dim, k, s)
    assert mod.dw.kernel_size == (5,) and mod.dw.stride == (2,) and mod.dw.padding == (2,) and mod.dw.groups == 16


@pytest.mark.parametrize("name", ["hilbert32_1d", "raster32_2d"])
def test_models_gain_exactly_the_ta_keys(name):
    from sfcvit.models import VisionTransformer, VisionTransformer1D
    cfg, _ = MODEL_CASES[name]
    gold = load_fixture()["model_keys"]
    torch.manual_seed(7)
    base = build_model(cfg).state_dict()
    torch.manual_seed(7)
    again = build_model(cfg).state_dict()
    assert list(base) == list(again) and all(torch.equal(base[k], again[k]) for k in base)
    assert not any(k.startswith("ta.") for k in base)
    cls = VisionTransformer1D if cfg.variant == "1d" else VisionTransformer
    for option, k in ((True, 3), (5, 5)):
        torch.manual_seed(7)
        sd = _with_option(cfg, cls, option).state_dict()
        assert sorted(set(sd) - set(base)) == sorted(gold["keys"])
        assert set(base) <= set(sd)
        assert all(torch.equal(sd[k2], base[k2]) for k2 in base), "the option changed another parameter's initial value"
        assert list(sd["ta.dw.weight"].shape) == [cfg.embed_dim, 1, k]
    with pytest.raises(ValueError, match="odd"):
        _with_option(cfg, cls, 4)


def _with_option(cfg, cls, option):
    """build_model(cfg) (test_host_cpu) with token_aggregator=option: same tokenizer construction, same argument order."""
    import sfcvit.models as models
    orig = {n: getattr(models, n) for n in ("VisionTransformer", "VisionTransformer1D")}

    def patched(c):
        return lambda pe, **kw: c(pe, token_aggregator=option, **kw)
    try:
        for n, c in orig.items():
            setattr(models, n, patched(c))
        return build_model(cfg)
    finally:
        for n, c in orig.items():
            setattr(models, n, c)


def test_out_len_is_conv1d_s():
    from sfcvit._lib import lib
    for k in range(1, 10):
        for s in range(1, 5):
            conv = nn.Conv1d(1, 1, k, s, padding=k // 2)
            for N in range(1, 21):
                assert lib.sfcvit_dwconv1d_out_len(N, k, s) == conv(torch.zeros(1, 1, N)).shape[-1], (N, k, s)
    for bad in ((5, 0, 1), (5, 10, 1), (5, 3, 0), (5, 3, 5), (0, 3, 1)):
        assert lib.sfcvit_dwconv1d_out_len(*bad) < 0, bad


def test_host_refusals_launch_nothing():
    """Every refusal is SFCVIT_EINVAL with a message, decided before any HIP call: this machine has no GPU, so a launch
    attempt would come back as a launch error (status 2), not as status 1."""
    from sfcvit._lib import lib
    raw = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(raw) + 15) // 16 * 16                # a 16-byte aligned host address: never dereferenced
    big = 1 << 30

    def fwd(x=p, w=p, u=p, B=2, N=5, D=16, k=3, s=1):
        return lib.sfcvit_dwconv1d_fwd(x, w, None, u, B, N, D, k, s, None)

    def bwd(du=p, x=p, w=p, dx=p, dw=p, db=p, B=2, N=5, D=16, k=3, s=1, ws=p, ws_bytes=big):
        return lib.sfcvit_dwconv1d_bwd(du, x, w, dx, dw, db, 0, B, N, D, k, s, ws, ws_bytes, None)

    def refused(rc, word):
        msg = lib.sfcvit_last_error().decode()
        assert rc == EINVAL and word in msg, (rc, msg)

    refused(fwd(x=None), "null")
    refused(fwd(w=None), "null")
    refused(fwd(u=None), "null")
    refused(bwd(du=None), "null")
    refused(bwd(x=None), "null")                               # dw needs x
    refused(bwd(w=None), "null")                               # dx needs w
    refused(bwd(dx=None, dw=None, db=None), "NULL")
    for f in (fwd, bwd):
        refused(f(k=0), "k=0")
        refused(f(k=10), "k=10")
        refused(f(s=0), "s=0")
        refused(f(s=5), "s=5")
        refused(f(D=12), "D=12")
        refused(f(B=0), "B=0")
        refused(f(x=p + 2), "aligned")
    need = lib.sfcvit_dwconv1d_bwd_workspace(2, 5, 16, 3, 1)
    assert need > 0 and need % 4 == 0
    refused(bwd(ws_bytes=need - 1), "workspace")
    refused(bwd(ws=None), "workspace")
    assert lib.sfcvit_dwconv1d_bwd_workspace(2, 5, 12, 3, 1) == 0
    # the header, sfcvit/_lib.py and the library agree on the new entry points
    from sfcvit import _lib
    for name in ("sfcvit_dwconv1d_out_len", "sfcvit_dwconv1d_fwd", "sfcvit_dwconv1d_bwd", "sfcvit_dwconv1d_bwd_workspace",
                 "sfcvit_last_dwconv_kernel"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_cpu_tensors_are_refused_by_the_python_layers():
    from sfcvit import functional as F
    from sfcvit._lib import SfcvitError
    from sfcvit.models import TokenAggregator
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        TokenAggregator(16)(torch.zeros(2, 5, 16))
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        F.dwconv1d(torch.zeros(2, 5, 16), torch.zeros(16, 1, 3), torch.zeros(16))
