"""The token-mix branch of MixerBlock without a GPU: the fixture against an fp64 restatement, the model surface with and
without the option, and the host-side refusals of sfcvit_tokmix_left / _wgrad (decided before any HIP call)."""
import ctypes
import os

import pytest
import torch

from oracle.cases import MODEL_CASES
from token_mix_ref import CM_KEYS, TM_KEYS, case_inputs, case_shapes, load_fixture, mixer_ref, unpack

EINVAL = 1


def _rel(got, ref):
    return float((got.double().flatten() - ref.double().flatten()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize("idx", [0, 1])
def test_fixture_equals_the_fp64_statement(idx):
    """The reference modules' fp32 outputs and gradients (tests/golden/token_mix.json, computed on the transposed
    activation as vit.py:269-271 spells it) against plain einsum along the token axis in fp64: rtol 1e-4 of max |value|,
    the bar of test_oracle_golden.py."""
    case = load_fixture()["cases"][idx]
    B, N, D, hid = case["B"], case["N"], case["D"], case["hid"]
    x, cot, sd = case_inputs(B, N, D, hid)
    y, dx, grads = mixer_ref(x, sd, cot)
    y_tm, _, _ = mixer_ref(x, sd, cot, channel_mix=False)
    figures = {"y": _rel(unpack(case["y"], (B, N, D)), y), "dx": _rel(unpack(case["dx"], (B, N, D)), dx),
               "y_token_mix": _rel(unpack(case["y_token_mix"], (B, N, D)), y_tm)}
    shapes = case_shapes(N, D, hid)
    for key, g in grads.items():
        figures[key] = _rel(unpack(case["grads"][key], shapes[key]), g)
    print(figures)
    assert set(case["grads"]) == set(grads) == set(TM_KEYS) | set(CM_KEYS)
    assert all(v <= 1e-4 for v in figures.values()), figures


def test_fixture_is_small_and_names_the_keys_that_gain_gradients():
    from token_mix_ref import GOLDEN
    assert os.path.getsize(GOLDEN) < 100_000
    gains = load_fixture()["gains_grad"]
    one_d = [name for name, (cfg, _) in MODEL_CASES.items() if cfg.variant == "1d" and name in gains]
    assert one_d
    for name, keys in gains.items():
        want = sorted("mlp_mixer." + k for k in TM_KEYS) if name in one_d else []
        assert keys == want, name


def _model(name, **kw):
    from sfcvit.models import VisionTransformer1D
    from sfcvit.tokenizers import HilbertEmbedding1D
    cfg, _ = MODEL_CASES[name]
    torch.manual_seed(7)
    pe = HilbertEmbedding1D(cfg.img_size, cfg.patch_size, cfg.in_channels, cfg.embed_dim)
    return VisionTransformer1D(pe, depth=cfg.depth, n_heads=cfg.n_heads, mlp_dim=cfg.mlp_dim, num_classes=cfg.num_classes, **kw)


def test_the_option_changes_no_key_and_no_seeded_value():
    import sfcvit.models.vit as vit
    import src.models.vit as refpath
    assert refpath.MixerBlock is vit.MixerBlock and refpath.VisionTransformer1D is vit.VisionTransformer1D
    base, on = _model("hilbert32_1d").state_dict(), _model("hilbert32_1d", token_mix=True).state_dict()
    assert list(base) == list(on)
    assert all(torch.equal(base[k], on[k]) for k in base)
    assert all("mlp_mixer." + k in base for k in TM_KEYS)
    torch.manual_seed(3)
    a = vit.MixerBlock(5, 16, 32, 16).state_dict()
    torch.manual_seed(3)
    b = vit.MixerBlock(5, 16, 32, 16, token_mix=True).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert vit.MixerBlock(5, 16, 32, 16).use_token_mix is False


def test_a_changed_token_count_is_refused():
    from sfcvit.models import MixerBlock
    with pytest.raises(ValueError, match="token count"):
        MixerBlock(5, 16, 32, 16, token_mix=True)(torch.zeros(2, 3, 16))


def test_host_refusals_launch_nothing():
    """Every refusal is SFCVIT_EINVAL with a message, decided before any HIP call: this machine has no GPU, so a launch
    attempt would come back as a launch error (status 2), not as status 1."""
    from sfcvit import _lib
    from sfcvit._lib import lib
    raw = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(raw) + 15) // 16 * 16                # a 16-byte aligned host address: never dereferenced
    big = 1 << 30

    def left(w=p, x=p, c=p, bias=None, residual=None, aux_in=None, aux_out=None, B=2, M=32, K=5, D=16, tr=0, act=0):
        a = _lib.TokmixArgs()
        a.w, a.x, a.c, a.bias, a.residual, a.aux_in, a.aux_out = w, x, c, bias, residual, aux_in, aux_out
        a.B, a.M, a.K, a.D, a.w_transposed, a.act = B, M, K, D, tr, act
        return lib.sfcvit_tokmix_left(ctypes.byref(a), None)

    def wgrad(g=p, x=p, dw=p, db=p, B=2, M=32, K=5, D=16, ws=p, ws_bytes=big):
        return lib.sfcvit_tokmix_wgrad(g, x, dw, db, 0, B, M, K, D, ws, ws_bytes, None)

    def refused(rc, word):
        msg = lib.sfcvit_last_error().decode()
        assert rc == EINVAL and word in msg, (rc, msg)

    refused(lib.sfcvit_tokmix_left(None, None), "null")
    refused(left(w=None), "null")
    refused(left(x=None), "null")
    refused(left(c=None), "null")
    refused(wgrad(g=None), "null")
    refused(wgrad(x=None), "null")                             # dw needs x
    refused(wgrad(dw=None, db=None), "NULL")
    for f in (left, wgrad):
        refused(f(D=12), "D=12")
        refused(f(D=0), "D=0")
        refused(f(M=36, K=5), "hidden width")                  # hid = 36: neither extent is a multiple of 8
        refused(f(M=5, K=36), "hidden width")
        refused(f(K=0), "K=0")                                 # N <= 0, as the contracted extent ...
        refused(f(M=0, K=32), "M=0")                           # ... and as the output extent
        refused(f(K=-3), "K=-3")
        refused(f(B=0), "B=0")
        refused(f(x=p + 2), "aligned")
    refused(left(c=p + 8), "aligned")
    refused(left(residual=p + 4), "aligned")
    refused(left(w=p + 1), "aligned")
    refused(left(act=1), "act=1")                              # ReLU is not part of this epilogue
    need = lib.sfcvit_tokmix_wgrad_workspace(2, 32, 5, 16)
    assert need == 2 * (32 * 5 + 32) * 4                        # one partial row [M K | M] per image at this size
    refused(wgrad(ws_bytes=need - 1), "workspace")
    refused(wgrad(ws=None), "workspace")
    refused(wgrad(ws=p + 4), "aligned")
    assert lib.sfcvit_tokmix_wgrad_workspace(2, 32, 5, 12) == 0
    assert lib.sfcvit_tokmix_wgrad_workspace(2, 36, 5, 16) == 0
    assert lib.sfcvit_tokmix_wgrad_workspace(2, 32, 0, 16) == 0
    # many images share a range once the tile count times the batch exceeds the device: never more than 64 rows
    assert lib.sfcvit_tokmix_wgrad_workspace(4096, 32, 5, 16) == 64 * (32 * 5 + 32) * 4
    # the header, sfcvit/_lib.py and the library agree on the new entry points
    for name in ("sfcvit_tokmix_left", "sfcvit_tokmix_wgrad", "sfcvit_tokmix_wgrad_workspace", "sfcvit_last_tokmix_kernel"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "sfcvit.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in ("sfcvit_tokmix_left", "sfcvit_tokmix_wgrad", "sfcvit_tokmix_wgrad_workspace",
                                                 "sfcvit_last_tokmix_kernel"))
    assert "#define SFCVIT_ABI_VERSION 1" in header and lib.sfcvit_abi_version() == 1
    buf = ctypes.create_string_buffer(96)
    assert lib.sfcvit_last_tokmix_kernel(buf, 96) == 0 and buf.value == b"none"      # nothing was launched above


def test_cpu_tensors_are_refused_by_the_python_layers():
    from sfcvit import functional as F
    from sfcvit import ops
    from sfcvit._lib import SfcvitError
    from sfcvit.models import MixerBlock
    bf = torch.bfloat16
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        MixerBlock(5, 16, 32, 16, token_mix=True)(torch.zeros(2, 5, 16))
    z = torch.zeros
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        F.token_mix(z(2, 5, 16), z(16), z(16), z(32, 5), z(32), z(5, 32), z(5))
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        ops.tokmix_left(z(32, 5, dtype=bf), z(2, 5, 16, dtype=bf))
    with pytest.raises(SfcvitError, match="no CPU fallback"):
        ops.tokmix_wgrad(z(2, 32, 16, dtype=bf), z(2, 5, 16, dtype=bf))
    with pytest.raises(ValueError, match="multiples of 8"):
        F.token_mix(z(2, 5, 16), z(16), z(16), z(36, 5), z(36), z(5, 36), z(5))
    with pytest.raises(ValueError, match="token count"):
        F.token_mix(z(2, 6, 16), z(16), z(16), z(32, 5), z(32), z(5, 32), z(5))
