"""The two encoder layers' host side: which C entry points one forward + backward calls, in order, for every combination of
the options that changes the sequence (dropout, DropPath, masked / biased attention, a frozen bias table, activation,
LayerScale).  Sequences only: the numbers are held by test_prenorm_gpu, test_drop_path_gpu, test_dropout_gpu,
test_attention_mask_gpu, test_attention_bias_gpu and test_parity_gpu.

(B, N, D, H, F) = (2, 9, 64, 1, 128): an odd token count below one 64-token block, kernel head dim 64 (the masked and bias
kernels apply), F a multiple of 16 (the ReLU bit matrix is on).  The layers are called through encoder_layer /
pre_norm_layer with ops.next_seed replaced by a fixed list, which also pins how many seeds a call draws."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, N, D, H, FD = 2, 9, 64, 1, 128
SEEDS = (11, 22, 33, 44, 66, 1234)          # four dropout seeds, then two path seeds


class Recorder:
    """Stands in for ops.lib: every entry point called is noted by name (without the sfcvit_ prefix) and passed on.  The
    sfcvit_last_* readers are passed on unrecorded."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("sfcvit_last_"):
            return fn

        def call(*args):
            self._calls.append(name[len("sfcvit_"):])
            return fn(*args)
        return call


# case id -> (layer, keyword arguments; "mask" / "bias" / "bias_frozen" / "lam" are replaced by the objects in run_case)
CASES = {
    "post-p0": ("post", dict(dropout_p=0.0)),
    "post-p0.1": ("post", dict(dropout_p=0.1)),
    "post-p0.1-path": ("post", dict(dropout_p=0.1, drop_path=0.5)),
    "post-masked": ("post", dict(dropout_p=0.1, attn_mask="mask")),
    "post-bias": ("post", dict(dropout_p=0.1, rel_bias="bias")),
    "post-bias-frozen": ("post", dict(dropout_p=0.1, rel_bias="bias_frozen")),
    "pre-relu": ("pre", dict(dropout_p=0.1, activation="relu")),
    "pre-relu-path": ("pre", dict(dropout_p=0.1, activation="relu", drop_path=0.5)),
    "pre-relu-lam": ("pre", dict(dropout_p=0.1, activation="relu", layer_scale="lam")),
    "pre-relu-lam-path": ("pre", dict(dropout_p=0.1, activation="relu", layer_scale="lam", drop_path=0.5)),
    "pre-gelu": ("pre", dict(dropout_p=0.1, activation="gelu")),
    "pre-gelu-path": ("pre", dict(dropout_p=0.1, activation="gelu", drop_path=0.5)),
    "pre-gelu-lam": ("pre", dict(dropout_p=0.1, activation="gelu", layer_scale="lam")),
    "pre-gelu-lam-path": ("pre", dict(dropout_p=0.1, activation="gelu", layer_scale="lam", drop_path=0.5)),
    "pre-gelu-p0": ("pre", dict(dropout_p=0.0, activation="gelu")),
    "pre-relu-masked": ("pre", dict(dropout_p=0.1, activation="relu", attn_mask="mask")),
    "pre-gelu-lam-bias": ("pre", dict(dropout_p=0.1, activation="gelu", layer_scale="lam", rel_bias="bias")),
}


def run_case(case, monkeypatch):
    """One forward + backward of CASES[case] -> (the entry points called, in order; the number of seeds drawn)."""
    import sfcvit.functional as F
    from sfcvit import masks, ops, relpos
    layer, kw = CASES[case]
    g = torch.Generator(device="cuda").manual_seed(5)
    r = lambda *s, sc=1.0: (torch.randn(*s, device="cuda", generator=g) * sc).to(BF16).requires_grad_(True)     # noqa: E731
    x = r(B, N, D)
    params = [r(3 * D, D, sc=D ** -0.5), r(3 * D, sc=0.1), r(D, D, sc=D ** -0.5), r(D, sc=0.1), r(D), r(D, sc=0.1),
              r(FD, D, sc=D ** -0.5), r(FD, sc=0.1), r(D, FD, sc=FD ** -0.5), r(D, sc=0.1), r(D), r(D, sc=0.1)]
    dy, dn = r(B, N, D).detach(), r(B, N, D).detach()
    kw = dict(kw)
    if kw.get("attn_mask") == "mask":
        kw["attn_mask"] = ops.as_attention_mask(masks.curve_window(N, 4), N)
    if "rel_bias" in kw:
        idx, T = relpos.curve_offsets(N, 4)
        table = (0.5 * torch.randn(H, T, device="cuda", generator=g)).requires_grad_(kw["rel_bias"] == "bias")
        kw["rel_bias"] = (table, ops.AttentionBiasIndex(idx, T))
    if kw.get("layer_scale") == "lam":
        kw["layer_scale"] = r(2, D, sc=0.1)
    calls, seeds = [], iter(SEEDS)
    drawn = []
    monkeypatch.setattr(ops, "next_seed", lambda: drawn.append(next(seeds)) or drawn[-1])
    monkeypatch.setattr(ops, "lib", Recorder(ops.lib, calls))
    if layer == "post":
        y = F.encoder_layer(x, *params, H, **kw)
        y.backward(dy)
    else:
        n = F.layer_norm(x.detach(), params[4].detach(), params[5].detach()).requires_grad_(True)
        del calls[:]
        s2, n2 = F.pre_norm_layer(x, n, *params, H, **kw)
        torch.autograd.backward([s2, n2], [dy, dn])
    torch.cuda.synchronize()
    return calls, len(drawn)


# ---- the sequences -------------------------------------------------------------------------------------------------------------
# Recorded from the layers as they were before their shared pieces were factored out.  The *_workspace / *_ws names are the
# size queries a wrapper makes before its launch.  Forward: in_proj, attention, site 1, the MLP, site 2; backward: the
# LayerNorm after site 2, dW2, the MLP's dX (+ b1's column sums), dW1, dX of linear1, the LayerNorm after site 1, dW_out, dX
# of out_proj, attention (+ in_proj's bias column sums), dW_in, dX of in_proj.
TABLE = {
    "post-p0":
        "gemm attention_fwd_any gemm layernorm_fwd gemm gemm layernorm_fwd "
        "layernorm_bwd_ws layernorm_bwd_drop gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_ws layernorm_bwd_drop gemm gemm "
        "attention_colsum_workspace attention_bwd_any gemm gemm",
    "post-p0.1":
        "gemm attention_fwd_any gemm layernorm_fwd gemm gemm layernorm_fwd "
        "layernorm_bwd_ws layernorm_bwd_drop gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_ws layernorm_bwd_drop gemm gemm "
        "attention_colsum_workspace attention_bwd_any gemm gemm",
    "post-p0.1-path":
        "gemm attention_fwd_any gemm add_layernorm_path_fwd gemm gemm add_layernorm_path_fwd "
        "layernorm_bwd_ws layernorm_bwd_path gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_ws layernorm_bwd_path gemm gemm "
        "attention_colsum_workspace attention_bwd_any gemm gemm",
    "post-masked":
        "gemm attention_masked_fwd gemm layernorm_fwd gemm gemm layernorm_fwd "
        "layernorm_bwd_ws layernorm_bwd_drop gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_ws layernorm_bwd_drop gemm gemm "
        "attention_colsum_workspace attention_masked_bwd gemm gemm",
    "post-bias":
        "gemm attention_bias_fwd gemm layernorm_fwd gemm gemm layernorm_fwd "
        "layernorm_bwd_ws layernorm_bwd_drop gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_ws layernorm_bwd_drop gemm gemm "
        "attention_bias_workspace attention_colsum_workspace attention_bias_bwd gemm gemm",
    "post-bias-frozen":
        "gemm attention_bias_fwd gemm layernorm_fwd gemm gemm layernorm_fwd "
        "layernorm_bwd_ws layernorm_bwd_drop gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_ws layernorm_bwd_drop gemm gemm "
        "attention_colsum_workspace attention_bias_bwd gemm gemm",
    "pre-relu":
        "gemm attention_fwd_any gemm layernorm_fwd gemm gemm layernorm_fwd "
        "layernorm_bwd_ws layernorm_bwd_drop gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_ws layernorm_bwd_drop gemm gemm "
        "attention_colsum_workspace attention_bwd_any gemm gemm",
    "pre-relu-path":
        "gemm attention_fwd_any gemm add_layernorm_path_fwd gemm gemm add_layernorm_path_fwd "
        "layernorm_bwd_ws layernorm_bwd_path gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_ws layernorm_bwd_path gemm gemm "
        "attention_colsum_workspace attention_bwd_any gemm gemm",
    "pre-relu-lam":
        "gemm attention_fwd_any gemm add_layernorm_scale_fwd gemm gemm add_layernorm_scale_fwd "
        "layernorm_bwd_scale_ws layernorm_bwd_scale gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_scale_ws layernorm_bwd_scale "
        "gemm gemm attention_colsum_workspace attention_bwd_any gemm gemm",
    "pre-relu-lam-path":
        "gemm attention_fwd_any gemm add_layernorm_scale_fwd gemm gemm add_layernorm_scale_fwd "
        "layernorm_bwd_scale_ws layernorm_bwd_scale gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_scale_ws layernorm_bwd_scale "
        "gemm gemm attention_colsum_workspace attention_bwd_any gemm gemm",
    "pre-gelu":
        "gemm attention_fwd_any gemm layernorm_fwd gemm gelu_drop_fwd gemm layernorm_fwd "
        "layernorm_bwd_ws layernorm_bwd_drop gemm gemm gelu_drop_bwd colsum_workspace colsum gemm gemm layernorm_bwd_ws layernorm_bwd_drop "
        "gemm gemm attention_colsum_workspace attention_bwd_any gemm gemm",
    "pre-gelu-path":
        "gemm attention_fwd_any gemm add_layernorm_path_fwd gemm gelu_drop_fwd gemm add_layernorm_path_fwd "
        "layernorm_bwd_ws layernorm_bwd_path gemm gemm gelu_drop_bwd colsum_workspace colsum gemm gemm layernorm_bwd_ws layernorm_bwd_path "
        "gemm gemm attention_colsum_workspace attention_bwd_any gemm gemm",
    "pre-gelu-lam":
        "gemm attention_fwd_any gemm add_layernorm_scale_fwd gemm gelu_drop_fwd gemm add_layernorm_scale_fwd "
        "layernorm_bwd_scale_ws layernorm_bwd_scale gemm gemm gelu_drop_bwd colsum_workspace colsum gemm gemm layernorm_bwd_scale_ws "
        "layernorm_bwd_scale gemm gemm attention_colsum_workspace attention_bwd_any gemm gemm",
    "pre-gelu-lam-path":
        "gemm attention_fwd_any gemm add_layernorm_scale_fwd gemm gelu_drop_fwd gemm add_layernorm_scale_fwd "
        "layernorm_bwd_scale_ws layernorm_bwd_scale gemm gemm gelu_drop_bwd colsum_workspace colsum gemm gemm layernorm_bwd_scale_ws "
        "layernorm_bwd_scale gemm gemm attention_colsum_workspace attention_bwd_any gemm gemm",
    "pre-gelu-p0":
        "gemm attention_fwd_any gemm layernorm_fwd gemm gelu_fwd gemm layernorm_fwd "
        "layernorm_bwd_ws layernorm_bwd_drop gemm gemm gelu_bwd colsum_workspace colsum gemm gemm layernorm_bwd_ws layernorm_bwd_drop "
        "gemm gemm attention_colsum_workspace attention_bwd_any gemm gemm",
    "pre-relu-masked":
        "gemm attention_masked_fwd gemm layernorm_fwd gemm gemm layernorm_fwd "
        "layernorm_bwd_ws layernorm_bwd_drop gemm gemm_colsum_workspace gemm gemm gemm layernorm_bwd_ws layernorm_bwd_drop gemm gemm "
        "attention_colsum_workspace attention_masked_bwd gemm gemm",
    "pre-gelu-lam-bias":
        "gemm attention_bias_fwd gemm add_layernorm_scale_fwd gemm gelu_drop_fwd gemm add_layernorm_scale_fwd "
        "layernorm_bwd_scale_ws layernorm_bwd_scale gemm gemm gelu_drop_bwd colsum_workspace colsum gemm gemm layernorm_bwd_scale_ws "
        "layernorm_bwd_scale gemm gemm attention_bias_workspace attention_colsum_workspace attention_bias_bwd gemm gemm",
}


@pytest.mark.parametrize("case", list(CASES))
def test_entry_point_sequence(case, monkeypatch):
    calls, drawn = run_case(case, monkeypatch)
    kw = CASES[case][1]
    assert drawn == (4 if kw["dropout_p"] > 0 else 0) + (2 if kw.get("drop_path", 0) > 0 else 0)
    assert calls == TABLE[case].split(), " ".join(calls)
