"""fp64 statements of the token-mix branch of MixerBlock (src/models/vit.py:269-271) and of the two kernels under it,
shared by test_token_mix_cpu.py and test_token_mix_gpu.py.  Plain einsum on [B, N, D] as it lies in memory, no
transposes: independent of the kernels and of the fixture's generator (which runs the reference's own modules on the
transposed activation).  Every function also has an `_abs` twin returning the sums of |terms|, the scale of the error
bounds."""
import base64
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import formula

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_mix.json")
TM_KEYS = ("token_mix_ln.weight", "token_mix_ln.bias", "token_mix.0.weight", "token_mix.0.bias", "token_mix.2.weight",
           "token_mix.2.bias")
CM_KEYS = ("channel_mix_ln.weight", "channel_mix_ln.bias", "channel_mix.0.weight", "channel_mix.0.bias", "channel_mix.2.weight",
           "channel_mix.2.bias")


def load_fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def unpack(s, shape):
    """A fixture entry (base64 of little-endian float32) as an fp32 tensor of `shape`."""
    return torch.from_numpy(np.frombuffer(base64.b64decode(s), dtype="<f4").astype(np.float32)).reshape(shape)


def case_shapes(N, D, hid):
    return {"token_mix_ln.weight": (D,), "token_mix_ln.bias": (D,), "channel_mix_ln.weight": (D,), "channel_mix_ln.bias": (D,),
            "token_mix.0.weight": (hid, N), "token_mix.0.bias": (hid,), "token_mix.2.weight": (N, hid), "token_mix.2.bias": (N,),
            "channel_mix.0.weight": (hid, D), "channel_mix.0.bias": (hid,), "channel_mix.2.weight": (D, hid),
            "channel_mix.2.bias": (D,)}


def case_inputs(B, N, D, hid):
    """x, cotangent and the MixerBlock(N, D, hid, D) state of a fixture case (tools/make_golden_token_mix.py's formula)."""
    tag = f"tm_{B}_{N}_{D}_{hid}"
    x = formula.wave(tag + ".x", (B, N, D))
    cot = formula.wave(tag + ".cot", (B, N, D))
    return x, cot, {key: formula.param_value(tag + "." + key, shp) for key, shp in case_shapes(N, D, hid).items()}


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


# ---- the two kernels ---------------------------------------------------------------------------------------------------
def left_ref(w, x, transposed=False, bias=None):
    """fp64 op(W) X_b + bias[m] on x [B, K, D] -> [B, M, D] (the value in front of the epilogue's activation)."""
    w, x = w.double(), x.double()
    v = torch.einsum("km,bkd->bmd" if transposed else "mk,bkd->bmd", w, x)
    return v if bias is None else v + bias.double()[None, :, None]


def left_abs(w, x, transposed=False, bias=None):
    """Sum of |terms| of left_ref, bias included."""
    return left_ref(w.abs(), x.abs(), transposed, None if bias is None else bias.abs())


def wgrad_ref(g, x):
    """fp64 (dW [M, K] = sum_b G_b X_b^T, db [M] = sum_{b, d} G_b[m, d])."""
    g, x = g.double(), x.double()
    return torch.einsum("bmd,bkd->mk", g, x), g.sum(dim=(0, 2))


def wgrad_abs(g, x):
    return wgrad_ref(g.abs(), x.abs())


# ---- the block ---------------------------------------------------------------------------------------------------------
def token_mix_forward(x, p, eps=1e-5):
    """x + W2 gelu(W1 LN(x) + b1) + b2 along the token axis, in the dtype of x / p (autograd-able)."""
    D = x.shape[-1]
    z = TF.layer_norm(x, (D,), p["token_mix_ln.weight"], p["token_mix_ln.bias"], eps)
    u = torch.einsum("hn,bnd->bhd", p["token_mix.0.weight"], z) + p["token_mix.0.bias"][None, :, None]
    t = torch.einsum("nh,bhd->bnd", p["token_mix.2.weight"], gelu(u)) + p["token_mix.2.bias"][None, :, None]
    return x + t


def channel_mix_forward(x, p, eps=1e-5):
    D = x.shape[-1]
    z = TF.layer_norm(x, (D,), p["channel_mix_ln.weight"], p["channel_mix_ln.bias"], eps)
    return x + TF.linear(gelu(TF.linear(z, p["channel_mix.0.weight"], p["channel_mix.0.bias"])), p["channel_mix.2.weight"],
                         p["channel_mix.2.bias"])


def mixer_ref(x, sd, cot, token_mix=True, channel_mix=True, eps=1e-5):
    """fp64 MixerBlock with the token-mix branch on: (y, dx, {param: grad}) of sum(y * cot); parameters of a branch that is
    switched off get no entry."""
    x = x.double().clone().requires_grad_(True)
    p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    y = x
    if token_mix:
        y = token_mix_forward(y, p, eps)
    if channel_mix:
        y = channel_mix_forward(y, p, eps)
    (y * cot.double()).sum().backward()
    return y.detach(), x.grad, {k: t.grad for k, t in p.items() if t.grad is not None}
