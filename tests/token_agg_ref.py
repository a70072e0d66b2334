"""fp64 statements of the depth-wise sequence convolution and of TokenAggregator, shared by test_token_agg_cpu.py and
test_token_agg_gpu.py.  Written with torch's own conv1d / linear / gelu / layer_norm on the CPU: independent of the
kernels and of the fixture's generator."""
import json
import os

import torch
import torch.nn.functional as TF

from oracle import formula

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_aggregator.json")


def load_fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def case_inputs(B, N, D, k):
    """x, cotangent and the TokenAggregator(D, k) state of a fixture case (tools/make_golden_aggregator.py's formula)."""
    tag = f"ta_{B}_{N}_{D}_{k}"
    x = formula.wave(tag + ".x", (B, N, D))
    cot = formula.wave(tag + ".cot", (B, N, D))
    shapes = {"dw.weight": (D, 1, k), "dw.bias": (D,), "pw.weight": (D, D, 1), "pw.bias": (D,), "norm.weight": (D,), "norm.bias": (D,)}
    return x, cot, {key: formula.param_value(tag + "." + key, shp) for key, shp in shapes.items()}


def dwconv_ref(x, w, bias, s):
    """fp64 nn.Conv1d(D, D, k, s, padding=k // 2, groups=D) on [B, N, D]; w [D, k] -> [B, Nout, D]."""
    D, k = w.shape
    y = TF.conv1d(x.double().transpose(1, 2), w.double().view(D, 1, k), None if bias is None else bias.double(), stride=s,
                  padding=k // 2, groups=D)
    return y.transpose(1, 2).contiguous()


def dwconv_grads_ref(x, w, bias, du, s):
    """fp64 (u, dx, dw, db) of sum(u * du) by autograd through dwconv_ref."""
    x = x.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    b = bias.double().clone().requires_grad_(True)
    u = dwconv_ref(x, w, b, s)
    (u * du.double()).sum().backward()
    return u.detach(), x.grad, w.grad, b.grad


def dwconv_abs_ref(x, w, bias, du, s):
    """The sums of absolute values of the terms of u, dx, dw, db (the error bounds' scale): the same convolutions on |.|."""
    return dwconv_grads_ref(x.abs(), w.abs(), bias.abs(), du.abs(), s)


def aggregator_ref(x, sd, cot, s=1, eps=1e-5):
    """fp64 TokenAggregator: (y, dx, {param: grad}) of sum(y * cot)."""
    x = x.double().clone().requires_grad_(True)
    p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    D, _, k = p["dw.weight"].shape
    u = TF.conv1d(x.transpose(1, 2), p["dw.weight"], p["dw.bias"], stride=s, padding=k // 2, groups=D).transpose(1, 2)
    v = TF.linear(u, p["pw.weight"].view(D, D), p["pw.bias"])
    y = TF.layer_norm(TF.gelu(v), (D,), p["norm.weight"], p["norm.bias"], eps)
    (y * cot.double()).sum().backward()
    return y.detach(), x.grad, {k: t.grad for k, t in p.items()}
