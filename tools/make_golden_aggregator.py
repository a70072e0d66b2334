#!/usr/bin/env python3
"""Generate tests/golden/token_aggregator.json by importing the reference's TokenAggregator (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_aggregator.py [path/to/reference]

What is committed is data only.  For (B, N, D, k) = (2, 5, 16, 3) and (2, 12, 24, 5): formula-generated input, parameters
and cotangent (oracle/formula.py's generator, so the fixture stores names and shapes, not values), and what the
reference module computes from them in fp32 on the CPU -- output, input gradient and parameter gradients of
sum(y * cotangent).  Plus the key / shape manifest and seeded initial values of TokenAggregator(192), and the keys a
VisionTransformer / VisionTransformer1D state gains with `ta` present.  Without the reference this script does nothing."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

CASES = [(2, 5, 16, 3), (2, 12, 24, 5)]
INIT_SEED, INIT_DIM = 1234, 192


def case_inputs(B, N, D, k):
    """x, cotangent and the state_dict of TokenAggregator(D, k) by formula (tests rebuild them the same way)."""
    from oracle import formula
    tag = f"ta_{B}_{N}_{D}_{k}"
    x = formula.wave(tag + ".x", (B, N, D))
    cot = formula.wave(tag + ".cot", (B, N, D))
    shapes = {"dw.weight": (D, 1, k), "dw.bias": (D,), "pw.weight": (D, D, 1), "pw.bias": (D,), "norm.weight": (D,), "norm.bias": (D,)}
    sd = {key: formula.param_value(tag + "." + key, shp) for key, shp in shapes.items()}
    return x, cot, sd


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    if not os.path.isdir(ref):
        print("reference not present: fixture left as committed")
        return 0
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    from src.models.vit import TokenAggregator

    out = {"cases": [], "init": {}, "model_keys": {}}
    for B, N, D, k in CASES:
        x, cot, sd = case_inputs(B, N, D, k)
        mod = TokenAggregator(D, k)
        mod.load_state_dict(sd)
        x = x.clone().requires_grad_(True)
        y = mod(x)
        (y * cot).sum().backward()
        grads = {key: p.grad.flatten().tolist() for key, p in mod.named_parameters()}
        out["cases"].append({"B": B, "N": N, "D": D, "k": k, "y": y.detach().flatten().tolist(), "dx": x.grad.flatten().tolist(),
                             "grads": grads})
    torch.manual_seed(INIT_SEED)
    mod = TokenAggregator(INIT_DIM)
    out["init"] = {"seed": INIT_SEED, "dim": INIT_DIM,
                   "keys": {key: [list(v.shape), str(v.dtype).replace("torch.", "")] for key, v in mod.state_dict().items()},
                   # enough to pin the initialisation: first 8 values and the sum of every entry
                   "head": {key: v.flatten()[:8].tolist() for key, v in mod.state_dict().items()},
                   "sum": {key: float(v.double().sum()) for key, v in mod.state_dict().items()}}
    # a VisionTransformer(...) of the reference with its two commented lines switched on gains exactly these keys
    out["model_keys"] = {"prefix": "ta.", "dim": 64,
                         "keys": {"ta." + key: list(v.shape) for key, v in TokenAggregator(64).state_dict().items()}}
    os.makedirs(GOLD, exist_ok=True)
    with open(os.path.join(GOLD, "token_aggregator.json"), "w") as f:
        json.dump(out, f)
    print("cases:", [(c["B"], c["N"], c["D"], c["k"]) for c in out["cases"]], "keys:", sorted(out["init"]["keys"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
