#!/usr/bin/env python3
"""Generate tests/golden/token_mix.json by importing the reference's MixerBlock (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_token_mix.py [path/to/reference]

What is committed is data only.  The reference ships MixerBlock.forward with its token-mix branch commented out
(src/models/vit.py:269-271); this script evaluates the two lines as written there,

    x = x + token_mix(token_mix_ln(x).transpose(1, 2)).transpose(1, 2)
    x = x + channel_mix(channel_mix_ln(x))

with the reference module's OWN submodules, in fp32 on the CPU.  For (B, N, D, hid) = (2, 5, 16, 32) and (2, 12, 24, 48):
formula-generated input, parameters and cotangent (oracle/formula.py's generator, so the fixture stores names and shapes,
not values), and the output, input gradient and every parameter gradient of sum(y * cotangent).  Plus the keys of
tests/golden/state_manifest.json that gain a gradient with the branch on.  Without the reference this script does nothing."""
import base64
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

CASES = [(2, 5, 16, 32), (2, 12, 24, 48)]
PREFIXES = ("mlp_mixer.token_mix.", "mlp_mixer.token_mix_ln.")


def pack(t):
    """fp32 tensor -> base64 of its little-endian bytes (exact, a quarter of the decimal spelling; tests/token_mix_ref.py
    unpacks it)."""
    return base64.b64encode(t.detach().contiguous().numpy().astype("<f4").tobytes()).decode("ascii")


def case_inputs(B, N, D, hid):
    """x, cotangent and the state_dict of MixerBlock(N, D, hid, D) by formula (tests rebuild them the same way)."""
    from oracle import formula
    tag = f"tm_{B}_{N}_{D}_{hid}"
    x = formula.wave(tag + ".x", (B, N, D))
    cot = formula.wave(tag + ".cot", (B, N, D))
    shapes = {"token_mix_ln.weight": (D,), "token_mix_ln.bias": (D,), "channel_mix_ln.weight": (D,), "channel_mix_ln.bias": (D,),
              "token_mix.0.weight": (hid, N), "token_mix.0.bias": (hid,), "token_mix.2.weight": (N, hid), "token_mix.2.bias": (N,),
              "channel_mix.0.weight": (hid, D), "channel_mix.0.bias": (hid,), "channel_mix.2.weight": (D, hid),
              "channel_mix.2.bias": (D,)}
    sd = {key: formula.param_value(tag + "." + key, shp) for key, shp in shapes.items()}
    return x, cot, sd


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    if not os.path.isdir(ref):
        print("reference not present: fixture left as committed")
        return 0
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    from src.models.vit import MixerBlock

    out = {"encoding": "base64 of little-endian float32, flattened", "cases": [], "gains_grad": {}}
    for B, N, D, hid in CASES:
        x, cot, sd = case_inputs(B, N, D, hid)
        mod = MixerBlock(N, D, hid, D)
        assert set(mod.state_dict()) == set(sd)
        mod.load_state_dict(sd)
        x = x.clone().requires_grad_(True)
        t = x + mod.token_mix(mod.token_mix_ln(x).transpose(1, 2)).transpose(1, 2)      # vit.py:269-271
        y_tm = t.detach().clone()
        y = t + mod.channel_mix(mod.channel_mix_ln(t))                                  # vit.py:272
        (y * cot).sum().backward()
        grads = {key: pack(p.grad) for key, p in mod.named_parameters()}
        out["cases"].append({"B": B, "N": N, "D": D, "hid": hid, "y": pack(y), "y_token_mix": pack(y_tm), "dx": pack(x.grad),
                             "grads": grads})
    with open(os.path.join(GOLD, "state_manifest.json")) as f:
        manifest = json.load(f)
    out["gains_grad"] = {name: sorted(k for k in keys if k.startswith(PREFIXES)) for name, keys in manifest.items()}
    with open(os.path.join(GOLD, "token_mix.json"), "w") as f:
        json.dump(out, f)
    print("cases:", [(c["B"], c["N"], c["D"], c["hid"]) for c in out["cases"]], "grad keys:", sorted(out["cases"][0]["grads"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
