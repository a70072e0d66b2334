"""fp64 statements of the positional embedding, shared by test_pos_embed_cpu.py and test_pos_embed_gpu.py: the add and its
gradient as plain torch arithmetic on the CPU, the fixed tables from their formulas, and the whole model with the table
added after the tokenizer -- the oracle's blocks evaluated in fp64 around one `+`.  Independent of the kernels."""
import json
import math
import os

import torch

from oracle import formula, vit_oracle
from oracle.cases import MODEL_CASES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pos_embed.json")
_cache = {}


def load_fixture():
    if "fixture" not in _cache:
        with open(GOLDEN) as f:
            _cache["fixture"] = json.load(f)
    return _cache["fixture"]


def table_value(name, n, d):
    """The [1, N, D] table of a fixture case (tools/make_golden_pos_embed.py's formula)."""
    return formula.wave(f"pos_embed.{name}", (1, n, d), scale=load_fixture()["table_scale"])


def add_ref(x, pos):
    """fp64 x[b, n, :] + pos[n, :]."""
    return x.double() + pos.double().reshape(1, *x.shape[1:])


def dpos_ref(dy):
    """fp64 (sum_b dy[b], sum_b |dy[b]|): the table's gradient and the scale of its rounding-error bound."""
    return dy.double().sum(dim=0), dy.double().abs().sum(dim=0)


def sincos1d_ref(n, d, temperature=10000.0):
    """fp64: column 2i = sin(p w_i), column 2i + 1 = cos(p w_i), w_i = temperature^(-2i / d)."""
    out = torch.empty(n, d, dtype=torch.float64)
    for p in range(n):
        for i in range(d // 2):
            a = p * temperature ** (-2.0 * i / d)
            out[p, 2 * i], out[p, 2 * i + 1] = math.sin(a), math.cos(a)
    return out


def sincos2d_ref(positions, d, temperature=10000.0):
    """fp64 [sin(col w) | cos(col w) | sin(row w) | cos(row w)], w_k = temperature^(-k / (d / 4)), of [N, 2] (row, col)."""
    q = d // 4
    out = torch.empty(len(positions), d, dtype=torch.float64)
    for t, (row, col) in enumerate(positions.tolist()):
        for k in range(q):
            w = temperature ** (-k / q)
            out[t, k], out[t, q + k] = math.sin(col * w), math.cos(col * w)
            out[t, 2 * q + k], out[t, 3 * q + k] = math.sin(row * w), math.cos(row * w)
    return out


def model_ref(name):
    """fp64 forward and backward of fixture case `name` with the table added directly after the tokenizer (vit.py:382):
    -> dict(logits, loss, table_grad [1, N, D], grad_l2 {key: norm}).  Computed once and shared."""
    if ("model", name) in _cache:
        return _cache[("model", name)]
    cfg, batch = MODEL_CASES[name]
    sd = {k: (v.double().requires_grad_(True) if torch.is_floating_point(v) and not k.startswith("encoder.to_patch_embedding.") else v)
          for k, v in vit_oracle.formula_state(cfg).items()}
    for k in list(sd):                                         # the tokenizer's second registration: the same tensors
        if k.startswith("encoder.to_patch_embedding."):
            sd[k] = sd["patch_embed." + k[len("encoder.to_patch_embedding."):]]
    table = table_value(name, cfg.n_patches, cfg.embed_dim).double().requires_grad_(True)
    x = formula.image_batch(batch, cfg.in_channels, cfg.img_size, cfg.img_size).double()
    tgt = formula.soft_targets(batch, cfg.num_classes).double()
    t = vit_oracle.tokenize(x, sd, cfg) + table
    if cfg.variant == "1d":
        t = vit_oracle.mixer_block(t, sd)
    for layer in range(cfg.depth):
        t = vit_oracle.encoder_layer(t, sd, f"encoder.transformer.layers.{layer}.", cfg.n_heads)
    logits = vit_oracle.head(t, sd)
    loss = vit_oracle.soft_target_ce(logits, tgt)
    loss.backward()
    grads = {k: (None if v.grad is None else float(v.grad.norm())) for k, v in sd.items()
             if torch.is_floating_point(v) and not k.startswith("encoder.to_patch_embedding.")}
    out = {"logits": logits.detach(), "loss": float(loss.detach()), "table_grad": table.grad, "grad_l2": grads, "cfg": cfg, "batch": batch}
    _cache[("model", name)] = out
    return out


def build_with(cfg, **kw):
    """build_model(cfg) of test_host_cpu with extra model keywords: same tokenizer construction, same argument order."""
    import sfcvit.models as models
    from test_host_cpu import build_model
    orig = {n: getattr(models, n) for n in ("VisionTransformer", "VisionTransformer1D")}

    def patched(c):
        return lambda pe, **k2: c(pe, **k2, **kw)
    try:
        for n, c in orig.items():
            setattr(models, n, patched(c))
        return build_model(cfg)
    finally:
        for n, c in orig.items():
            setattr(models, n, c)
