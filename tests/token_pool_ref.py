"""fp64 statements of the CLS token and the pooled read-outs, shared by test_token_pool_cpu.py and test_token_pool_gpu.py:
the four operations as plain torch arithmetic on the CPU, and the whole model with either pool kind -- the oracle's blocks
evaluated in fp64 around one `cat` and one pooled LayerNorm + Linear.  Independent of the kernels."""
import json
import os

import torch

from oracle import formula, vit_oracle
from oracle.cases import MODEL_CASES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_pool.json")
_cache = {}


def load_fixture():
    if "fixture" not in _cache:
        with open(GOLDEN) as f:
            _cache["fixture"] = json.load(f)
    return _cache["fixture"]


def prepend_ref(x, cls):
    """fp64 cat([cls, x], dim=1)."""
    return torch.cat([cls.double().reshape(1, 1, -1).expand(x.shape[0], -1, -1), x.double()], dim=1)


def prepend_bwd_ref(dy):
    """fp64 (dx = dy[:, 1:], dcls = sum_b dy[b, 0], sum_b |dy[b, 0]|: the scale of dcls's rounding-error bound)."""
    d = dy.double()
    return d[:, 1:], d[:, 0].sum(dim=0), d[:, 0].abs().sum(dim=0)


def pool_ref(x, first, count):
    """fp64 (mean of tokens [first, first + count), sum_t |x| / count: the scale of the sum's rounding-error bound)."""
    s = x.double()[:, first:first + count]
    return s.sum(dim=1) / count, s.abs().sum(dim=1) / count


def pool_bwd_ref(dy, T, first, count):
    """fp64 dx [B, T, D]: dy / count on the range, 0 elsewhere."""
    dx = torch.zeros(dy.shape[0], T, dy.shape[1], dtype=torch.float64)
    dx[:, first:first + count] = (dy.double() / count).unsqueeze(1)
    return dx


def pooled_state(cfg, pool):
    """Formula-valued fp32 state of `cfg` with a pooled head: the parent's state without the factorised head's tensors, the
    pooled head's four (mlp_head.0 = LayerNorm, mlp_head.1 = Linear) and, for "cls", encoder.cls_token."""
    sd = {k: v for k, v in vit_oracle.formula_state(cfg).items() if not k.startswith("mlp_head.")}
    d, c = cfg.embed_dim, cfg.num_classes
    for k, shape in (("mlp_head.0.weight", (d,)), ("mlp_head.0.bias", (d,)), ("mlp_head.1.weight", (c, d)), ("mlp_head.1.bias", (c,))):
        sd[k] = formula.param_value(k, shape)
    if pool == "cls":
        sd["encoder.cls_token"] = formula.wave("encoder.cls_token", (1, 1, d), scale=load_fixture()["cls_scale"])
    return sd


def model_ref(name, pool):
    """fp64 forward and backward of fixture case `name` with pool kind `pool`: the CLS token joins after the mixer block (1-D
    model) and before the first encoder layer (vit.py:237-238); the head is LayerNorm + Linear on token 0 or on the token mean.
    -> dict(logits, loss, dcls [D] or None, grad_l2 {key: norm}).  Computed once and shared."""
    if ("model", name, pool) in _cache:
        return _cache[("model", name, pool)]
    cfg, batch = MODEL_CASES[name]
    sd = {k: (v.double().requires_grad_(True) if torch.is_floating_point(v) and not k.startswith("encoder.to_patch_embedding.") else v)
          for k, v in pooled_state(cfg, pool).items()}
    for k in list(sd):                                         # the tokenizer's second registration: the same tensors
        if k.startswith("encoder.to_patch_embedding."):
            sd[k] = sd["patch_embed." + k[len("encoder.to_patch_embedding."):]]
    x = formula.image_batch(batch, cfg.in_channels, cfg.img_size, cfg.img_size).double()
    tgt = formula.soft_targets(batch, cfg.num_classes).double()
    t = vit_oracle.tokenize(x, sd, cfg)
    if cfg.variant == "1d":
        t = vit_oracle.mixer_block(t, sd)
    if pool == "cls":
        t = torch.cat([sd["encoder.cls_token"].expand(t.shape[0], -1, -1), t], dim=1)
    for layer in range(cfg.depth):
        t = vit_oracle.encoder_layer(t, sd, f"encoder.transformer.layers.{layer}.", cfg.n_heads)
    v = t[:, 0] if pool == "cls" else t.mean(dim=1)
    z = vit_oracle.layer_norm(v, sd["mlp_head.0.weight"], sd["mlp_head.0.bias"])
    logits = z @ sd["mlp_head.1.weight"].t() + sd["mlp_head.1.bias"]
    loss = vit_oracle.soft_target_ce(logits, tgt)
    loss.backward()
    grads = {k: (None if v.grad is None else float(v.grad.norm())) for k, v in sd.items()
             if torch.is_floating_point(v) and not k.startswith("encoder.to_patch_embedding.")}
    out = {"logits": logits.detach(), "loss": float(loss.detach()), "grad_l2": grads, "cfg": cfg, "batch": batch,
           "dcls": sd["encoder.cls_token"].grad.flatten() if pool == "cls" else None}
    _cache[("model", name, pool)] = out
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
