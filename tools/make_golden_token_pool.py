#!/usr/bin/env python3
"""Generate tests/golden/token_pool.json by importing the reference's models (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_token_pool.py [path/to/reference]

What is committed is data only.  The reference ships TransformerSeqEncoder with its learnable [CLS] token commented out
(src/models/vit.py:209-210, :237-238: `torch.cat((cls_tokens, x), dim=1)` in front of `self.transformer`) and a docstring
that promises the encoded [CLS] token; altvit.py pools with `x.mean(dim=1)`.  This script evaluates both read-outs with
the reference's OWN modules, in fp32 on the CPU: the real VisionTransformer at MODEL_CASES["raster32_2d"] and the real
VisionTransformer1D at ["hilbert32_1d"] give `patch_embed`, `mlp_mixer` and `encoder.transformer` (an
nn.TransformerEncoder), which runs on cat([cls, x]) or on x; an nn.LayerNorm + nn.Linear reads token 0 or the token
mean.  Weights are formula values (oracle/formula.py's generator, so the fixture stores names, not values); the pooled
head's four tensors take the keys mlp_head.0.* / mlp_head.1.*, the token the key encoder.cls_token.  Stored per case and
pool kind: eval logits, the loss of formula.soft_targets, the L2 norm of every gradient and the token's gradient.
Without the reference this script does nothing."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

CASES = ("raster32_2d", "hilbert32_1d")
POOLS = ("cls", "mean")
CLS_SCALE = 0.5


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    if not os.path.isdir(ref):
        print("reference not present: fixture left as committed")
        return 0
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, ref)
    from src.models.vit import VisionTransformer, VisionTransformer1D
    from src.tokenizers._1D.hilbert_embedding1D import HilbertEmbedding1D
    from src.tokenizers._1D.zigzag_embedding1D import RasterScan1DEmbedding
    from oracle import formula
    from oracle.cases import MODEL_CASES

    torch.set_num_threads(8)
    out = {"cls_scale": CLS_SCALE, "cases": {}}
    for name in CASES:
        cfg, batch = MODEL_CASES[name]
        tok = {"hilbert1d": HilbertEmbedding1D, "raster1d": RasterScan1DEmbedding}[cfg.tokenizer]
        kind = VisionTransformer1D if cfg.variant == "1d" else VisionTransformer
        out["cases"][name] = {}
        for pool in POOLS:
            pe = tok(cfg.img_size, cfg.patch_size, cfg.in_channels, cfg.embed_dim)
            model = kind(pe, depth=cfg.depth, n_heads=cfg.n_heads, mlp_dim=cfg.mlp_dim, num_classes=cfg.num_classes)
            n, d = model.patch_embed.n_patches, model.patch_embed.embed_dim
            model.load_state_dict(formula.fill_state_dict(model.state_dict()))
            model.eval()                                        # dropout off: parity is eval-mode
            head = torch.nn.Sequential(torch.nn.LayerNorm(d), torch.nn.Linear(d, cfg.num_classes))
            head.load_state_dict({k: formula.param_value("mlp_head." + k, tuple(v.shape)) for k, v in head.state_dict().items()})
            head.eval()
            cls = formula.wave("encoder.cls_token", (1, 1, d), scale=CLS_SCALE).requires_grad_(True)
            x = formula.image_batch(batch, cfg.in_channels, cfg.img_size, cfg.img_size)
            tgt = formula.soft_targets(batch, cfg.num_classes)
            t = model.patch_embed(x)
            if cfg.variant == "1d":
                t = model.mlp_mixer(t)
            if pool == "cls":
                t = torch.cat((cls.expand(t.size(0), -1, -1), t), dim=1)         # vit.py:237-238
            t = model.encoder.transformer(t)                    # vit.py:241
            logits = head(t[:, 0] if pool == "cls" else t.mean(dim=1))
            loss = -(tgt * torch.log_softmax(logits, dim=-1)).sum(-1).mean()      # main.py:49-51
            loss.backward()
            grads = {k: (None if p.grad is None else float(p.grad.double().norm())) for k, p in model.named_parameters()
                     if not k.startswith("mlp_head.")}         # the factorised head is not part of a pooled model
            grads.update({"mlp_head." + k: float(p.grad.double().norm()) for k, p in head.named_parameters()})
            case = {"batch": batch, "N": n, "D": d, "logits": logits.detach().tolist(), "loss": float(loss.detach()), "grad_l2": grads}
            if pool == "cls":
                grads["encoder.cls_token"] = float(cls.grad.double().norm())
                case["dcls"] = cls.grad.flatten().tolist()
            out["cases"][name][pool] = case
            print(name, pool, "loss", case["loss"], "tokens", t.shape[1])
    os.makedirs(GOLD, exist_ok=True)
    with open(os.path.join(GOLD, "token_pool.json"), "w") as f:
        json.dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
