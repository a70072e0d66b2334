#!/usr/bin/env python3
"""Generate tests/golden/pos_embed.json by importing the reference's models (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_pos_embed.py [path/to/reference]

What is committed is data only.  The reference ships VisionTransformer.forward with its positional embedding commented
out (src/models/vit.py:360-361, :382: a [1, N, D] parameter added to the tokenizer's output, sliced to the token count,
before the encoder); this script evaluates that addition at its place
by a forward hook on the reference model's OWN `patch_embed` that adds a [1, N, D] table to the tokenizer's output, in
fp32 on the CPU, for the real VisionTransformer at MODEL_CASES["raster32_2d"] and the real VisionTransformer1D at
["hilbert32_1d"] with formula weights (oracle/formula.py's generator, so the fixture stores names and shapes, not values)
and a formula table.  Stored: eval logits, the loss of formula.soft_targets, the gradient of the table and the L2 norm of
every other gradient.  Plus, to pin the constructed-last rule, the first 8 values and the sum of torch.randn(1, N, D)
drawn at a fixed seed directly after the reference model's construction, and the reference's posemb_sincos_1d(5, 16)
(src/models/altvit.py).  Without the reference this script does nothing."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

CASES = ("raster32_2d", "hilbert32_1d")
INIT_SEED = 1234
TABLE_SCALE = 0.5


def table_value(name, n, d):
    """The [1, N, D] table of a fixture case by formula (tests rebuild it the same way)."""
    from oracle import formula
    return formula.wave(f"pos_embed.{name}", (1, n, d), scale=TABLE_SCALE)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    if not os.path.isdir(ref):
        print("reference not present: fixture left as committed")
        return 0
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, ref)
    from src.models.altvit import posemb_sincos_1d
    from src.models.vit import VisionTransformer, VisionTransformer1D
    from src.tokenizers._1D.hilbert_embedding1D import HilbertEmbedding1D
    from src.tokenizers._1D.zigzag_embedding1D import RasterScan1DEmbedding
    from oracle import formula
    from oracle.cases import MODEL_CASES

    torch.set_num_threads(8)
    out = {"table_scale": TABLE_SCALE, "cases": {}, "init": {}}
    for name in CASES:
        cfg, batch = MODEL_CASES[name]
        tok = {"hilbert1d": HilbertEmbedding1D, "raster1d": RasterScan1DEmbedding}[cfg.tokenizer]
        cls = VisionTransformer1D if cfg.variant == "1d" else VisionTransformer

        def build():
            pe = tok(cfg.img_size, cfg.patch_size, cfg.in_channels, cfg.embed_dim)
            return cls(pe, depth=cfg.depth, n_heads=cfg.n_heads, mlp_dim=cfg.mlp_dim, num_classes=cfg.num_classes)

        model = build()
        n, d = model.patch_embed.n_patches, model.patch_embed.embed_dim
        model.load_state_dict(formula.fill_state_dict(model.state_dict()))
        model.eval()                                            # dropout off: parity is eval-mode
        table = table_value(name, n, d).requires_grad_(True)
        model.patch_embed.register_forward_hook(lambda _m, _i, y: y + table[:, :y.size(1), :])      # vit.py:382
        x = formula.image_batch(batch, cfg.in_channels, cfg.img_size, cfg.img_size)
        tgt = formula.soft_targets(batch, cfg.num_classes)
        logits = model(x)
        loss = -(tgt * torch.log_softmax(logits, dim=-1)).sum(-1).mean()      # main.py:49-51
        loss.backward()
        grads = {k: (None if p.grad is None else float(p.grad.double().norm())) for k, p in model.named_parameters()}
        torch.manual_seed(INIT_SEED)
        build()
        drawn = torch.randn(1, n, d)                           # what a parameter constructed LAST draws
        out["cases"][name] = {"batch": batch, "N": n, "D": d, "logits": logits.detach().tolist(), "loss": float(loss.detach()),
                              "table_grad": table.grad.flatten().tolist(), "grad_l2": grads}
        out["init"][name] = {"seed": INIT_SEED, "head": drawn.flatten()[:8].tolist(), "sum": float(drawn.double().sum())}
        print(name, "loss", out["cases"][name]["loss"], "|dtable|", float(table.grad.norm()))
    out["sincos1d_5_16"] = posemb_sincos_1d(5, 16).flatten().tolist()
    os.makedirs(GOLD, exist_ok=True)
    with open(os.path.join(GOLD, "pos_embed.json"), "w") as f:
        json.dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
