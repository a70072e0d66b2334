#!/usr/bin/env python3
"""Generate tests/golden/mix.json and mix_batches.npz by importing the reference's MixUp / CutMix helpers (authoring container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_mix.py [path/to/reference]

What is committed is data only: for a handful of seeds the draws of the reference's loop (train.py:148-160:
np.random.rand() < 0.5 -> mixup_data(alpha=0.2), else cutmix_data(alpha=1.0)) on CPU tensors -- lam, idx, box, adjusted
lam -- the mixed [4, 3, 32, 32] batch of one MixUp and one CutMix draw (fp32 bit patterns), and the soft-target loss of
fixed logits.  Without the reference this script does nothing."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

SEEDS = list(range(12))
B, C, H, W, CLASSES = 4, 3, 32, 32, 10


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    if not os.path.isdir(ref):
        print("reference not present: fixture left as committed")
        return 0
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    from src.training import train as rt
    from oracle import formula

    x0 = formula.image_batch(B, C, H, W)
    labels = torch.tensor([3, 7, 7, 1])
    logits = ((torch.arange(B * CLASSES, dtype=torch.float32).reshape(B, CLASSES) * 0.37) % 5.0) - 2.0
    out = {"shape": [B, C, H, W], "labels": labels.tolist(), "logits": logits.tolist(), "draws": [], "mixed": {}}
    arrays = {}                                                     # kind -> fp32 bit patterns of the mixed batch (mix_batches.npz)
    for seed in SEEDS:
        np.random.seed(seed)
        torch.manual_seed(seed)
        x = x0.clone()
        mixup = np.random.rand() < 0.5                              # train.py:153-158
        kind, alpha = ("mixup", 0.2) if mixup else ("cutmix", 1.0)
        # what the helper is about to draw, replayed from the state it will see: beta, randperm, (rand_bbox's randints)
        st_np, st_t = np.random.get_state(), torch.get_rng_state()
        lam0 = float(np.random.beta(alpha, alpha))
        idx = torch.randperm(B)
        box = None if mixup else [int(v) for v in rt.rand_bbox(H, W, lam0)]
        np.random.set_state(st_np)
        torch.set_rng_state(st_t)
        mixed, y_a, y_b, lam = (rt.mixup_data if mixup else rt.cutmix_data)(x, labels, alpha=alpha)
        assert torch.equal(y_b, labels[idx]) and torch.equal(y_a, labels)
        if mixup:
            assert lam == lam0 and torch.equal(mixed, lam * x0 + (1 - lam) * x0[idx])
        else:
            assert torch.equal(mixed[:, :, box[0]:box[2], box[1]:box[3]], x0[idx][:, :, box[0]:box[2], box[1]:box[3]])
        idx = idx.tolist()
        soft = lam * torch.nn.functional.one_hot(y_a, CLASSES).float() + (1 - lam) * torch.nn.functional.one_hot(y_b, CLASSES).float()
        loss = float(torch.sum(-soft * torch.nn.functional.log_softmax(logits, dim=-1), dim=-1).mean())
        out["draws"].append({"seed": seed, "kind": kind, "lam_drawn": lam0, "lam": float(lam), "idx": idx, "box": box,
                             "y_b": y_b.tolist(), "loss": loss})
        if kind not in out["mixed"] and 0.05 < lam < 0.95:          # a draw that really mixes (beta(0.2, 0.2) favours 0 and 1)
            out["mixed"][kind] = seed
            arrays[kind] = mixed.contiguous().view(torch.int32).numpy().copy()
    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, "mix_batches.npz"), **arrays)
    with open(os.path.join(GOLD, "mix.json"), "w") as f:
        json.dump(out, f)
    print("draws:", [(d["seed"], d["kind"], round(d["lam"], 4), d["idx"], d["box"]) for d in out["draws"]])
    return 0


if __name__ == "__main__":
    sys.exit(main())
