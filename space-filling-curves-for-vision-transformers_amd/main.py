#!/usr/bin/env python3
"""Entry script with the structure of the reference's main.py (seeds, tokenizer menu, model, AdamW +
warm-up cosine schedule, MixUp/CutMix epochs, evaluate, checkpoint on best accuracy) running on the
MI355X kernels.  The reference hard-codes everything and needs torchvision + a CIFAR-10 download; here
the same defaults are arguments and `--synthetic` (default when torchvision is missing) feeds random
CIFAR-shaped batches so that the script runs on an air-gapped GPU box.

    python main.py --epochs 2 --synthetic                       # reference default model on 32x32
    python main.py --tokenizer hilbert --img-size 224 --patch-size 256 --embed-dim 768 --depth 12 \\
                   --heads 12 --mlp-dim 3072 --classes 1000 --batch-size 256 --synthetic
    torchrun --nproc-per-node 8 main.py ...                     # data parallel (one process per GPU)
"""
import argparse
import os
import sys

# dmabuf IPC is the only kind this pool's host driver supports: without it RCCL (and any cross-process sharing of
# device memory) fails with "hipIpcGetMemHandle: invalid argument".  Must be in the environment before HIP initialises.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sfcvit.models.vit import VisionTransformer1D                                  # noqa: E402
import sfcvit.tokenizers as T                                                       # noqa: E402
from sfcvit.training import BatchMix, DeviceAugment, FusedAdamW, GradReducer, GraphedTrainStep, SoftTargetCrossEntropy, WarmupCosine   # noqa: E402
from sfcvit.training.loops import evaluate, train_with_mixup_or_cutmix             # noqa: E402


class SyntheticLoader:
    """CIFAR-shaped random batches, regenerated deterministically every epoch.  uint8=True (--device-augment): raw
    [0, 255] images, as a dataset holds them before any transform."""

    def __init__(self, n, batch, img, classes, seed, device, uint8=False):
        self.n, self.batch, self.img, self.classes, self.seed, self.device = n, batch, img, classes, seed, device
        self.uint8 = uint8
        self.dataset = range(n)

    def __len__(self):
        return self.n // self.batch

    def __iter__(self):
        g = torch.Generator(device=self.device).manual_seed(self.seed)
        for _ in range(len(self)):
            if self.uint8:
                yield (torch.randint(0, 256, (self.batch, 3, self.img, self.img), device=self.device, generator=g, dtype=torch.uint8),
                       torch.randint(0, self.classes, (self.batch,), device=self.device, generator=g))
                continue
            yield (torch.randn(self.batch, 3, self.img, self.img, device=self.device, generator=g),
                   torch.randint(0, self.classes, (self.batch,), device=self.device, generator=g))


def build_tokenizer(a):
    one_d = {"raster": T.RasterScan1DEmbedding, "hilbert": T.HilbertEmbedding1D, "peano": T.PeanoEmbedding1D,
             "moore": T.MooreEmbedding1D, "onion": T.OnionEmbedding1D, "morton": T.MortonEmbedding1D,
             "zigzag": T.ZigzagEmbedding, "hilbert2d": T.HilbertEmbedding}           # main.py:232-240 (+ _2D/hilbert)
    hier = {"hier_raster": T.HierarchicalRasterScanEmbedding, "hier_hilbert": T.HierarchicalHilbertEmbedding,
            "hier_peano": T.HierarchicalPeanoEmbedding, "hier_moore": T.HierarchicalMooreEmbedding,
            "hier_onion": T.HierarchicalOnionEmbedding, "hier_morton": T.HierarchicalMortonEmbedding}   # main.py:242-250
    if a.tokenizer in one_d:
        return one_d[a.tokenizer](a.img_size, a.patch_size, 3, a.embed_dim)
    if a.tokenizer not in hier:
        raise SystemExit(f"--tokenizer must be one of {sorted(one_d) + sorted(hier)}")
    return hier[a.tokenizer](a.img_size, 3, a.levels, a.embed_dim)          # main.py:269-274: ([16, 4, 1], 256)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokenizer", default="hier_morton")       # the reference's active menu entry (main.py:232-240)
    ap.add_argument("--img-size", type=int, default=32)
    ap.add_argument("--patch-size", type=int, default=256)
    ap.add_argument("--levels", type=int, nargs="+", default=[16, 4, 1])
    ap.add_argument("--embed-dim", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)             # main.py:276-282
    ap.add_argument("--heads", type=int, default=4)             # head dim 768 / 4 = 192, any image size (attention_wide.hip up to N = 192, attention_wide_stream.hip beyond)
    ap.add_argument("--mlp-dim", type=int, default=512)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=512)      # main.py:228
    ap.add_argument("--epochs", type=int, default=300)          # main.py:306
    ap.add_argument("--warmup-epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--weight-decay", type=float, default=5e-5)
    ap.add_argument("--train-size", type=int, default=50000)
    ap.add_argument("--test-size", type=int, default=10000)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--data-module", default=None,
                    help="pkg.module:function returning (train_loader, test_loader) -- the caller's own DataLoaders in place "
                         "of the reference's inline CIFAR-10 pipeline (main.py:169-230)")
    ap.add_argument("--checkpoint-dir", default="./vit_checkpoints")
    ap.add_argument("--resume", default=None)
    ap.add_argument("--resume-model-only", action="store_true",
                    help="take only the weights from --resume (e.g. a checkpoint the REFERENCE's main.py wrote: its "
                         "optimizer / scheduler states are torch.optim formats, see INTEGRATION.md)")
    ap.add_argument("--graph", action="store_true",
                    help="replay every training step from one hipGraph (the reference's torch.compile(model, "
                         "mode='reduce-overhead'), main.py:284, for the whole step); single process")
    ap.add_argument("--device-mix", action="store_true",
                    help="MixUp / CutMix on the device: the batch is mixed inside the tokenizer's gather and the loss taken "
                         "from the label pair (same seeded draws); with --graph the augmentation is part of the replayed step")
    ap.add_argument("--device-augment", action="store_true",
                    help="the reference's transform stack (RandomResizedCrop, flip, ColorJitter, RandomErasing, Normalize; "
                         "main.py:169-188) on the device: the loaders then yield raw uint8 batches [B, 3, H, W]; works with "
                         "--device-mix and --graph")
    ap.add_argument("--attention-report", default=None, metavar="FILE",
                    help="after building (or resuming) the model, measure one test batch with sfcvit.analysis.attention_report "
                         "and write per-layer, per-head batch means of attention distance (image and curve) and entropy as JSON")
    ap.add_argument("--token-aggregator", type=int, nargs="?", const=3, default=None, metavar="K",
                    help="apply the reference's TokenAggregator (src/models/vit.py:20-42: depth-wise conv of K taps along the "
                         "curve, point-wise conv, GELU, LayerNorm) directly after the tokenizer; K odd, default 3.  Checkpoints "
                         "then carry the ta.* keys")
    ap.add_argument("--token-mix", action="store_true",
                    help="switch the MixerBlock's token-mix branch on (src/models/vit.py:269-271, commented out in the "
                         "reference): a learned mixing along the curve in front of the channel mix.  Checkpoints keep their keys")
    ap.add_argument("--pos-embed", choices=["learned", "sincos1d", "sincos2d"], default=None,
                    help="add a positional embedding directly after the tokenizer (src/models/vit.py:360-361, :382, commented "
                         "out in the reference): a learned table (checkpoints then carry pos_embed [1, N, D]), a fixed sin-cos "
                         "encoding of the token index along the curve, or a fixed sin-cos encoding of the token's centre in the "
                         "image (the same whatever curve orders the tokens)")
    ap.add_argument("--pos-embed-std", type=float, default=1.0,
                    help="standard deviation of the learned table's initial values (the reference's randn: 1.0)")
    ap.add_argument("--pool", choices=["cls", "mean"], default=None,
                    help="a pooled classifier head, LayerNorm + Linear on one vector per image, in place of the factorised head "
                         "over all tokens: 'cls' puts a learnable [CLS] token in front of the encoder's sequence "
                         "(src/models/vit.py:209-210, :237-238, commented out in the reference; checkpoints then carry "
                         "encoder.cls_token) and reads it out, 'mean' reads the mean of the tokens.  The head then holds no weight "
                         "per token index")
    ap.add_argument("--drop-path", type=float, default=0.0, metavar="R",
                    help="stochastic depth (DropPath, the DeiT recipe's drop_path_rate): in training every encoder layer drops "
                         "each of its two residual branches per image, with a probability that grows linearly with depth from 0 "
                         "to R, and scales the kept ones up; 0 <= R < 1, default 0 (off).  Works with --graph; no checkpoint key")
    ap.add_argument("--pre-norm", action="store_true",
                    help="pre-norm encoder layers, x + f(LN(x)), with a final LayerNorm after the last one (torch's "
                         "norm_first=True under nn.TransformerEncoder(norm=): the DeiT / timm block); checkpoints then carry "
                         "encoder.transformer.norm.*.  Works with --graph, --accum-steps, --model-ema, --drop-path, --device-mix, "
                         "--device-augment and the model options")
    ap.add_argument("--activation", choices=["relu", "gelu"], default="relu",
                    help="the encoder MLP's activation; gelu (erf) needs --pre-norm")
    ap.add_argument("--layer-scale", type=float, nargs="?", const=1e-4, default=None, metavar="INIT",
                    help="LayerScale (CaiT / DeiT-III): a learned per-channel scale on each residual branch of every encoder "
                         "layer, initialised to INIT (1e-4 when the value is omitted); needs --pre-norm; checkpoints then carry "
                         "encoder.layer_scale.<l> [2, embed dim]")
    ap.add_argument("--qk-norm", type=float, nargs="?", const=1e-6, default=None, metavar="EPS",
                    help="QK-norm (ViT-22B; timm's qk_norm): a LayerNorm over the head dim on the queries and keys of every head "
                         "before q k^T, with epsilon EPS (1e-6 when the value is omitted): keeps the attention logits of deep and "
                         "wide models bounded in bf16; checkpoints then carry encoder.qk_norm.<l> [4, head dim] (q weight, q "
                         "bias, k weight, k bias).  Works with post- and pre-norm layers, --rel-pos-bias, --attn-window*, "
                         "--drop-path, --layer-scale, --graph, --accum-steps, --model-ema, --pool, --pos-embed and "
                         "--attention-report")
    ap.add_argument("--rope", choices=("curve", "image"), default=None,
                    help="rotary position embedding (RoPE-ViT, EVA-02, timm's rope blocks) on the queries and keys of every "
                         "encoder layer, after QK-norm: channel pairs are rotated by an angle that grows with the token's index "
                         "along the curve ('curve') or, half of the pairs each, with the column and the row of its centre in the "
                         "image ('image': the same whatever curve orders the tokens), so q . k depends on the offset only.  A "
                         "fixed table, no parameter and no checkpoint key; the kind and base are stored in the checkpoint and "
                         "--resume rebuilds the same table.  Works with post- and pre-norm layers, --qk-norm, --layer-scale, "
                         "--rel-pos-bias, --attn-window*, --pos-embed, --pool, --drop-path, --graph, --accum-steps, --model-ema "
                         "and --attention-report")
    ap.add_argument("--rope-base", type=float, default=None, metavar="X",
                    help="the base of the --rope frequencies (default: 10000 for 'curve', 100 for 'image')")
    ap.add_argument("--model-ema", type=float, nargs="?", const=0.9999, default=None, metavar="DECAY",
                    help="keep an exponential moving average of the weights (timm's --model-ema; DECAY defaults to 0.9999): "
                         "averaged in fp32 inside the AdamW kernel, evaluated after every epoch next to the raw weights (one "
                         "extra 'EMA Test Loss / EMA Test Acc' line) and checkpointed as model_ema_state_dict / ema_test_acc; "
                         "--resume continues the average.  Works with --graph, --device-mix and --device-augment")
    ap.add_argument("--accum-steps", type=int, default=1, metavar="K",
                    help="gradient accumulation: K consecutive batches of --batch-size form one optimizer step (effective batch "
                         "K x --batch-size; fp32 running sum, the average formed inside the clip pass); the scheduler, the EMA "
                         "and the clip advance once per optimizer step.  Works with --device-mix, --device-augment and data "
                         "parallelism (one exchange per optimizer step); not with --graph")
    ap.add_argument("--model-ema-warmup", action="store_true",
                    help="with --model-ema: the decay of step t is min(DECAY, (1 + t) / (10 + t)), so that the average follows "
                         "the weights closely in the first steps")
    win = ap.add_mutually_exclusive_group()
    win.add_argument("--attn-window", type=int, default=None, metavar="W",
                     help="local attention along the curve: every token attends to the tokens within W positions of it in "
                          "sequence order (sfcvit.masks.curve_window); runs on the masked attention kernels, also with --graph")
    win.add_argument("--attn-window-2d", type=float, default=None, metavar="R",
                     help="local attention in the image: every token attends to the tokens whose centres lie within R pixels "
                          "of its own in both axes (sfcvit.masks.image_window on the tokenizer's positions)")
    ap.add_argument("--rel-pos-bias", choices=["curve", "image"], default=None,
                    help="a learned relative position bias per head and encoder layer on the attention scores (Swin / BEiT), the "
                         "offset taken along the curve (j - i) or in the image (the displacement of the token centres, whatever "
                         "the curve); checkpoints then carry encoder.rel_pos_bias.<l> [heads, buckets].  --attn-window W (with "
                         "curve) or --attn-window-2d R (with image) given with it becomes the window of the bias index instead "
                         "of a mask.  Works with --graph, --accum-steps, --model-ema, --drop-path, --pool and --pos-embed")
    ap.add_argument("--rel-pos-init-std", type=float, default=0.0,
                    help="standard deviation of the bias tables' initial values (default 0: the model starts out computing "
                         "what it computes without the bias)")
    ap.add_argument("--mean", type=float, nargs=3, default=[0.4914, 0.4822, 0.4465])      # main.py:176-177 (CIFAR)
    ap.add_argument("--std", type=float, nargs=3, default=[0.2023, 0.1994, 0.2010])
    return ap


def rel_pos_window(a):
    """The window of --rel-pos-bias's index, taken from the window option of its own kind (None: every pair visible);
    SystemExit for the other kind's option."""
    if a.rel_pos_bias == "curve" and a.attn_window_2d is not None:
        raise SystemExit("--rel-pos-bias curve counts offsets along the curve: its window is --attn-window W (tokens), not "
                         "--attn-window-2d")
    if a.rel_pos_bias == "image" and a.attn_window is not None:
        raise SystemExit("--rel-pos-bias image counts offsets in the image: its window is --attn-window-2d R (pixels), not "
                         "--attn-window")
    return a.attn_window if a.rel_pos_bias == "curve" else a.attn_window_2d


def build_model(a, patch_embed, attn_mask=None):
    """The model of the parsed arguments `a` (fp32, on the CPU: main() moves and casts it)."""
    rel = {}
    if getattr(a, "rel_pos_bias", None) is not None:      # else: the call as it is without the option
        rel = dict(rel_pos_bias=a.rel_pos_bias, rel_pos_window=rel_pos_window(a), rel_pos_init_std=a.rel_pos_init_std)
    if getattr(a, "pre_norm", False) or getattr(a, "activation", "relu") != "relu" or getattr(a, "layer_scale", None) is not None:
        rel.update(norm_first=a.pre_norm, activation=a.activation, layer_scale=a.layer_scale)
    if getattr(a, "qk_norm", None) is not None:
        rel.update(qk_norm=True, qk_norm_eps=a.qk_norm)
    if getattr(a, "rope", None) is not None:
        rel.update(rope=a.rope, rope_base=getattr(a, "rope_base", None))
    return VisionTransformer1D(patch_embed=patch_embed, depth=a.depth, n_heads=a.heads, mlp_dim=a.mlp_dim,
                               num_classes=a.classes,
                               token_aggregator=a.token_aggregator or False, token_mix=a.token_mix,
                               attn_mask=attn_mask, pos_embed=a.pos_embed,
                               pos_embed_std=a.pos_embed_std, pool=a.pool, drop_path_rate=a.drop_path, **rel)


def parse_args(argv=None):
    """The parsed arguments, with the combinations refused that no later code could honour."""
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.accum_steps < 1:
        ap.error(f"--accum-steps {a.accum_steps}: a positive number of batches per optimizer step expected")
    if a.activation != "relu" and not a.pre_norm:
        ap.error(f"--activation {a.activation} needs --pre-norm: the post-norm layer has the ReLU MLP only")
    if a.layer_scale is not None and not a.pre_norm:
        ap.error("--layer-scale needs --pre-norm: the post-norm layer has no LayerScale")
    if a.qk_norm is not None and not (a.qk_norm >= 0.0 and a.qk_norm < float("inf")):
        ap.error(f"--qk-norm {a.qk_norm}: a finite epsilon >= 0 expected")
    if a.rope_base is not None and a.rope is None:
        ap.error("--rope-base needs --rope curve or --rope image")
    if a.rope_base is not None and not (a.rope_base > 0.0 and a.rope_base < float("inf")):
        ap.error(f"--rope-base {a.rope_base}: a finite base > 0 expected")
    if a.graph and a.accum_steps > 1:
        ap.error("--graph cannot be combined with --accum-steps > 1: a captured step does not accumulate (graphs serve "
                 "launch-bound small models, accumulation serves models too large for the batch)")
    return a


def main():
    a = parse_args()

    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        from sfcvit.training.distributed import dist_timeout
        dist.init_process_group("nccl", device_id=device, timeout=dist_timeout())      # bounded collectives (SFCVIT_DIST_TIMEOUT)
    seed = 42                                                   # main.py:151-154
    torch.manual_seed(seed)
    np.random.seed(seed + rank)

    try:
        import torchvision  # noqa: F401
        have_tv = True
    except ImportError:
        have_tv = False
    per_rank = a.batch_size // world
    if a.data_module:
        # The reference builds its loaders inline (main.py:169-230: torchvision CIFAR-10 + v2 transforms, DataLoader with
        # 16 workers).  That pipeline is the caller's; this is the hook for it: `pkg.mod:fn` names a factory
        #     fn(batch_size=, img_size=, classes=, rank=, world=, seed=) -> (train_loader, test_loader)
        # returning iterables of (images [B, 3, H, W] float -- raw uint8 under --device-augment --, labels [B] int64) with __len__, on any device (the loops move
        # every batch to the GPU, src/training/train.py:144-145), each rank's own shard, every batch of `batch_size` rows.
        import importlib
        mod, _, fn = a.data_module.partition(":")
        if not mod or not fn:
            raise SystemExit("--data-module takes pkg.module:function")
        factory = getattr(importlib.import_module(mod), fn)
        train_loader, test_loader = factory(batch_size=per_rank, img_size=a.img_size, classes=a.classes, rank=rank,
                                            world=world, seed=seed)
    else:
        if not a.synthetic:
            print("no --data-module given (the reference's torchvision CIFAR-10 pipeline, main.py:169-230, is not part of "
                  "this package" + ("" if have_tv else " and torchvision is not installed") + "): using --synthetic data")
            a.synthetic = True
        train_loader = SyntheticLoader(a.train_size // world, per_rank, a.img_size, a.classes, seed + 1 + rank, device,
                                       uint8=a.device_augment)
        test_loader = SyntheticLoader(a.test_size // world, per_rank, a.img_size, a.classes, seed + 1001 + rank, device,
                                      uint8=a.device_augment)
    augment = test_transform = None
    if a.device_augment:
        augment = DeviceAugment(per_rank, a.img_size, a.img_size, mean=a.mean, std=a.std, seed=seed, device=device)
        augment.sample_base = rank * per_rank          # one draw stream per sample index, whatever the rank layout
        test_transform = DeviceAugment.test_transform(per_rank, a.img_size, a.img_size, mean=a.mean, std=a.std, device=device)

    patch_embed = build_tokenizer(a)
    attn_mask = None
    if a.rel_pos_bias is not None:
        rel_pos_window(a)                                       # a window of the other kind: refused before anything is built
    elif a.attn_window is not None or a.attn_window_2d is not None:
        from sfcvit import masks
        from sfcvit.ops import AttentionMask
        if a.attn_window is not None:
            window = masks.curve_window(patch_embed.n_patches, a.attn_window)
        else:
            from sfcvit.analysis import token_positions
            window = masks.image_window(token_positions(patch_embed), a.attn_window_2d)
        # --pool cls: the CLS token sees and is seen by every token; the window holds between the patch tokens
        attn_mask = AttentionMask(masks.with_cls_token(window) if a.pool == "cls" else window)
        if rank == 0:
            print(f"attention mask: {attn_mask.visited_blocks}/{attn_mask.total_blocks} blocks of 64 x 64 visited "
                  f"(N = {attn_mask.n_tokens})")
    model = build_model(a, patch_embed, attn_mask).to(device, dtype=torch.bfloat16)   # main.py:157: bf16 parameters
    if a.rel_pos_bias is not None and rank == 0:
        bi = model.encoder.rel_pos_index
        print(f"relative position bias ({a.rel_pos_bias}): {bi.n_buckets} buckets per head, {bi.visited_blocks}/{bi.total_blocks} "
              f"blocks of 64 x 64 visited (N = {bi.n_tokens})")
    train_criterion, test_criterion = SoftTargetCrossEntropy(), nn.CrossEntropyLoss()
    if a.model_ema_warmup and a.model_ema is None:
        raise SystemExit("--model-ema-warmup needs --model-ema")
    optimizer = FusedAdamW(model.parameters(), lr=a.lr, weight_decay=a.weight_decay, max_grad_norm=1.0,
                           ema_decay=a.model_ema, ema_warmup=a.model_ema_warmup)
    reducer = GradReducer(optimizer, overlap=not a.graph) if world > 1 else None    # --graph: collectives between two graphs
    steps_per_epoch = -(-len(train_loader) // a.accum_steps)        # optimizer steps: the last group of an epoch may be short
    scheduler = WarmupCosine(optimizer, a.warmup_epochs * steps_per_epoch, a.epochs * steps_per_epoch)
    if a.accum_steps > 1 and rank == 0:
        print(f"gradient accumulation: {a.accum_steps} x {a.batch_size} = effective batch {a.accum_steps * a.batch_size}, "
              f"{steps_per_epoch} optimizer steps per epoch")
    start_epoch, best = 0, 0.0
    if a.resume:
        ck = torch.load(a.resume, map_location=device, weights_only=True)
        # the reference saves the torch.compile wrapper's state_dict: same keys behind an "_orig_mod." prefix
        msd = {(k[len("_orig_mod."):] if k.startswith("_orig_mod.") else k): v for k, v in ck["model_state_dict"].items()}
        model.load_state_dict(msd)
        saved = ck.get("rope")                                  # {"kind", "base"} of the run that wrote it: the table is a function of them
        if saved and a.rope is None:
            model.encoder.attach_rope(saved["kind"], saved["base"])
            if rank == 0:
                print(f"rotary position embedding ({saved['kind']}, base {saved['base']:g}): taken from the checkpoint")
        elif saved and (saved["kind"], saved["base"]) != (model.encoder.rope_kind, model.encoder.rope_base):
            raise SystemExit(f"--resume: the checkpoint was trained with --rope {saved['kind']} --rope-base {saved['base']:g}, "
                             f"this run asks for --rope {model.encoder.rope_kind} --rope-base {model.encoder.rope_base:g}")
        osd = ck.get("optimizer_state_dict") or {}
        if osd and not a.resume_model_only:
            # this repository's flat fp32 state (FusedAdamW.state_dict), or a torch.optim.AdamW state_dict as the reference's
            # checkpoints hold (main.py:345-354): Adam moments and step count are mapped into the flat buffers
            optimizer.load_state_dict(osd)
            start_epoch, best = ck["epoch"] + 1, ck.get("test_acc", 0.0)
            ssd = ck.get("scheduler_state_dict") or {}
            # ours: {"n": steps taken}; the reference's LambdaLR (transformers' cosine schedule): {"last_epoch": steps taken}
            scheduler.n = ssd.get("n", ssd.get("last_epoch", start_epoch * steps_per_epoch))
            optimizer.lr = scheduler.lr_at(scheduler.n)
            if augment is not None and ck.get("augment_state_dict"):
                augment.load_state_dict(ck["augment_state_dict"])       # the draw stream goes on where it stopped
    if a.attention_report and attn_mask is not None:
        raise SystemExit("--attention-report measures unmasked attention; it cannot be combined with --attn-window / --attn-window-2d")
    if a.attention_report and a.rel_pos_bias is not None:
        raise SystemExit("--attention-report measures attention without a bias; it cannot be combined with --rel-pos-bias")
    if a.attention_report and a.pool == "cls":
        raise SystemExit("--attention-report has no place in the image for the CLS token; it cannot be combined with --pool cls")
    if a.attention_report and rank == 0:
        import json
        from sfcvit.analysis import attention_report, report_summary
        images, _ = next(iter(test_loader))
        images = images.to(device)
        if test_transform is not None:
            images = test_transform(images)
        summary = report_summary(attention_report(model, images))
        summary.update(tokenizer=a.tokenizer, img_size=a.img_size, heads=a.heads, batch=int(images.shape[0]))
        with open(a.attention_report, "w") as f:
            json.dump(summary, f, indent=1)
        print(f"attention report: {len(summary['layers'])} layers -> {a.attention_report}")
    os.makedirs(a.checkpoint_dir, exist_ok=True)
    ckpt = os.path.join(a.checkpoint_dir, f"checkpoint_{a.tokenizer}.pt")
    graphed = None
    if a.graph:
        model.train()
        images0 = torch.zeros(per_rank, 3, a.img_size, a.img_size, device=device)
        if a.device_mix:
            graphed = GraphedTrainStep(model, images0, None, optimizer, scheduler, reducer=reducer,
                                       mix=BatchMix(per_rank, device),
                                       labels=(torch.zeros(per_rank, dtype=torch.int64, device=device),
                                               torch.zeros(per_rank, dtype=torch.int64, device=device)))
        else:
            graphed = GraphedTrainStep(model, images0, torch.zeros(per_rank, a.classes, device=device), optimizer, scheduler,
                                       reducer=reducer)

    for epoch in range(start_epoch, a.epochs):
        tr_loss, tr_acc = train_with_mixup_or_cutmix(model, train_loader, train_criterion, optimizer, scheduler,
                                                     device, reducer=reducer, graphed=graphed, device_mix=a.device_mix,
                                                     augment=augment, accum_steps=a.accum_steps)
        te_loss, te_acc = evaluate(model, test_loader, test_criterion, device, transform=test_transform)
        ema_loss = ema_acc = 0.0
        if a.model_ema is not None:
            with optimizer.ema_weights():              # the same model, its parameters pointing at the averaged weights
                ema_loss, ema_acc = evaluate(model, test_loader, test_criterion, device, transform=test_transform)
        if world > 1:                                  # equal shards per rank: the global figures are the rank means
            t = torch.tensor([tr_loss, tr_acc, te_loss, te_acc, ema_loss, ema_acc], device=device, dtype=torch.float64)
            dist.all_reduce(t)
            tr_loss, tr_acc, te_loss, te_acc, ema_loss, ema_acc = (t / world).tolist()
        if rank == 0:
            print(f"Epoch {epoch + 1}/{a.epochs} | Train Loss: {tr_loss:.4f}, Train Acc: {tr_acc:.4f} | "
                  f"Test Loss: {te_loss:.4f}, Test Acc: {te_acc:.4f}")            # main.py:331-335
            if a.model_ema is not None:
                print(f"Epoch {epoch + 1}/{a.epochs} | EMA Test Loss: {ema_loss:.4f}, EMA Test Acc: {ema_acc:.4f}")
            if te_acc > best or epoch == start_epoch:
                best = te_acc
                ck = {"epoch": epoch, "model_state_dict": model.state_dict(),
                      "optimizer_state_dict": optimizer.state_dict() if optimizer.master is not None else {},
                      "scheduler_state_dict": {"n": scheduler.n},
                      "augment_state_dict": augment.state_dict() if augment is not None else {}, "train_loss": tr_loss, "train_acc": tr_acc,
                      "test_loss": te_loss, "test_acc": te_acc}                  # main.py:345-354 keys
                if getattr(model.encoder, "rope", None) is not None:
                    ck["rope"] = {"kind": model.encoder.rope_kind, "base": model.encoder.rope_base}
                if a.model_ema is not None:            # the averaged weights under the reference's keys: model.load_state_dict takes them
                    ck.update(model_ema_state_dict=optimizer.ema_state_dict(model), ema_test_acc=ema_acc)
                torch.save(ck, ckpt)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
