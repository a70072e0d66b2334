"""Device-resident description of one batch's MixUp / CutMix (include/sfcvit.h, "MixUp / CutMix on the device").

The reference mixes the image batch with stock torch before the tokenizer and builds dense soft targets behind the logits
(src/training/train.py:7-47, 148-172).  A BatchMix holds the same draw -- partner permutation, lam, CutMix box -- in two
small device buffers that the gather kernels, ops.mix_images and the label-pair loss read when they RUN, so the
augmentation costs no pass of its own and sits inside a captured training step."""
import numpy as np
import torch
import torch.nn.functional as TF

MODE_NONE, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2
_SLOTS = 8          # pinned staging records in flight before the host has to look at an event


class BatchMix:
    """perm (int32 [B]) and rec (int32 [8]: mode, r0, r1, c0, c1, lam bits, (1 - lam) bits, 0) on `device`.

    `.mode`, `.lam`, `.box`, `.idx` keep the host-side values of the last draw: lam is the Python float the reference
    returns (for CutMix the adjusted one, train.py:46), box = (bbx1, bby1, bbx2, bby2) as rand_bbox names them, idx the
    permutation tensor on the device.  The record stores the box as cutmix_data APPLIES it: bbx on dim 2, bby on dim 3."""

    def __init__(self, batch_size, device):
        self.batch_size = int(batch_size)
        self.device = torch.device(device)
        self.perm = torch.arange(self.batch_size, dtype=torch.int32, device=self.device)
        self.rec = torch.zeros(8, dtype=torch.int32, device=self.device)
        self._stage = self._events = None
        if self.device.type == "cuda":
            # a ring of pinned records: the copy of draw n may still be queued when the host writes draw n + 1
            self._stage = torch.zeros((_SLOTS, 8), dtype=torch.int32).pin_memory()
            self._events = [None] * _SLOTS
        self._n = 0
        self.mode, self.lam, self.box, self.idx = MODE_NONE, 1.0, (0, 0, 0, 0), None

    # ---- the record ---------------------------------------------------------------------------------------------
    def _write(self, mode, rows, cols, lam):
        lam = float(lam)
        bits = np.array([lam, 1.0 - lam], dtype=np.float64).astype(np.float32).view(np.int32)   # 1 - lam in double, rounded once
        words = np.array([mode, rows[0], rows[1], cols[0], cols[1], bits[0], bits[1], 0], dtype=np.int32)
        if self._stage is None:
            self.rec.copy_(torch.from_numpy(words))
            return
        slot = self._n % _SLOTS
        self._n += 1
        if self._events[slot] is not None:
            self._events[slot].synchronize()          # _SLOTS draws ago: complete long since, unless the host runs far ahead
        self._stage[slot].copy_(torch.from_numpy(words))
        self.rec.copy_(self._stage[slot], non_blocking=True)      # one small host-to-device copy on the current stream
        ev = torch.cuda.Event()
        ev.record()
        self._events[slot] = ev

    def _set_perm(self, idx):
        if idx.numel() != self.batch_size:
            raise ValueError(f"BatchMix: permutation of {idx.numel()} for a batch of {self.batch_size}")
        self.perm.copy_(idx)                          # narrows int64 -> int32 on the device
        self.idx = idx

    def set_none(self):
        self.mode, self.lam, self.box = MODE_NONE, 1.0, (0, 0, 0, 0)
        self._write(MODE_NONE, (0, 0), (0, 0), 1.0)

    def set_mixup(self, lam, idx):
        """lam * x + (1 - lam) * x[idx] (mixup_data, train.py:7-14)."""
        self._set_perm(idx)
        self.mode, self.lam, self.box = MODE_MIXUP, float(lam), (0, 0, 0, 0)
        self._write(MODE_MIXUP, (0, 0), (0, 0), lam)

    def set_cutmix(self, box, idx, H, W):
        """x[:, :, bbx1:bbx2, bby1:bby2] = x[idx, :, bbx1:bbx2, bby1:bby2] with box = (bbx1, bby1, bbx2, bby2) from
        rand_bbox; lam becomes 1 - box area / (H * W) (cutmix_data, train.py:41-46).  The slices clamp to the tensor's
        extents as torch's do."""
        bbx1, bby1, bbx2, bby2 = (int(v) for v in box)
        self._set_perm(idx)
        lam = 1 - ((bbx2 - bbx1) * (bby2 - bby1) / (H * W))
        self.mode, self.lam, self.box = MODE_CUTMIX, float(lam), (bbx1, bby1, bbx2, bby2)
        rows = (min(max(bbx1, 0), H), min(max(bbx2, 0), H))
        cols = (min(max(bby1, 0), W), min(max(bby2, 0), W))
        self._write(MODE_CUTMIX, rows, cols, lam)

    def draw(self, H, W, mixup_alpha=0.2, cutmix_alpha=1.0, mix_prob=0.5):
        """One batch's augmentation, consuming np.random and torch's generator in the order of
        train_with_mixup_or_cutmix: rand, beta, randperm on the device, and for CutMix rand_bbox's two randints."""
        from .loops import rand_bbox
        if np.random.rand() < mix_prob:
            lam = np.random.beta(mixup_alpha, mixup_alpha) if mixup_alpha > 0 else 1.0
            idx = torch.randperm(self.batch_size, device=self.device)
            self.set_mixup(lam, idx)
        else:
            lam = np.random.beta(cutmix_alpha, cutmix_alpha) if cutmix_alpha > 0 else 1.0
            idx = torch.randperm(self.batch_size, device=self.device)
            self.set_cutmix(rand_bbox(H, W, lam), idx, H, W)
        return self

    # ---- host-side companions -----------------------------------------------------------------------------------
    def dense_targets(self, y_a, y_b, num_classes):
        """The [B, C] fp32 soft targets the reference loop builds (train.py:160), for callers with their own criterion."""
        lam = self.lam
        return lam * TF.one_hot(y_a, num_classes).float() + (1 - lam) * TF.one_hot(y_b, num_classes).float()

    def apply_torch(self, x):
        """The mixed batch as stock torch computes it (new tensor; x is left alone): what the kernels must reproduce."""
        if self.mode == MODE_MIXUP:
            return self.lam * x + (1 - self.lam) * x[self.idx]
        out = x.clone()
        if self.mode == MODE_CUTMIX:
            bbx1, bby1, bbx2, bby2 = self.box
            out[:, :, bbx1:bbx2, bby1:bby2] = x[self.idx, :, bbx1:bbx2, bby1:bby2]
        return out
