"""The reference's per-sample transform stack on the device (include/sfcvit.h, "Train / test image transforms on the
device"): the raw uint8 batch goes in, the augmented, scaled, normalized batch comes out of ONE launch.

The reference runs RandomResizedCrop -> RandomHorizontalFlip -> ColorJitter -> ToDtype(scale) -> RandomErasing ->
Normalize per sample in DataLoader workers (main.py:169-188).  A DeviceAugment draws the same parameters on the host --
one 16-word record per image, every number a pure function of (seed, step, sample index) -- copies them to the device
through pinned memory, and ops.augment_apply reads them when it RUNS, so a captured launch picks up every new draw."""
import numpy as np
import torch

from .. import _lib, ops

CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)      # the reference's Normalize (main.py:176-177)
_SLOTS = 8          # pinned staging records in flight before the host has to look at an event

# record layout, as include/sfcvit.h fixes it
WORDS, FLAGS, CROP, ORDER, FACTORS, ERASE = (_lib.AUG_WORDS, _lib.AUG_FLAGS, _lib.AUG_CROP, _lib.AUG_ORDER, _lib.AUG_FACTORS,
                                             _lib.AUG_ERASE)
FLIP_BIT, ERASE_BIT, JITTER_SHIFT, ORDER_IDENTITY = _lib.AUG_FLIP_BIT, _lib.AUG_ERASE_BIT, _lib.AUG_JITTER_SHIFT, _lib.AUG_ORDER_IDENTITY


def make_cfg(size, mean=CIFAR_MEAN, std=CIFAR_STD, crop=True, flip=True, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0),
             brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, erase_p=0.2, out_dtype=torch.float32):
    """The C struct (sfcvit_augment_cfg) of one transform; the defaults are the reference's train stack."""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
    c = _lib.AugmentCfg()
    c.S, c.crop, c.flip, c.out_is_bf16 = int(size), int(bool(crop)), int(bool(flip)), int(out_dtype == torch.bfloat16)
    c.scale[0], c.scale[1] = float(scale[0]), float(scale[1])
    c.ratio[0], c.ratio[1] = float(ratio[0]), float(ratio[1])
    c.brightness, c.contrast, c.saturation, c.hue, c.erase_p = (float(brightness), float(contrast), float(saturation), float(hue),
                                                                  float(erase_p))
    for i in range(3):
        c.mean[i], c.std[i] = float(mean[i]), float(std[i])
    return c


class DeviceAugment:
    """Transform of uint8 batches [B, C, H, W] to [B, C, size, size] (size defaults to H; needs size >= H, W).

    `.draw()` draws the records of the next step and queues their copy to the device, `aug(u8, out=None)` applies the
    records that are on the device (no draw, no sync, capturable; a shorter batch uses the first rows).  `.rec` is the
    device buffer [B, 16] int32, `.host` the last drawn records (numpy view, do not keep across draws).  `step` counts the
    draws; state_dict / load_state_dict carry seed and counter, so a resumed run continues the stream.  sample_base (an
    attribute, or per draw) offsets the sample index: rank r of a data-parallel run uses r * B."""

    def __init__(self, B, H, W, size=None, mean=CIFAR_MEAN, std=CIFAR_STD, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0),
                 brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, erase_p=0.2, crop=True, flip=True,
                 out_dtype=torch.float32, seed=0, device="cuda"):
        self.B, self.H, self.W = int(B), int(H), int(W)
        self.size = int(size) if size is not None else self.H
        self.device = torch.device(device)
        self.cfg = make_cfg(self.size, mean, std, crop, flip, scale, ratio, brightness, contrast, saturation, hue, erase_p, out_dtype)
        self.random = bool(crop or flip or brightness > 0 or contrast > 0 or saturation > 0 or hue > 0 or erase_p > 0)
        self.out_dtype = out_dtype
        self.seed, self.step, self.sample_base = int(seed), 0, 0
        self.rec = torch.zeros((self.B, WORDS), dtype=torch.int32, device=self.device)
        cuda = self.device.type == "cuda"
        self._stage = torch.zeros((_SLOTS if cuda else 1, self.B, WORDS), dtype=torch.int32)
        if cuda:
            self._stage = self._stage.pin_memory()
        self._events = [None] * _SLOTS
        self._n = 0
        self.host = None
        self._fill(0, 0)          # the records are valid from the start (a test transform never draws again)

    @classmethod
    def test_transform(cls, B, H, W, size=None, mean=CIFAR_MEAN, std=CIFAR_STD, out_dtype=torch.float32, device="cuda"):
        """ToDtype(scale) -> Normalize (resized to `size` when it is larger than the source): flags 0, no draws."""
        return cls(B, H, W, size=size, mean=mean, std=std, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, erase_p=0.0,
                   crop=False, flip=False, out_dtype=out_dtype, device=device)

    def _fill(self, step, sample_base):
        slot = self._n % self._stage.size(0)
        self._n += 1
        if self._events[slot] is not None:
            self._events[slot].synchronize()          # _SLOTS draws ago: complete long since, unless the host runs far ahead
        stage = self._stage[slot]
        ops.augment_draw(stage, self.H, self.W, self.cfg, self.seed, step, sample_base)
        self.rec.copy_(stage, non_blocking=True)      # one small host-to-device copy on the current stream
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            self._events[slot] = ev
        self.host = stage.numpy().view(np.uint32)

    def draw(self, step=None, sample_base=None):
        """Records of step `step` (default: the internal counter, which then advances) for samples sample_base .. + B - 1."""
        if not self.random:
            return self
        if step is None:
            step = self.step
            self.step += 1
        self._fill(int(step), self.sample_base if sample_base is None else int(sample_base))
        return self

    def __call__(self, u8, out=None):
        n = u8.size(0)
        if n > self.B:
            raise ValueError(f"DeviceAugment: batch of {n} images, records for {self.B}")
        return ops.augment_apply(u8, self.rec if n == self.B else self.rec[:n], self.cfg, out=out)

    def state_dict(self):
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, sd):
        self.seed, self.step = int(sd["seed"]), int(sd["step"])
