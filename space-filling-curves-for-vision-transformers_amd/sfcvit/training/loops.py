"""Epoch loops with the semantics of src/training/train.py (MixUp / CutMix, soft-target CE, clip 1.0,
optimizer + scheduler step per batch; evaluate = eval-mode forward + CE + accuracy), on the HIP modules.

Differences that do not change the math: no torch.autocast (the modules compute in bf16 with fp32
accumulation themselves), running loss / accuracy stay on the device and are read once per epoch
(the reference calls .item() twice per step, train.py:170-172), and FusedAdamW.step() does the
clip_grad_norm_(1.0) inside the optimizer kernel (train.py:165-166).

accum_steps=K (every training loop): K consecutive loader batches form ONE optimizer step -- the loader's batch is the
micro-batch, each draws its own mix, loss / accuracy bookkeeping stays per micro-batch, and the last group of an epoch steps
with as many batches as it has (sfcvit.training.train.AccumSteps holds the sequence).  Needs len(train_loader)."""
import numpy as np
import torch
import torch.nn.functional as TF

from .optim import FusedAdamW
from .train import AccumSteps


def mixup_data(x, y, alpha=0.2):
    """train.py:7-14."""
    lam = np.random.beta(alpha, alpha) if alpha > 0 else 1.0
    idx = torch.randperm(x.size(0), device=x.device)
    return lam * x + (1 - lam) * x[idx], y, y[idx], lam


def rand_bbox(H, W, lam):
    """train.py:17-30."""
    cut_rat = np.sqrt(1.0 - lam)
    cut_w, cut_h = int(W * cut_rat), int(H * cut_rat)
    cx, cy = np.random.randint(W), np.random.randint(H)
    return (np.clip(cx - cut_w // 2, 0, W), np.clip(cy - cut_h // 2, 0, H),
            np.clip(cx + cut_w // 2, 0, W), np.clip(cy + cut_h // 2, 0, H))


def cutmix_data(x, y, alpha=0.2):
    """train.py:33-47 (mutates x in place, as the reference does)."""
    lam = np.random.beta(alpha, alpha) if alpha > 0 else 1.0
    _, _, H, W = x.size()
    idx = torch.randperm(x.size(0), device=x.device)
    bbx1, bby1, bbx2, bby2 = rand_bbox(H, W, lam)
    x[:, :, bbx1:bbx2, bby1:bby2] = x[idx, :, bbx1:bbx2, bby1:bby2]
    lam = 1 - ((bbx2 - bbx1) * (bby2 - bby1) / (H * W))
    return x, y, y[idx], lam


def mixup_criterion(criterion, pred, y_a, y_b, lam):
    """train.py:50-54."""
    return lam * criterion(pred, y_a) + (1 - lam) * criterion(pred, y_b)


def _augmented(images, augment, graphed=None):
    """augment= (a sfcvit.training.DeviceAugment): the loader's batch is the raw uint8 one; draw this step's records and
    transform it on the device -- straight into the graphed step's static image buffer when the result fits it."""
    augment.draw()
    dst = None
    if graphed is not None and graphed.images.dtype == augment.out_dtype and \
            tuple(graphed.images.shape) == (images.size(0), images.size(1), augment.size, augment.size):
        dst = graphed.images
    return augment(images, out=dst)


def _accum_seq(train_loader, optimizer, scheduler, reducer, accum_steps, clip=None):
    return AccumSteps(optimizer, scheduler, reducer, n_batches=len(train_loader) if accum_steps != 1 else None,
                      accum_steps=accum_steps, clip_params=clip)


def _clip_params(model, optimizer):
    """The loops of train.py:133-178 clip to 1.0; FusedAdamW does that inside its kernel."""
    return None if isinstance(optimizer, FusedAdamW) else list(model.parameters())


def _plain_epoch(model, train_loader, criterion, optimizer, scheduler, device, augment=None, accum_steps=1):
    model.train()
    total_loss = torch.zeros((), device=device)
    correct = torch.zeros((), device=device)
    seq = _accum_seq(train_loader, optimizer, scheduler, None, accum_steps)
    for i, (images, labels) in enumerate(train_loader):
        images, labels = images.to(device), labels.to(device)
        if augment is not None:
            images = _augmented(images, augment)
        seq.begin(i)
        outputs = model(images)
        loss = criterion(outputs.float(), labels)
        seq.backward(loss)
        seq.end()
        total_loss += loss.detach().float() * images.size(0)
        correct += (outputs.argmax(dim=1) == labels).sum()
    n = len(train_loader.dataset)
    return float(total_loss) / n, float(correct) / n


def train(model, train_loader, criterion, optimizer, device, augment=None, accum_steps=1):
    """train.py:57-77: hard labels, no scheduler.  The reference does not clip here: construct
    FusedAdamW(..., max_grad_norm=None) for the same behaviour.  augment: see train_with_mixup_or_cutmix."""
    return _plain_epoch(model, train_loader, criterion, optimizer, None, device, augment, accum_steps)


def train_with_scheduler(model, train_loader, criterion, optimizer, scheduler, device, augment=None, accum_steps=1):
    """train.py:102-130: as `train` with a per-step scheduler (one scheduler step per optimizer step)."""
    return _plain_epoch(model, train_loader, criterion, optimizer, scheduler, device, augment, accum_steps)


def _device_mix_epoch(model, train_loader, optimizer, scheduler, device, mixup_alpha, cutmix_alpha, mix_prob, reducer, graphed,
                      augment=None, accum_steps=1):
    """train_with_mixup_or_cutmix(device_mix=True): the same draws, but the batch is mixed where the tokenizer reads it
    (model(images, mix=bm)) and the loss / accuracy come from the label pair (F.mixed_target_cross_entropy)."""
    from .. import functional as F
    from .mix import BatchMix
    model.train()
    total_loss = torch.zeros((), device=device)
    total_correct = torch.zeros((), device=device)
    total_samples = 0
    mixes = {}                                       # one record per batch size (the last batch of an epoch may be short)
    seq = _accum_seq(train_loader, optimizer, scheduler, reducer, accum_steps, _clip_params(model, optimizer))
    for i, (images, labels) in enumerate(train_loader):
        images, labels = images.to(device), labels.to(device)
        if augment is not None:
            images = _augmented(images, augment, graphed if graphed is not None and graphed.mix is not None else None)
        B, (H, W) = images.size(0), images.shape[2:]
        if graphed is not None and graphed.mix is not None and images.shape == graphed.images.shape:
            bm = graphed.mix.draw(H, W, mixup_alpha, cutmix_alpha, mix_prob)
            if images is not graphed.images:
                graphed.images.copy_(images)
            graphed.labels[0].copy_(labels)
            torch.index_select(labels, 0, bm.idx, out=graphed.labels[1])
            loss = graphed()
            total_correct += graphed.hits.sum()
            total_loss += loss.float() * B
            total_samples += B
            continue
        bm = mixes.get(B)
        if bm is None:
            bm = mixes[B] = BatchMix(B, images.device)
        bm.draw(H, W, mixup_alpha, cutmix_alpha, mix_prob)
        y_a, y_b = labels, labels[bm.idx]
        seq.begin(i)
        outputs = model(images, mix=bm)
        loss, hits = F.mixed_target_cross_entropy(outputs, y_a, y_b, bm)
        seq.backward(loss)
        seq.end()
        total_correct += hits.sum()
        total_loss += loss.detach().float() * B
        total_samples += B
    return float(total_loss) / total_samples, float(total_correct) / total_samples


def train_with_mixup_or_cutmix(model, train_loader, criterion, optimizer, scheduler, device,
                               mixup_alpha=0.2, cutmix_alpha=1.0, mix_prob=0.5, reducer=None, graphed=None, device_mix=False,
                               augment=None, accum_steps=1):
    """train.py:133-178.  `optimizer` is a FusedAdamW (clip inside) or any torch optimizer.
    graphed: a sfcvit.training.GraphedTrainStep built on this model / optimizer / scheduler with static buffers of the
    loader's batch shape -- the step (forward, soft-target CE, backward, clip, AdamW, scheduler) is then one hipGraph
    replay per batch (what main.py:284's torch.compile(mode="reduce-overhead") is after); batches of another size run
    eagerly.
    device_mix: MixUp / CutMix on the device (sfcvit.training.BatchMix): the same seeded draws, the batch mixed inside
    the tokenizer's gather and the loss / accuracy taken from the label pair; `criterion` is not called (the loss is
    soft-target cross entropy, as main.py's).  With a GraphedTrainStep(mix=..., labels=...) the augmentation is part
    of the replayed step.
    augment: a sfcvit.training.DeviceAugment -- the loader then yields the raw uint8 batches [B, C, H, W] and the
    reference's transform stack (main.py:169-188) runs on the device in front of the mix, one launch per batch; with a
    device-mix GraphedTrainStep the result is written straight into its static image buffer.  None = float batches, as
    before.
    accum_steps: K loader batches per optimizer step (the module docstring); not together with `graphed`."""
    if graphed is not None and accum_steps != 1:
        raise ValueError("accum_steps > 1 with a GraphedTrainStep: a captured step does not accumulate")
    if device_mix:
        return _device_mix_epoch(model, train_loader, optimizer, scheduler, device, mixup_alpha, cutmix_alpha, mix_prob,
                                 reducer, graphed, augment, accum_steps)
    model.train()
    total_loss = torch.zeros((), device=device)
    total_correct = torch.zeros((), device=device)
    total_samples = 0
    seq = _accum_seq(train_loader, optimizer, scheduler, reducer, accum_steps, _clip_params(model, optimizer))
    for i, (images, labels) in enumerate(train_loader):
        images, labels = images.to(device), labels.to(device)
        if augment is not None:
            images = _augmented(images, augment)
        if np.random.rand() < mix_prob:
            images, y_a, y_b, lam = mixup_data(images, labels, alpha=mixup_alpha)
        else:
            images, y_a, y_b, lam = cutmix_data(images, labels, alpha=cutmix_alpha)
        if graphed is not None and images.shape == graphed.images.shape:
            num_classes = graphed.targets.size(1)
            graphed.images.copy_(images)
            graphed.targets.copy_(lam * TF.one_hot(y_a, num_classes).float() + (1 - lam) * TF.one_hot(y_b, num_classes).float())
            loss = graphed()
            outputs = graphed.logits
            preds = outputs.argmax(dim=1)
            total_correct += (lam * (preds == y_a).float() + (1 - lam) * (preds == y_b).float()).sum()
            total_loss += loss.float() * images.size(0)
            total_samples += images.size(0)
            continue
        seq.begin(i)                     # (also for a batch the graph cannot replay, odd size: the device step state advances here)
        outputs = model(images)
        num_classes = outputs.size(1)
        soft_targets = lam * TF.one_hot(y_a, num_classes).float() + (1 - lam) * TF.one_hot(y_b, num_classes).float()
        loss = criterion(outputs, soft_targets)
        seq.backward(loss)
        seq.end()
        preds = outputs.argmax(dim=1)
        total_correct += (lam * (preds == y_a).float() + (1 - lam) * (preds == y_b).float()).sum()
        total_loss += loss.detach().float() * images.size(0)
        total_samples += images.size(0)
    return float(total_loss) / total_samples, float(total_correct) / total_samples


def evaluate(model, test_loader, criterion, device, transform=None):
    """train.py:80-99.  transform: a DeviceAugment.test_transform (any callable on the device batch) -- the loader then
    yields raw uint8 batches."""
    model.eval()
    total_loss = torch.zeros((), device=device)
    correct = torch.zeros((), device=device)
    n = 0
    with torch.no_grad():
        for images, labels in test_loader:
            images, labels = images.to(device), labels.to(device)
            if transform is not None:
                images = transform(images)
            outputs = model(images)
            total_loss += criterion(outputs.float(), labels) * images.size(0)
            correct += (outputs.argmax(dim=1) == labels).sum()
            n += images.size(0)
    return float(total_loss) / n, float(correct) / n
