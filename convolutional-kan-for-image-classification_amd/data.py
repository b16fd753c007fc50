"""Device-resident datasets: the uint8 images and the labels live on the device, and every batch is ONE launch of csrc/kan_feed.hip
(``ops.prepare_batch``: gather by a shuffled index, crop with zero padding, flip, ToTensor, Normalize, the labels) with no host read.

Replaces the transforms, the shuffling and the batching of the reference's loader for its four small datasets (utils/dataloader.py:56-90 and
:111-112: PIL transforms per sample in Python worker processes, then an fp32 copy to the device).  Not carried over: reading the dataset files
and anything that downloads (:92-108: the caller loads ``dataset.data`` / ``dataset.targets`` once and hands them over), and the ImageNet branch
(:26-54: Resize, RandomResizedCrop, Grayscale).

The DISTRIBUTION of torchvision's random transforms is reproduced, not its random stream: crop offsets are uniform over the same range, flips
are fair coins and the order is a uniform permutation, but they are drawn per epoch from a ``torch.Generator`` seeded with (seed, epoch), so
the draws differ from what torchvision would draw from the global generators.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

# mean, std, crop, padding, flip of transform_train / transform_test, utils/dataloader.py:56-90 (the non-ImageNet branch); crop None: no crop
_MNIST = dict(mean=(0.1307,), std=(0.3081,), crop=None, padding=0, flip=False)                                              # :56-61
_SVHN = dict(mean=(0.4377, 0.4438, 0.4728), std=(0.1980, 0.2010, 0.1970), crop=None, padding=0, flip=False)                 # :62-67
_CIFAR10 = dict(mean=(0.4914, 0.4822, 0.4465), std=(0.2470, 0.2435, 0.2616))                                                # :68-78
_CIFAR100 = dict(mean=(0.5071, 0.4867, 0.4408), std=(0.2675, 0.2565, 0.2761))                                               # :79-90
_TRAIN_AUG = dict(crop=32, padding=4, flip=True)                    # RandomCrop(32, padding=4) + RandomHorizontalFlip, :70-71 and :81-82
_PLAIN = dict(crop=None, padding=0, flip=False)
TRANSFORMS = {
    "MNIST": {"train": _MNIST, "test": _MNIST},
    "SVHN": {"train": _SVHN, "test": _SVHN},
    "CIFAR10": {"train": {**_CIFAR10, **_TRAIN_AUG}, "test": {**_CIFAR10, **_PLAIN}},
    "CIFAR100": {"train": {**_CIFAR100, **_TRAIN_AUG}, "test": {**_CIFAR100, **_PLAIN}},
}
# how torchvision's dataset objects hold their images: MNIST .data [N, 28, 28], CIFAR .data [N, 32, 32, 3], SVHN .data [N, 3, 32, 32]
CHANNELS_LAST = {"MNIST": True, "SVHN": False, "CIFAR10": True, "CIFAR100": True}


class DeviceBatches:
    """A re-iterable over (data, target) batches of a uint8 dataset on the device; every ``iter()`` starts the next epoch.

    ``images``: uint8 [N, H, W, C] (``channels_last``), [N, C, H, W] or [N, H, W]; ``labels``: int64 [N] (or None: target is None).
    ``crop``: output size, an int or (Ho, Wo), None for the image's own; ``padding`` p > 0: top and left are drawn uniformly from
    [-p, H - Ho + p] and [-p, W - Wo + p] (``RandomCrop(crop, padding=p)``: [-p, p] when the crop is the image's size), p = 0: the centred
    offset; ``flip``: a fair coin per sample (``RandomHorizontalFlip``); ``shuffle``: a new permutation per epoch (DataLoader's ``shuffle``).
    ``rank`` / ``world_size``: every rank builds the same table from the same seed and takes rows ``rank::world_size``, the tail wrapping
    around as ``DistributedSampler(drop_last=False)`` does.  The table of the running epoch is ``.table`` (int32 [n, 4], rows (index, top,
    left, flip)); a batch is ``ops.prepare_batch`` on ``batch_size`` rows of it.  Nothing on the iteration path reads the device."""

    def __init__(self, images: torch.Tensor, labels: Optional[torch.Tensor], batch_size: int, mean, std, crop=None, padding: int = 0,
                 flip: bool = False, shuffle: bool = False, channels_last: bool = True, drop_last: bool = False, seed: int = 0, rank: int = 0,
                 world_size: int = 1, device=None):
        if device is not None:
            images = images.to(device)
            labels = labels.to(device) if labels is not None else None
        if images.dim() not in (3, 4):
            raise ValueError(f"images must be [N, H, W, C], [N, C, H, W] or [N, H, W], got {tuple(images.shape)}")
        if batch_size < 1 or padding < 0 or world_size < 1 or not 0 <= rank < world_size:
            raise ValueError(f"bad batch_size / padding / rank / world_size: {batch_size}, {padding}, {rank}, {world_size}")
        self.images, self.labels = images.contiguous(), labels.contiguous() if labels is not None else None
        self.N = images.shape[0]
        self.H, self.W = (images.shape[1], images.shape[2]) if channels_last or images.dim() == 3 else (images.shape[2], images.shape[3])
        crop = (self.H, self.W) if crop is None else ((crop, crop) if isinstance(crop, int) else tuple(crop))
        self.out_hw = (int(crop[0]), int(crop[1]))
        self.batch_size, self.mean, self.std = int(batch_size), tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.padding, self.flip, self.shuffle, self.channels_last, self.drop_last = int(padding), bool(flip), bool(shuffle), bool(channels_last), bool(drop_last)
        self.seed, self.rank, self.world_size = int(seed), int(rank), int(world_size)
        self.rows = -(-self.N // self.world_size)                  # rows of this rank's shard
        self.epoch = 0                                             # the epoch the next iter() runs
        self.table = None

    def __len__(self) -> int:
        return self.rows // self.batch_size if self.drop_last else -(-self.rows // self.batch_size)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def epoch_table(self, epoch: int) -> torch.Tensor:
        """int32 [rows, 4] of (index, top, left, flip): a pure function of (seed, epoch, N, the settings), built with torch ops on the device
        of ``images`` (CPU tensors included)."""
        dev, N, (Ho, Wo), p = self.images.device, self.N, self.out_hw, self.padding
        g = torch.Generator(device=dev)
        g.manual_seed((self.seed * 1000003 + int(epoch)) % (1 << 63))
        index = torch.randperm(N, generator=g, device=dev) if self.shuffle else torch.arange(N, device=dev)
        if p > 0:
            top = torch.randint(-p, self.H - Ho + p + 1, (N,), generator=g, device=dev)
            left = torch.randint(-p, self.W - Wo + p + 1, (N,), generator=g, device=dev)
        else:
            top = torch.full((N,), (self.H - Ho) // 2, device=dev, dtype=torch.int64)
            left = torch.full((N,), (self.W - Wo) // 2, device=dev, dtype=torch.int64)
        flip = torch.randint(0, 2, (N,), generator=g, device=dev) if self.flip else torch.zeros((N,), device=dev, dtype=torch.int64)
        table = torch.stack((index, top, left, flip), dim=1).to(torch.int32)
        if self.world_size > 1:
            short = self.rows * self.world_size - N
            if short:
                table = torch.cat((table, table[:short]))
            table = table[self.rank::self.world_size]
        return table.contiguous()

    def __iter__(self):
        self.table = table = self.epoch_table(self.epoch)
        self.epoch += 1
        bs = self.batch_size
        for i in range(len(self)):
            yield ops.prepare_batch(self.images, table[i * bs:(i + 1) * bs], self.out_hw, self.mean, self.std, self.labels, self.channels_last)


def device_batches(dataset: str, train: bool, images: torch.Tensor, labels: Optional[torch.Tensor], batch_size: int, **kw) -> DeviceBatches:
    """The ``DeviceBatches`` of one of the reference's four datasets (``TRANSFORMS``; utils/dataloader.py:56-90) and split; ``shuffle`` follows
    ``train`` (:111-112) and the layout follows torchvision's dataset object (``CHANNELS_LAST``).  Keywords override."""
    if dataset not in TRANSFORMS:
        raise ValueError(f"unknown dataset {dataset!r}: one of {sorted(TRANSFORMS)}")
    settings = dict(TRANSFORMS[dataset]["train" if train else "test"], shuffle=bool(train), channels_last=CHANNELS_LAST[dataset])
    settings.update(kw)
    return DeviceBatches(images, labels, batch_size, **settings)
