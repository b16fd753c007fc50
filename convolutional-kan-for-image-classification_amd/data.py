"""Device-resident datasets: the uint8 images and the labels live on the device, and every batch is ONE launch of csrc/kan_feed.hip
(``ops.prepare_batch``: gather by a shuffled index, crop with zero padding, flip, ToTensor, Normalize, the labels) with no host read.

Replaces the transforms, the shuffling and the batching of the reference's loader for its four small datasets (utils/dataloader.py:56-90 and
:111-112: PIL transforms per sample in Python worker processes, then an fp32 copy to the device).  The loader's ImageNet branch (:26-54:
Resize, RandomResizedCrop / CenterCrop, Grayscale(3); the only way the reference makes 3 x 224 x 224 inputs) is ``ResizedDeviceBatches`` /
``imagenet_device_batches`` on csrc/kan_feed_resize.hip (``ops.prepare_resized_batch``): PIL's 8-bit bilinear resampling is integer
arithmetic once its coefficients are known, ``resample_coeffs`` computes those on the host in float64 with PIL's operations in PIL's order,
and the kernel reproduces PIL's bytes.  Not carried over: reading the dataset files and anything that downloads (:92-108: the caller loads
``dataset.data`` / ``dataset.targets`` once and hands them over).

The DISTRIBUTION of torchvision's random transforms is reproduced, not its random stream: crop offsets and boxes are drawn from the same
distributions, flips are fair coins and the order is a uniform permutation, but they are drawn per epoch from a ``torch.Generator`` seeded
with (seed, epoch), so the draws differ from what torchvision would draw from the global generators.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
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


# ------------------------------------------------------------------------------------------------ the loader's ImageNet branch (:26-54)
def resample_coeffs(n: int, m: int):
    """The coefficients of one of PIL's 8-bit BILINEAR resampling passes from ``n`` to ``m`` samples over the whole axis (``precompute_coeffs``
    and ``normalize_coeffs_8bpc`` of PIL's Resample.c), in numpy float64 with one rounding per operation, in PIL's order:
    ``(bounds int32 [m, 2], k int32 [m, ksize])``, ``bounds[xx] = (xmin, count)``.  Output ``xx`` is
    ``clip((2**21 + sum_{t < count} src[xmin + t] * k[xx, t]) >> 22, 0, 255)``; ``k`` is zero past ``count``.  ``n == m`` is the identity."""
    n, m = int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError(f"resample_coeffs needs n, m >= 1, got {n}, {m}")
    scale = np.float64(n) / np.float64(m)
    fs = max(scale, np.float64(1.0))
    support = fs                                                   # the bilinear filter's support is 1
    ksize = 2 * int(math.ceil(support)) + 1
    ss = np.float64(1.0) / fs
    center = (np.arange(m, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    count = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs((((x + xmin[:, None]).astype(np.float64) - center[:, None]) + 0.5) * ss)
    w = np.where((t < 1.0) & (x < count[:, None]), 1.0 - t, 0.0)
    ww = np.zeros(m, dtype=np.float64)
    for i in range(ksize):                                         # PIL's running sum, in index order (a masked tap adds 0.0)
        ww = ww + w[:, i]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.trunc(0.5 + w * np.float64(1 << 22)).astype(np.int32)   # bilinear weights are never negative
    return np.stack((xmin, count), axis=1).astype(np.int32), k


def resized_hw(H: int, W: int, resize):
    """The size ``Resize(resize)`` gives an H x W image: an int makes the smaller edge ``resize`` and the longer ``int(resize * long / short)``;
    a pair is (Rh, Rw); None is the image's own size."""
    if resize is None:
        return int(H), int(W)
    if isinstance(resize, int):
        if H <= W:
            return resize, int(resize * W / H)
        return int(resize * H / W), resize
    Rh, Rw = resize
    return int(Rh), int(Rw)


class ResizeTables:
    """The four coefficient tables ``kan_feed_resize_batch`` reads for one geometry ``(H, W, Rh, Rw, Ho, Wo)``, as flat int32 tensors of rows
    ``(xmin, count, k[0 .. ksize))``: ``k1x`` (W -> Rw, Rw rows), ``k1y`` (H -> Rh, Rh rows), ``k2x`` (every source length 1 .. Rw -> Wo: block
    ``w - 1`` holds the Wo rows of the pass w -> Wo) and ``k2y`` (1 .. Rh -> Ho); ``ksize`` holds the four row widths (a block of fewer taps is
    zero-padded).  Built on the host once per geometry (``resize_tables``) and uploaded once (``.to(device)``)."""

    def __init__(self, geometry, tables, ksize):
        self.geometry, self.tables, self.ksize = tuple(int(v) for v in geometry), tuple(tables), tuple(int(v) for v in ksize)

    @property
    def device(self):
        return self.tables[0].device

    def to(self, device) -> "ResizeTables":
        return ResizeTables(self.geometry, [t.to(device) for t in self.tables], self.ksize)


def _packed_rows(passes, ksize):
    rows = []
    for bounds, k in passes:
        rows.append(np.concatenate((bounds, k, np.zeros((k.shape[0], ksize - k.shape[1]), dtype=np.int32)), axis=1))
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(rows, axis=0).reshape(-1)))


def resize_tables(H: int, W: int, Rh: int, Rw: int, Ho: int, Wo: int, device=None) -> ResizeTables:
    """``ResizeTables`` of the pipeline resize H x W -> Rh x Rw, crop any box, resize the box -> Ho x Wo."""
    if min(H, W, Rh, Rw, Ho, Wo) < 1:
        raise ValueError(f"resize_tables needs sizes >= 1, got {(H, W, Rh, Rw, Ho, Wo)}")
    tables, ksize = [], []
    for passes in ([resample_coeffs(W, Rw)], [resample_coeffs(H, Rh)], [resample_coeffs(w, Wo) for w in range(1, Rw + 1)],
                   [resample_coeffs(h, Ho) for h in range(1, Rh + 1)]):
        ksize.append(max(k.shape[1] for _, k in passes))
        tables.append(_packed_rows(passes, ksize[-1]))
    t = ResizeTables((H, W, Rh, Rw, Ho, Wo), tables, ksize)
    return t.to(device) if device is not None else t


class ResizedDeviceBatches:
    """``DeviceBatches`` for the loader's ImageNet branch (utils/dataloader.py:26-54): every batch is one ``ops.prepare_resized_batch`` --
    ``Resize(resize)`` of the whole image, a crop box, ``Resize`` of the box to ``crop``, flip, optional ``Grayscale(3)``, ToTensor, Normalize,
    with PIL's 8-bit bilinear bytes.

    ``images`` / ``labels`` / ``batch_size`` / ``shuffle`` / ``channels_last`` / ``drop_last`` / ``seed`` / ``rank`` / ``world_size`` / ``device`` and
    ``__len__`` / ``set_epoch`` / sharding are ``DeviceBatches``'; ``mean`` / ``std`` hold ``out_channels`` values (default: the images' C; 3 with
    C == 1 replicates the channel).  ``resize``: an int (``Resize(int)``: the smaller edge becomes ``resize``, the longer
    ``int(resize * long / short)``), a pair (Rh, Rw) or None (no stage-1 resize).  ``crop``: the output size, an int or (Ho, Wo); None: the
    stage-1 size, and the box is the whole stage-1 image.  Without ``random_resized_crop`` the box is ``CenterCrop(crop)``'s:
    ``top = int(round((Rh - Ho) / 2.0))``, likewise left, ``h, w = Ho, Wo`` (the crop must fit the stage-1 image).  With
    ``random_resized_crop=(scale, ratio)`` (True: torchvision's defaults (0.08, 1.0), (3/4, 4/3)) the boxes follow
    ``RandomResizedCrop.get_params``: ten attempts per sample of ``area * U(scale)``, ``exp(U(log ratio))``, ``w = round(sqrt(a * r))``,
    ``h = round(sqrt(a / r))``; the first attempt with ``0 < w <= Rw`` and ``0 < h <= Rh`` wins, with top uniform over ``[0, Rh - h]`` and left over
    ``[0, Rw - w]``; otherwise the centred box of full extent clamped to the ratio range.  All samples are drawn at once with torch ops on the
    images' device from a (seed, epoch) generator: the distribution is reproduced, not torchvision's random stream.  torchvision is not
    installed where this was written: the description above is the maintainer's reading of ``RandomResizedCrop``, ``CenterCrop`` and
    ``Resize`` and was not checked against torchvision itself.

    The table of the running epoch is ``.table`` (int32 [n, 6], rows (index, top, left, h, w, flip) in stage-1 coordinates).  The coefficient
    tables (``.coeffs``) are built and uploaded at construction; nothing on the iteration path reads the device."""

    def __init__(self, images: torch.Tensor, labels: Optional[torch.Tensor], batch_size: int, mean, std, resize=None, crop=None,
                 random_resized_crop=None, flip: bool = False, out_channels: Optional[int] = None, shuffle: bool = False,
                 channels_last: bool = True, drop_last: bool = False, seed: int = 0, rank: int = 0, world_size: int = 1, device=None):
        if device is not None:
            images = images.to(device)
            labels = labels.to(device) if labels is not None else None
        if images.dim() not in (3, 4):
            raise ValueError(f"images must be [N, H, W, C], [N, C, H, W] or [N, H, W], got {tuple(images.shape)}")
        if batch_size < 1 or world_size < 1 or not 0 <= rank < world_size:
            raise ValueError(f"bad batch_size / rank / world_size: {batch_size}, {rank}, {world_size}")
        self.images, self.labels = images.contiguous(), labels.contiguous() if labels is not None else None
        self.N = images.shape[0]
        self.H, self.W = (images.shape[1], images.shape[2]) if channels_last or images.dim() == 3 else (images.shape[2], images.shape[3])
        self.resize = resized_hw(self.H, self.W, resize)
        crop = self.resize if crop is None else ((crop, crop) if isinstance(crop, int) else tuple(crop))
        self.out_hw = (int(crop[0]), int(crop[1]))
        if random_resized_crop is True:
            random_resized_crop = ((0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0))
        self.random_resized_crop = tuple(tuple(float(v) for v in r) for r in random_resized_crop) if random_resized_crop else None
        Rh, Rw = self.resize
        if self.random_resized_crop is None and (self.out_hw[0] > Rh or self.out_hw[1] > Rw):
            raise ValueError(f"a centre crop of {self.out_hw} does not fit the resized image {self.resize}")
        self.batch_size, self.mean, self.std = int(batch_size), tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.out_channels = int(out_channels) if out_channels is not None else None
        self.flip, self.shuffle, self.channels_last, self.drop_last = bool(flip), bool(shuffle), bool(channels_last), bool(drop_last)
        self.seed, self.rank, self.world_size = int(seed), int(rank), int(world_size)
        self.rows = -(-self.N // self.world_size)                  # rows of this rank's shard
        self.epoch = 0                                             # the epoch the next iter() runs
        self.table = None
        self.coeffs = resize_tables(self.H, self.W, Rh, Rw, *self.out_hw, device=self.images.device)

    __len__ = DeviceBatches.__len__
    set_epoch = DeviceBatches.set_epoch

    def _boxes(self, g):
        """(top, left, h, w), int64 [N] each, of this epoch."""
        dev, N, (Rh, Rw), (Ho, Wo) = self.images.device, self.N, self.resize, self.out_hw
        if self.random_resized_crop is None:
            if (Ho, Wo) == (Rh, Rw):
                box = (0, 0, Rh, Rw)
            else:
                box = (int(round((Rh - Ho) / 2.0)), int(round((Rw - Wo) / 2.0)), Ho, Wo)
            return tuple(torch.full((N,), v, device=dev, dtype=torch.int64) for v in box)
        (s0, s1), (r0, r1) = self.random_resized_crop
        tries = 10
        area = float(Rh * Rw) * (s0 + (s1 - s0) * torch.rand((N, tries), generator=g, device=dev, dtype=torch.float64))
        lr0, lr1 = math.log(r0), math.log(r1)
        ratio = torch.exp(lr0 + (lr1 - lr0) * torch.rand((N, tries), generator=g, device=dev, dtype=torch.float64))
        w = torch.round(torch.sqrt(area * ratio)).long()
        h = torch.round(torch.sqrt(area / ratio)).long()
        fits = (w > 0) & (w <= Rw) & (h > 0) & (h <= Rh)
        first = torch.argmax(fits.to(torch.int8), dim=1, keepdim=True)          # the first attempt that fits (0 when none does)
        found = fits.any(dim=1)
        w, h = w.gather(1, first).squeeze(1), h.gather(1, first).squeeze(1)
        u_top = torch.rand((N,), generator=g, device=dev, dtype=torch.float64)
        u_left = torch.rand((N,), generator=g, device=dev, dtype=torch.float64)
        # the fallback: the centred box of full extent, clamped to the ratio range
        in_ratio = float(Rw) / float(Rh)
        if in_ratio < min(r0, r1):
            fw, fh = Rw, int(round(Rw / min(r0, r1)))
        elif in_ratio > max(r0, r1):
            fh, fw = Rh, int(round(Rh * max(r0, r1)))
        else:
            fw, fh = Rw, Rh
        fh, fw = max(1, min(fh, Rh)), max(1, min(fw, Rw))
        w = torch.where(found, w, torch.full_like(w, fw))
        h = torch.where(found, h, torch.full_like(h, fh))
        top = torch.minimum((u_top * (Rh - h + 1).double()).long(), Rh - h)       # randint(0, Rh - h + 1)
        left = torch.minimum((u_left * (Rw - w + 1).double()).long(), Rw - w)
        top = torch.where(found, top, torch.full_like(top, (Rh - fh) // 2))
        left = torch.where(found, left, torch.full_like(left, (Rw - fw) // 2))
        return top, left, h, w

    def epoch_table(self, epoch: int) -> torch.Tensor:
        """int32 [rows, 6] of (index, top, left, h, w, flip): a pure function of (seed, epoch, N, the settings), built with torch ops on the
        device of ``images`` (CPU tensors included)."""
        dev, N = self.images.device, self.N
        g = torch.Generator(device=dev)
        g.manual_seed((self.seed * 1000003 + int(epoch)) % (1 << 63))
        index = torch.randperm(N, generator=g, device=dev) if self.shuffle else torch.arange(N, device=dev)
        top, left, h, w = self._boxes(g)
        flip = torch.randint(0, 2, (N,), generator=g, device=dev) if self.flip else torch.zeros((N,), device=dev, dtype=torch.int64)
        table = torch.stack((index, top, left, h, w, flip), dim=1).to(torch.int32)
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
            yield ops.prepare_resized_batch(self.images, table[i * bs:(i + 1) * bs], self.resize, self.out_hw, self.mean, self.std, self.labels,
                                            self.channels_last, self.out_channels, self.coeffs)


# the transforms of utils/dataloader.py:9-54 (imagenet_preprocessing=True) per dataset and split
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)                                                   # :9-10
_IMAGENET_NORM = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD)
_IMAGENET_MNIST = dict(**_IMAGENET_NORM, resize=224, crop=None, random_resized_crop=None, flip=False, out_channels=3)       # :29-40
_IMAGENET_TRAIN = dict(**_IMAGENET_NORM, resize=256, crop=224, random_resized_crop=((0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)), flip=True,
                       out_channels=3)                                                                                       # :42-48
_IMAGENET_TEST = dict(**_IMAGENET_NORM, resize=256, crop=224, random_resized_crop=None, flip=False, out_channels=3)         # :49-54
IMAGENET_TRANSFORMS = {
    "MNIST": {"train": _IMAGENET_MNIST, "test": _IMAGENET_MNIST},
    "SVHN": {"train": _IMAGENET_TRAIN, "test": _IMAGENET_TEST},
    "CIFAR10": {"train": _IMAGENET_TRAIN, "test": _IMAGENET_TEST},
    "CIFAR100": {"train": _IMAGENET_TRAIN, "test": _IMAGENET_TEST},
}


def imagenet_device_batches(dataset: str, train: bool, images: torch.Tensor, labels: Optional[torch.Tensor], batch_size: int,
                            **kw) -> ResizedDeviceBatches:
    """The ``ResizedDeviceBatches`` of one of the reference's four datasets under ``--imagenet_preprocessing`` (``IMAGENET_TRANSFORMS``;
    utils/dataloader.py:26-54) and split; ``shuffle`` follows ``train`` (:111-112) and the layout torchvision's dataset object
    (``CHANNELS_LAST``).  Keywords override."""
    if dataset not in IMAGENET_TRANSFORMS:
        raise ValueError(f"unknown dataset {dataset!r}: one of {sorted(IMAGENET_TRANSFORMS)}")
    settings = dict(IMAGENET_TRANSFORMS[dataset]["train" if train else "test"], shuffle=bool(train), channels_last=CHANNELS_LAST[dataset])
    settings.update(kw)
    return ResizedDeviceBatches(images, labels, batch_size, **settings)
