"""Device-resident datasets, off the device: the C ABI of csrc/kan_feed.hip is declared, bound and refuses bad arguments by host arithmetic;
``ops.prepare_batch`` refuses what it cannot take; ``DeviceBatches.epoch_table`` (torch ops on the device of the images, so it runs on CPU
tensors) draws what the reference's transforms and DataLoader draw -- in distribution, not in stream; ``TRANSFORMS`` holds the values of
utils/dataloader.py:56-90; and the restatement the GPU tests compare against (feed_cases.py) places pixels as PIL does."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import convkan_amd as K
from convkan_amd import _lib as L
from convkan_amd.data import CHANNELS_LAST
import feed_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("kan_feed_batch", "kan_feed_max_image_bytes")


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "kanconv.h")).read()
    declared = set(re.findall(r"\b(kan_[a-z_]+)\s*\(", header))
    for name in ENTRY_POINTS:
        assert name in declared and name in L.SIGNATURES, name
    K.build_library()
    lib = L.load()
    raw = C.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), name
    assert lib.kan_feed_max_image_bytes() >= 65536
    for name in ("DeviceBatches", "device_batches", "TRANSFORMS"):
        assert hasattr(K, name), name
    assert callable(K.ops.prepare_batch)
    assert list(inspect.signature(K.ops.prepare_batch).parameters) == ["images", "table", "out_hw", "mean", "std", "labels", "channels_last", "out"]
    assert list(inspect.signature(K.DeviceBatches.__init__).parameters)[1:] == [
        "images", "labels", "batch_size", "mean", "std", "crop", "padding", "flip", "shuffle", "channels_last", "drop_last", "seed", "rank",
        "world_size", "device"]


def test_launcher_refuses_bad_arguments_without_a_device():
    K.build_library()
    lib = L.load()
    p, null, st = C.c_void_p(64), C.c_void_p(0), C.c_void_p(0)           # never dereferenced: every call below is refused before a launch
    host = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)

    def refused(rc, word):
        assert rc < 0
        msg = lib.kan_last_error().decode()
        assert word in msg, msg

    def args(**kw):
        a = dict(images=p, labels=p, table=p, N=10, B=4, C=3, H=8, W=8, Ho=8, Wo=8, cl=1, mean=host, std=host, data=p, target=p, stream=st)
        a.update(kw)
        return list(a.values())
    for name in ("images", "table", "mean", "std", "data"):
        refused(lib.kan_feed_batch(*args(**{name: null})), "kan_feed_batch: null pointer")
    refused(lib.kan_feed_batch(*args(labels=null)), "labels and target")          # one of the pair alone
    refused(lib.kan_feed_batch(*args(target=null)), "labels and target")
    for name in ("N", "B", "C", "H", "W", "Ho", "Wo"):
        refused(lib.kan_feed_batch(*args(**{name: 0})), "must be at least 1")
    refused(lib.kan_feed_batch(*args(C=5)), "at most 4 channels")
    limit = lib.kan_feed_max_image_bytes()
    refused(lib.kan_feed_batch(*args(C=1, H=1, W=limit + 1)), "at most 65536 bytes")
    refused(lib.kan_feed_batch(*args(C=4, H=129, W=128)), "at most 65536 bytes")


def test_prepare_batch_refuses_what_it_cannot_take():
    K.build_library()
    images = torch.zeros(6, 8, 8, 3, dtype=torch.uint8)
    table = torch.zeros(2, 4, dtype=torch.int32)
    mean, std = (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        K.ops.prepare_batch(images, table, (8, 8), mean, std)
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        K.ops.prepare_batch(images, table, (8, 8), mean, std, labels=torch.zeros(6, dtype=torch.int64))
    for bad, word in (
            (dict(images=images.float()), "uint8"),
            (dict(images=torch.zeros(6, 8, 3, 8, dtype=torch.uint8).transpose(2, 3)), "contiguous"),
            (dict(table=table.long()), "int32"),
            (dict(table=torch.zeros(2, 8, dtype=torch.int32)[:, ::2]), "contiguous"),
            (dict(table=torch.zeros(2, 3, dtype=torch.int32)), r"\[B, 4\]"),
            (dict(images=torch.zeros(6, 8, 8, 5, dtype=torch.uint8), mean=(0.5,) * 5, std=(0.5,) * 5), "at most 4 channels"),
            (dict(images=torch.zeros(2, 5, 8, 8, dtype=torch.uint8), channels_last=False, mean=(0.5,) * 5, std=(0.5,) * 5), "at most 4 channels"),
            (dict(images=torch.zeros(2, 128, 129, 4, dtype=torch.uint8), mean=(0.5,) * 4, std=(0.5,) * 4), "bytes"),
            (dict(mean=(0.5,)), "mean and std"),
            (dict(out_hw=(0, 8)), "out_hw"),
            (dict(labels=torch.zeros(6, dtype=torch.int32)), "labels"),
            (dict(labels=torch.zeros(5, dtype=torch.int64)), "labels")):
        kw = dict(images=images, table=table, out_hw=(8, 8), mean=mean, std=std)
        kw.update(bad)
        with pytest.raises(L.KanConvError, match=word):
            K.ops.prepare_batch(**kw)


def _cifar_train(N=2000, seed=0, **kw):
    return K.DeviceBatches(torch.zeros(N, 32, 32, 3, dtype=torch.uint8), torch.arange(N), 8, FC.CIFAR10_MEAN, FC.CIFAR10_STD, crop=32, padding=4,
                           flip=True, shuffle=True, seed=seed, **kw)


def test_epoch_table_draws():
    N, p = 2000, 4
    d = _cifar_train(N)
    t0, t1 = d.epoch_table(0), d.epoch_table(1)
    assert t0.dtype == torch.int32 and tuple(t0.shape) == (N, 4) and t0.device.type == "cpu" and t0.is_contiguous()
    assert sorted(t0[:, 0].tolist()) == list(range(N)) and sorted(t1[:, 0].tolist()) == list(range(N))
    assert torch.equal(d.epoch_table(0), t0) and torch.equal(_cifar_train(N).epoch_table(0), t0)      # a pure function of (seed, epoch)
    assert not torch.equal(t0, t1) and not torch.equal(t0[:, 0], t1[:, 0])
    assert not torch.equal(_cifar_train(N, seed=1).epoch_table(0), t0)
    for col in (1, 2):
        assert sorted(set(t0[:, col].tolist())) == list(range(-p, p + 1))                             # inside [-p, p], every value drawn
    assert sorted(set(t0[:, 3].tolist())) == [0, 1]
    assert t0[:, 0].tolist() != list(range(N))


def test_epoch_table_without_randomness_and_crops():
    imgs = torch.zeros(10, 3, 12, 9, dtype=torch.uint8)                                               # CHW: H 12, W 9
    d = K.DeviceBatches(imgs, None, 4, (0.5,) * 3, (0.5,) * 3, crop=(8, 5), channels_last=False)
    t = d.epoch_table(0)
    assert d.out_hw == (8, 5) and torch.equal(t, d.epoch_table(7))
    assert torch.equal(t, torch.tensor([[i, 2, 2, 0] for i in range(10)], dtype=torch.int32))         # (arange, centred, centred, 0)
    plain = K.DeviceBatches(imgs, None, 4, (0.5,) * 3, (0.5,) * 3, channels_last=False)
    assert plain.out_hw == (12, 9) and torch.equal(plain.epoch_table(0), torch.tensor([[i, 0, 0, 0] for i in range(10)], dtype=torch.int32))
    # RandomCrop(crop, padding=p) on a larger image: top in [-p, H - crop + p]
    r = K.DeviceBatches(torch.zeros(3000, 12, 9, dtype=torch.uint8), None, 4, (0.5,), (0.5,), crop=(8, 5), padding=1).epoch_table(0)
    assert sorted(set(r[:, 1].tolist())) == list(range(-1, 12 - 8 + 1 + 1)) and sorted(set(r[:, 2].tolist())) == list(range(-1, 9 - 5 + 1 + 1))


def test_epoch_table_shards_like_a_distributed_sampler():
    N, ws = 37, 3
    shards = [_cifar_train(N, rank=r, world_size=ws).epoch_table(2) for r in range(ws)]
    whole = _cifar_train(N).epoch_table(2)
    assert all(tuple(s.shape) == (13, 4) for s in shards)
    assert set(torch.cat(shards)[:, 0].tolist()) == set(range(N))
    padded = torch.cat((whole, whole[:2]))                                                           # 39 rows: the tail wraps around
    for r in range(ws):
        assert torch.equal(shards[r], padded[r::ws])
    assert len(_cifar_train(N, rank=1, world_size=ws)) == 2                                           # ceil(13 / 8)
    with pytest.raises(ValueError):
        _cifar_train(N, rank=3, world_size=3)


def test_len_with_and_without_drop_last():
    for N, bs, full, kept in ((37, 8, 5, 4), (40, 8, 5, 5), (7, 8, 1, 0), (1, 1, 1, 1)):
        imgs = torch.zeros(N, 4, 4, 1, dtype=torch.uint8)
        assert len(K.DeviceBatches(imgs, None, bs, (0.5,), (0.5,))) == full
        assert len(K.DeviceBatches(imgs, None, bs, (0.5,), (0.5,), drop_last=True)) == kept


def test_transforms_hold_the_reference_values():
    """utils/dataloader.py:56-90."""
    T = K.TRANSFORMS
    assert set(T) == {"MNIST", "SVHN", "CIFAR10", "CIFAR100"} and all(set(v) == {"train", "test"} for v in T.values())
    plain, aug = dict(crop=None, padding=0, flip=False), dict(crop=32, padding=4, flip=True)
    assert T["MNIST"]["train"] == T["MNIST"]["test"] == dict(mean=(0.1307,), std=(0.3081,), **plain)
    assert T["SVHN"]["train"] == T["SVHN"]["test"] == dict(mean=(0.4377, 0.4438, 0.4728), std=(0.1980, 0.2010, 0.1970), **plain)
    c10 = dict(mean=(0.4914, 0.4822, 0.4465), std=(0.2470, 0.2435, 0.2616))
    c100 = dict(mean=(0.5071, 0.4867, 0.4408), std=(0.2675, 0.2565, 0.2761))
    assert T["CIFAR10"]["train"] == dict(**c10, **aug) and T["CIFAR10"]["test"] == dict(**c10, **plain)
    assert T["CIFAR100"]["train"] == dict(**c100, **aug) and T["CIFAR100"]["test"] == dict(**c100, **plain)
    imgs, labels = torch.zeros(20, 32, 32, 3, dtype=torch.uint8), torch.zeros(20, dtype=torch.int64)
    tr, te = K.device_batches("CIFAR100", True, imgs, labels, 8), K.device_batches("CIFAR100", False, imgs, labels, 8, drop_last=True)
    assert (tr.shuffle, tr.flip, tr.padding, tr.out_hw, tr.mean, tr.channels_last) == (True, True, 4, (32, 32), c100["mean"], True)
    assert (te.shuffle, te.flip, te.padding, te.out_hw, te.std, len(te)) == (False, False, 0, (32, 32), c100["std"], 2)
    sv = K.device_batches("SVHN", True, torch.zeros(5, 3, 32, 32, dtype=torch.uint8), None, 2)
    assert (sv.shuffle, sv.channels_last, sv.out_hw) == (True, False, (32, 32))
    assert K.device_batches("MNIST", False, torch.zeros(5, 28, 28, dtype=torch.uint8), None, 2).out_hw == (28, 28)
    assert CHANNELS_LAST == {"MNIST": True, "SVHN": False, "CIFAR10": True, "CIFAR100": True}         # how torchvision's dataset objects hold .data
    with pytest.raises(ValueError, match="unknown dataset"):
        K.device_batches("ImageNet", True, imgs, labels, 8)


@pytest.mark.parametrize("name", ["c3_32x32", "c1_28x28", "c3_5x7", "c3_32x32_to_24x20"])
def test_restatement_places_pixels_as_pil_does(name):
    """Guards the reference, not the feature: ``ImageOps.expand(border=p, fill=0)``, ``.crop`` and ``.transpose(FLIP_LEFT_RIGHT)`` are the calls
    torchvision's pad / crop / hflip make on PIL inputs."""
    pytest.importorskip("PIL")
    from PIL import Image, ImageOps
    (Cn, H, W), (Ho, Wo), p = FC.SHAPES[name]
    images = FC.make_images(Cn, H, W, channels_last=True)
    table = FC.corner_table(H, W, Ho, Wo, p)
    for layout_cl in (True, False):
        src = images if layout_cl else np.ascontiguousarray(images.transpose(0, 3, 1, 2))
        u8, pad = FC.gather_u8(src, table, (Ho, Wo), layout_cl)
        for b, (index, top, left, flip) in enumerate(table.tolist()):
            img = Image.fromarray(images[index] if Cn == 3 else images[index][:, :, 0])
            img = ImageOps.expand(img, border=p, fill=0).crop((left + p, top + p, left + p + Wo, top + p + Ho))
            if flip:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
            got = np.asarray(img).reshape(Ho, Wo, Cn).transpose(2, 0, 1)
            assert np.array_equal(got, u8[b]), (name, b)
    assert pad.any() and not pad.all()


def test_restatement_arithmetic():
    """The fp32 restatement is ToTensor's and Normalize's three fp32 operations, one rounding each (numpy, operation by operation), and the
    padding value is (0 - mean) / std."""
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16).repeat(3, axis=1)
    r32 = FC.to_tensor_normalize(u8, FC.CIFAR10_MEAN, FC.CIFAR10_STD, torch.float32).numpy()
    m = np.asarray(FC.CIFAR10_MEAN, dtype=np.float32).reshape(1, 3, 1, 1)
    s = np.asarray(FC.CIFAR10_STD, dtype=np.float32).reshape(1, 3, 1, 1)
    assert np.array_equal(r32, (u8.astype(np.float32) / np.float32(255) - m) / s)
    assert np.array_equal(r32[0, :, 0, 0], FC.padding_values(FC.CIFAR10_MEAN, FC.CIFAR10_STD))
    r64 = FC.to_tensor_normalize(u8, FC.CIFAR10_MEAN, FC.CIFAR10_STD, torch.float64).numpy()
    assert r64.dtype == np.float64 and 0 < np.abs(r32 - r64).max() / np.abs(r64).max() < 1e-6
