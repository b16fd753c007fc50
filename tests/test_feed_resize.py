"""The loader's ImageNet branch on device-resident datasets, off the device: the restatement the GPU tests compare against (resize_cases.py)
gives PIL's bytes (against PIL itself where it is installed, against the stored fixture everywhere); ``data.resample_coeffs`` gives the
restatement's coefficients; the C ABI of csrc/kan_feed_resize.hip is declared, bound and refuses bad arguments by host arithmetic;
``ops.prepare_resized_batch`` refuses what it cannot take; ``ResizedDeviceBatches.epoch_table`` (torch ops on the device of the images, so it
runs on CPU tensors) draws what ``RandomResizedCrop`` / ``CenterCrop`` draw -- in distribution, not in stream; ``IMAGENET_TRANSFORMS`` holds
the values of utils/dataloader.py:9-54."""
import ctypes as C
import importlib.util
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import convkan_amd as K
from convkan_amd import _lib as L
from convkan_amd import data as D
import resize_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("kan_feed_resize_batch", "kan_feed_resize_max_ksize")


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_equals_the_stored_pil_bytes():
    """tests/golden/feed_resize/feed_resize_pil.npz carries PIL's bytes to where PIL may be missing."""
    assert os.path.getsize(RC.GOLDEN) < 100 * 1024
    golden = np.load(RC.GOLDEN)
    assert set(golden.files) == set(RC.CELLS) | {f"len_{n}" for n in RC.PIL_LENGTHS}
    for name in RC.CELLS:
        assert np.array_equal(RC.cell(name)["u8"], golden[name]), name
    for n in RC.PIL_LENGTHS:
        assert np.array_equal(RC.resample_last_axis(RC.length_image(n), 224), golden[f"len_{n}"]), n


def _golden_maker():
    spec = importlib.util.spec_from_file_location("make_golden_resize", os.path.join(ROOT, "tests", "golden", "make_golden_resize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stored_bytes_are_what_pil_gives():
    pytest.importorskip("PIL")
    golden, made = np.load(RC.GOLDEN), _golden_maker().build()
    assert set(golden.files) == set(made)
    for name in made:
        assert np.array_equal(golden[name], made[name]), name


@pytest.mark.parametrize("case", range(len(RC.PIL_CASES)))
def test_restatement_equals_pil(case):
    """``Image.resize(size, BILINEAR)`` and ``Image.crop``: the calls torchvision's Resize, RandomResizedCrop and CenterCrop make on PIL inputs."""
    pytest.importorskip("PIL")
    from PIL import Image
    mode, hw, size, box, out_hw = RC.PIL_CASES[case]
    a = RC.pil_case_image(mode, hw, case)
    img = Image.fromarray(a.transpose(1, 2, 0) if mode == "RGB" else a[0])
    Rh, Rw = size if size else hw
    top, left, h, w = box if box else (0, 0, Rh, Rw)
    if size:
        img = img.resize((Rw, Rh), Image.BILINEAR)
    if box:
        img = img.crop((left, top, left + w, top + h))
    img = img.resize((out_hw[1], out_hw[0]), Image.BILINEAR)
    got = np.asarray(img).reshape(out_hw + (a.shape[0],)).transpose(2, 0, 1)
    want = RC.pipeline_u8(a[None], [(0, top, left, h, w, 0)], size, out_hw, channels_last=False)[0]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", RC.PIL_LENGTHS)
def test_restatement_equals_pil_on_edge_lengths(n):
    """n -> 224 on both axes at once, a random n x n RGB image."""
    pytest.importorskip("PIL")
    from PIL import Image
    a = RC.pil_case_image("RGB", (n, n), 100 + n)
    got = np.asarray(Image.fromarray(a.transpose(1, 2, 0)).resize((224, 224), Image.BILINEAR)).transpose(2, 0, 1)
    assert np.array_equal(got, RC.resize(a, 224, 224))


# ------------------------------------------------------------------------------------------------------------------ the coefficients
@pytest.mark.parametrize("n,m", [(n, 224) for n in range(1, 257)] + [(32, 256), (28, 224), (13, 7), (7, 5), (224, 6)])
def test_resample_coeffs_equal_the_restatement(n, m):
    bounds, k = D.resample_coeffs(n, m)
    xmins, counts, ks = RC.coeffs(n, m)
    assert bounds.dtype == np.int32 and k.dtype == np.int32 and bounds.shape == (m, 2) and k.shape == (m, len(ks[0]))
    assert bounds[:, 0].tolist() == xmins and bounds[:, 1].tolist() == counts and k.tolist() == ks
    if n == m:                                                            # the identity: one tap of 2^22
        assert bounds.tolist() == [[x, min(2, n - x)] for x in range(m)] and k[:, 0].tolist() == [1 << 22] * m and not k[:, 1:].any()


def test_resize_tables_pack_the_passes():
    H, W, Rh, Rw, Ho, Wo = 5, 7, 13, 9, 6, 4
    t = D.resize_tables(H, W, Rh, Rw, Ho, Wo)
    assert isinstance(t, K.ResizeTables) and t.geometry == (H, W, Rh, Rw, Ho, Wo) and t.device.type == "cpu"
    assert all(x.dtype == torch.int32 and x.dim() == 1 and x.is_contiguous() for x in t.tables)
    k1x, k1y, k2x, k2y = (x.numpy().reshape(-1, ks + 2) for x, ks in zip(t.tables, t.ksize))
    assert t.ksize == (3, 3, 2 * math.ceil(Rw / Wo) + 1, 2 * math.ceil(Rh / Ho) + 1)
    assert k1x.shape[0] == Rw and k1y.shape[0] == Rh and k2x.shape[0] == Rw * Wo and k2y.shape[0] == Rh * Ho
    for rows, n, m in ((k1x, W, Rw), (k1y, H, Rh)) + tuple((k2x[(w - 1) * Wo:w * Wo], w, Wo) for w in range(1, Rw + 1)) \
            + tuple((k2y[(h - 1) * Ho:h * Ho], h, Ho) for h in range(1, Rh + 1)):
        xmins, counts, ks = RC.coeffs(n, m)
        assert rows[:, 0].tolist() == xmins and rows[:, 1].tolist() == counts
        assert rows[:, 2:2 + len(ks[0])].tolist() == ks and not rows[:, 2 + len(ks[0]):].any()
    assert D.resized_hw(32, 32, 256) == (256, 256) and D.resized_hw(7, 5, 10) == (14, 10) and D.resized_hw(5, 7, 10) == (10, 14)
    assert D.resized_hw(30, 45, 7) == (7, int(7 * 45 / 30)) and D.resized_hw(3, 4, (9, 8)) == (9, 8) and D.resized_hw(3, 4, None) == (3, 4)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
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
    assert lib.kan_feed_resize_max_ksize() >= 5                           # 256 -> 224 needs 5, downscaling by up to 2 needs 5 too
    for name in ("ResizedDeviceBatches", "imagenet_device_batches", "IMAGENET_TRANSFORMS", "resample_coeffs", "resize_tables", "ResizeTables"):
        assert hasattr(K, name), name
    assert list(inspect.signature(K.ops.prepare_resized_batch).parameters) == [
        "images", "table", "resize", "out_hw", "mean", "std", "labels", "channels_last", "out_channels", "coeffs", "out"]
    assert list(inspect.signature(K.ResizedDeviceBatches.__init__).parameters)[1:] == [
        "images", "labels", "batch_size", "mean", "std", "resize", "crop", "random_resized_crop", "flip", "out_channels", "shuffle",
        "channels_last", "drop_last", "seed", "rank", "world_size", "device"]


def test_launcher_refuses_bad_arguments_without_a_device():
    K.build_library()
    lib = L.load()
    p, null, st = C.c_void_p(64), C.c_void_p(0), C.c_void_p(0)           # never dereferenced: every call below is refused before a launch
    host = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    kmax = lib.kan_feed_resize_max_ksize()

    def refused(rc, word):
        assert rc < 0
        msg = lib.kan_last_error().decode()
        assert word in msg, msg

    def args(**kw):
        a = dict(images=p, labels=p, table=p, N=10, B=4, C=3, H=8, W=8, Rh=20, Rw=20, Ho=12, Wo=12, cl=1, oc=3, k1x=p, ks1x=3, k1y=p, ks1y=3,
                 k2x=p, ks2x=5, k2y=p, ks2y=5, mean=host, std=host, data=p, target=p, stream=st)
        a.update(kw)
        return list(a.values())
    for name in ("images", "table", "k1x", "k1y", "k2x", "k2y", "mean", "std", "data"):
        refused(lib.kan_feed_resize_batch(*args(**{name: null})), "kan_feed_resize_batch: null pointer")
    refused(lib.kan_feed_resize_batch(*args(labels=null)), "labels and target")          # one of the pair alone
    refused(lib.kan_feed_resize_batch(*args(target=null)), "labels and target")
    for name in ("N", "B", "C", "H", "W", "Rh", "Rw", "Ho", "Wo", "ks1x", "ks1y", "ks2x", "ks2y"):
        refused(lib.kan_feed_resize_batch(*args(**{name: 0})), "must be at least 1")
    refused(lib.kan_feed_resize_batch(*args(C=5, oc=5)), "at most 4 channels")
    for Cn, oc in ((3, 1), (3, 4), (1, 2), (1, 4), (2, 3), (3, 0)):
        refused(lib.kan_feed_resize_batch(*args(C=Cn, oc=oc)), "out_channels")
    limit = lib.kan_feed_max_image_bytes()
    refused(lib.kan_feed_resize_batch(*args(C=1, oc=1, H=1, W=limit + 1)), "at most 65536 bytes")
    refused(lib.kan_feed_resize_batch(*args(C=4, oc=4, H=129, W=128)), "at most 65536 bytes")
    for name in ("ks1x", "ks1y", "ks2x", "ks2y"):
        refused(lib.kan_feed_resize_batch(*args(**{name: kmax + 1})), "ksize above")
    for name in ("Rh", "Rw", "Ho", "Wo"):
        refused(lib.kan_feed_resize_batch(*args(**{name: 4097})), "at most 4096")
    refused(lib.kan_feed_resize_batch(*args(Rh=4096, Rw=4096, Ho=1024, Wo=1024, ks2x=9, ks2y=9)), "LDS")


def test_prepare_resized_batch_refuses_what_it_cannot_take():
    K.build_library()
    images = torch.zeros(6, 8, 8, 3, dtype=torch.uint8)
    table = torch.zeros(2, 6, dtype=torch.int32)
    mean, std = (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        K.ops.prepare_resized_batch(images, table, 20, (12, 12), mean, std)
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        K.ops.prepare_resized_batch(images, table, (20, 20), (12, 12), mean, std, labels=torch.zeros(6, dtype=torch.int64),
                                    coeffs=D.resize_tables(8, 8, 20, 20, 12, 12))
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        K.ops.prepare_resized_batch(torch.zeros(6, 8, 8, dtype=torch.uint8), table, None, (12, 12), mean, std, out_channels=3)
    for bad, word in (
            (dict(images=images.float()), "uint8"),
            (dict(images=torch.zeros(6, 8, 3, 8, dtype=torch.uint8).transpose(2, 3)), "contiguous"),
            (dict(table=table.long()), "int32"),
            (dict(table=torch.zeros(2, 12, dtype=torch.int32)[:, ::2]), "contiguous"),
            (dict(table=torch.zeros(2, 4, dtype=torch.int32)), r"\[B, 6\]"),
            (dict(images=torch.zeros(6, 8, 8, 5, dtype=torch.uint8), mean=(0.5,) * 5, std=(0.5,) * 5), "at most 4 channels"),
            (dict(images=torch.zeros(2, 5, 8, 8, dtype=torch.uint8), channels_last=False, mean=(0.5,) * 5, std=(0.5,) * 5), "at most 4 channels"),
            (dict(images=torch.zeros(2, 128, 129, 4, dtype=torch.uint8), mean=(0.5,) * 4, std=(0.5,) * 4), "bytes"),
            (dict(resize=(0, 20)), "resize"),
            (dict(out_hw=(0, 8)), "out_hw"),
            (dict(out_channels=1), "out_channels"),
            (dict(images=torch.zeros(6, 8, 8, 2, dtype=torch.uint8), out_channels=3), "out_channels"),
            (dict(mean=(0.5,)), "mean and std"),
            (dict(images=torch.zeros(6, 8, 8, dtype=torch.uint8), out_channels=3, mean=(0.5,), std=(0.5,)), "mean and std"),
            (dict(labels=torch.zeros(6, dtype=torch.int32)), "labels"),
            (dict(labels=torch.zeros(5, dtype=torch.int64)), "labels"),
            (dict(coeffs=D.resize_tables(8, 8, 20, 20, 12, 8)), "coeffs"),
            (dict(coeffs="tables"), "coeffs"),
            (dict(resize=8, out_hw=(1, 1), coeffs=D.resize_tables(8, 8, 8, 8, 1, 1)), "taps")):
        kw = dict(images=images, table=table, resize=20, out_hw=(12, 12), mean=mean, std=std)
        kw.update(bad)
        with pytest.raises(L.KanConvError, match=word):
            K.ops.prepare_resized_batch(**kw)


# ------------------------------------------------------------------------------------------------------------------ the tables of an epoch
def _cifar_train(N=4000, seed=0, **kw):
    return K.imagenet_device_batches("CIFAR10", True, torch.zeros(N, 32, 32, 3, dtype=torch.uint8), torch.arange(N), 8, seed=seed, **kw)


def test_epoch_table_draws_random_resized_crops():
    N, R = 4000, 256
    d = _cifar_train(N)
    assert (d.resize, d.out_hw, d.flip, d.shuffle, d.out_channels) == ((R, R), (224, 224), True, True, 3)
    t0, t1 = d.epoch_table(0), d.epoch_table(1)
    assert t0.dtype == torch.int32 and tuple(t0.shape) == (N, 6) and t0.device.type == "cpu" and t0.is_contiguous()
    assert sorted(t0[:, 0].tolist()) == list(range(N)) and t0[:, 0].tolist() != list(range(N))
    assert torch.equal(d.epoch_table(0), t0) and torch.equal(_cifar_train(N).epoch_table(0), t0)      # a pure function of (seed, epoch)
    assert not torch.equal(t0, t1) and not torch.equal(_cifar_train(N, seed=1).epoch_table(0), t0)
    top, left, h, w, flip = (t0[:, i].long() for i in range(1, 6))
    assert bool(((h >= 1) & (w >= 1) & (top >= 0) & (left >= 0) & (top + h <= R) & (left + w <= R)).all())        # inside the stage-1 image
    assert sorted(set(flip.tolist())) == [0, 1]
    # w = round(sqrt(a r)), h = round(sqrt(a / r)) with a / R^2 in [0.08, 1] and r in [3/4, 4/3]: each edge is off by at most 1/2
    hd, wd = h.double(), w.double()
    assert bool(((hd + 0.5) * (wd + 0.5) >= 0.08 * R * R).all()) and bool(((hd - 0.5) * (wd - 0.5) <= 1.0 * R * R).all())
    assert bool(((wd + 0.5) / (hd - 0.5) >= 3 / 4).all()) and bool(((wd - 0.5) / (hd + 0.5) <= 4 / 3).all())
    frac = (hd * wd / (R * R))
    assert 0.3 < float(frac.mean()) < 0.7 and float(frac.min()) < 0.12 and float(frac.max()) > 0.9      # U(0.08, 1), thinned where a box does not fit
    assert bool((w > h).any()) and bool((w < h).any())
    assert int(top.max()) > 100 and int(left.max()) > 100 and int(top.min()) == 0 and int(left.min()) == 0


def test_epoch_table_fallback_and_centre_crop():
    imgs = torch.zeros(50, 32, 32, 3, dtype=torch.uint8)
    # an area four times the image never fits: the fallback is the whole image for a square source
    d = K.ResizedDeviceBatches(imgs, None, 8, (0.5,) * 3, (0.5,) * 3, resize=256, crop=224, random_resized_crop=((4, 4), (3 / 4, 4 / 3)))
    assert torch.equal(d.epoch_table(0), torch.tensor([[i, 0, 0, 256, 256, 0] for i in range(50)], dtype=torch.int32))
    # a ratio range the stage-1 image lies outside of: the centred box of full extent clamped to it
    wide = K.ResizedDeviceBatches(torch.zeros(5, 10, 40, dtype=torch.uint8), None, 8, (0.5,), (0.5,), resize=None, crop=8,
                                  random_resized_crop=((4, 4), (3 / 4, 4 / 3))).epoch_table(0)
    assert wide.tolist() == [[i, 0, (40 - 13) // 2, 10, 13, 0] for i in range(5)]                      # w = round(10 * 4 / 3)
    test = K.imagenet_device_batches("CIFAR10", False, imgs, None, 8)
    assert torch.equal(test.epoch_table(0), torch.tensor([[i, 16, 16, 224, 224, 0] for i in range(50)], dtype=torch.int32))
    assert torch.equal(test.epoch_table(0), test.epoch_table(5))
    mnist = K.imagenet_device_batches("MNIST", True, torch.zeros(5, 28, 28, dtype=torch.uint8), None, 2)
    assert (mnist.resize, mnist.out_hw, mnist.out_channels, mnist.shuffle) == ((224, 224), (224, 224), 3, True)
    assert sorted(mnist.epoch_table(0).tolist()) == [[i, 0, 0, 224, 224, 0] for i in range(5)]
    odd = K.ResizedDeviceBatches(torch.zeros(3, 7, 5, dtype=torch.uint8), None, 2, (0.5,), (0.5,), resize=10, crop=(9, 6))
    assert odd.resize == (14, 10) and odd.epoch_table(0).tolist() == [[i, int(round(2.5)), 2, 9, 6, 0] for i in range(3)]   # round half to even
    with pytest.raises(ValueError, match="does not fit"):
        K.ResizedDeviceBatches(imgs, None, 8, (0.5,) * 3, (0.5,) * 3, resize=20, crop=24)
    assert d.coeffs.geometry == (32, 32, 256, 256, 224, 224) and d.coeffs.ksize == (3, 3, 5, 5)


def test_epoch_table_shards_like_a_distributed_sampler():
    N, ws = 37, 3
    shards = [_cifar_train(N, rank=r, world_size=ws).epoch_table(2) for r in range(ws)]
    whole = _cifar_train(N).epoch_table(2)
    assert all(tuple(s.shape) == (13, 6) for s in shards)
    padded = torch.cat((whole, whole[:2]))                                                           # 39 rows: the tail wraps around
    for r in range(ws):
        assert torch.equal(shards[r], padded[r::ws])
    assert len(_cifar_train(N, rank=1, world_size=ws)) == 2                                           # ceil(13 / 8)
    assert len(_cifar_train(N, drop_last=True)) == 4 and len(_cifar_train(N)) == 5
    with pytest.raises(ValueError):
        _cifar_train(N, rank=3, world_size=3)


def test_imagenet_transforms_hold_the_reference_values():
    """utils/dataloader.py:9-54."""
    T = K.IMAGENET_TRANSFORMS
    assert set(T) == {"MNIST", "SVHN", "CIFAR10", "CIFAR100"} and all(set(v) == {"train", "test"} for v in T.values())
    norm = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    assert T["MNIST"]["train"] == T["MNIST"]["test"] == dict(**norm, resize=224, crop=None, random_resized_crop=None, flip=False, out_channels=3)
    for name in ("SVHN", "CIFAR10", "CIFAR100"):
        assert T[name]["train"] == dict(**norm, resize=256, crop=224, random_resized_crop=((0.08, 1.0), (3 / 4, 4 / 3)), flip=True, out_channels=3)
        assert T[name]["test"] == dict(**norm, resize=256, crop=224, random_resized_crop=None, flip=False, out_channels=3)
    sv = K.imagenet_device_batches("SVHN", True, torch.zeros(5, 3, 32, 32, dtype=torch.uint8), None, 2)
    assert (sv.shuffle, sv.channels_last, sv.resize, sv.out_hw, sv.mean) == (True, False, (256, 256), (224, 224), norm["mean"])
    with pytest.raises(ValueError, match="unknown dataset"):
        K.imagenet_device_batches("ImageNet", True, torch.zeros(5, 3, 32, 32, dtype=torch.uint8), None, 2)
