"""The batch-preparation kernel of csrc/kan_feed.hip (ops.prepare_batch), K.DeviceBatches and the loop on them, on the device.

The reference of every case is the test-side restatement of torchvision's pipeline in feed_cases.py (pad the uint8 image with zeros, slice,
reverse W, ``/ 255``, ``(x - mean) / std``; torch CPU ops in that order, once in fp32 -- r32 -- and once in fp64 -- r64).  Placement is exact:
with mean 0 and std 1, round(data * 255) is the gathered byte.  Values follow the project's calibrated rule with no flat term,
    max|y - r64| / max|r64|  <=  4 x max|r32 - r64| / max|r64|,
and a padded pixel equals (0 - mean[c]) / std[c] bit for bit.  Every case prints what it measured, including whether the output was
bit-identical to r32 (an observation, not an assertion)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import feed_cases as FC

pytestmark = pytest.mark.gpu

PAD, SENT = 64, 0x7FA5A5A5           # sentinel words on each side of a guarded output (a NaN pattern no kernel writes)


def _norm(Cn):
    return (FC.MNIST_MEAN, FC.MNIST_STD) if Cn == 1 else (FC.CIFAR10_MEAN[:Cn], FC.CIFAR10_STD[:Cn])


@functools.lru_cache(maxsize=None)
def _cell(name, channels_last):
    """The dataset, the table and the restatement of one (shape, layout), computed once and shared by the cases that need them."""
    (Cn, H, W), out_hw, p = FC.SHAPES[name]
    images = FC.make_images(Cn, H, W, channels_last)
    table = FC.corner_table(H, W, *out_hw, p)
    mean, std = _norm(Cn)
    u8, pad, r32, r64 = FC.restate(images, table, out_hw, mean, std, channels_last)
    return dict(images=images, table=table, out_hw=out_hw, mean=mean, std=std, u8=u8, pad=pad, r32=r32, r64=r64, C=Cn)


def _check_values(tag, y, u8, pad, r32, r64, mean, std):
    """The value rule on one batch; y, r32, r64 on the CPU."""
    scale = float(r64.abs().max())
    err, ref_err = float((y.double() - r64).abs().max()) / scale, float((r32.double() - r64).abs().max()) / scale
    print(f"[feed {tag}] err {err:.3e} restatement fp32 err {ref_err:.3e} tol {4 * ref_err:.3e} bit-identical to r32: {torch.equal(y, r32)}")
    assert err <= 4 * ref_err
    pv = FC.padding_values(mean, std)
    for c in range(y.shape[1]):
        got = y[:, c][torch.from_numpy(pad[:, c])]
        assert bool((got == float(pv[c])).all()), (tag, c)


@pytest.mark.parametrize("B", [1, 8, 5])
@pytest.mark.parametrize("name", list(FC.SHAPES))
@pytest.mark.parametrize("channels_last", [True, False], ids=["channels_last", "chw"])
def test_cell(gpu_lib, channels_last, name, B):
    from convkan_amd import ops
    c = _cell(name, channels_last)
    images = torch.from_numpy(c["images"]).cuda()
    zeros, ones = (0.0,) * c["C"], (1.0,) * c["C"]
    for lo, hi in FC.chunks(len(c["table"]), B):
        table = torch.from_numpy(c["table"][lo:hi]).cuda()
        raw, none = ops.prepare_batch(images, table, c["out_hw"], zeros, ones, channels_last=channels_last)
        assert none is None and raw.dtype == torch.float32 and tuple(raw.shape) == (B, c["C"]) + tuple(c["out_hw"]) and raw.is_contiguous()
        placed = torch.round(raw * 255).cpu()
        assert torch.equal(placed, torch.from_numpy(c["u8"][lo:hi]).float()), (name, lo, hi)         # placement, padding included
        y, _ = ops.prepare_batch(images, table, c["out_hw"], c["mean"], c["std"], channels_last=channels_last)
        _check_values(f"{name} {'cl' if channels_last else 'chw'} rows {lo}:{hi}", y.cpu(), c["u8"][lo:hi], c["pad"][lo:hi], c["r32"][lo:hi],
                      c["r64"][lo:hi], c["mean"], c["std"])


# images above the 16 KiB a workgroup stages (blocks of output rows): a 16-byte stride, a stride that is none (and Wo % 4 != 0), and the largest image (one row
# of 65536 bytes: the staging needs more than the default 64 KiB of LDS)
@pytest.mark.parametrize("channels_last", [True, False], ids=["channels_last", "chw"])
@pytest.mark.parametrize("shape,out_hw,p", [((3, 80, 72), (80, 72), 4), ((1, 140, 127), (140, 127), 3), ((4, 1, 16384), (1, 16384), 2),
                                            ((2, 300, 100), (9, 12), 2)], ids=["17280B", "17780B", "65536B_one_row", "60000B_small_crop"])
def test_row_blocks(gpu_lib, channels_last, shape, out_hw, p):
    from convkan_amd import ops
    (Cn, H, W), n = shape, 3
    rng = np.random.default_rng(5)
    images = rng.integers(0, 256, size=(n, H, W, Cn) if channels_last else (n, Cn, H, W), dtype=np.uint8)
    table = np.array([(2, -p, -p, 1), (0, H - out_hw[0] + p, W - out_hw[1] + p, 0), (2, H - out_hw[0] + p, -p, 0), (1, -p, W - out_hw[1] + p, 1),
                      (1, (H - out_hw[0]) // 2, (W - out_hw[1]) // 2, 1)], dtype=np.int32)
    mean, std = _norm(Cn) if Cn <= 3 else (FC.CIFAR10_MEAN + (0.5,), FC.CIFAR10_STD + (0.25,))
    u8, pad, r32, r64 = FC.restate(images, table, out_hw, mean, std, channels_last)
    dev = torch.from_numpy(images).cuda()
    raw, _ = ops.prepare_batch(dev, torch.from_numpy(table).cuda(), out_hw, (0.0,) * Cn, (1.0,) * Cn, channels_last=channels_last)
    assert torch.equal(torch.round(raw * 255).cpu(), torch.from_numpy(u8).float())
    y, _ = ops.prepare_batch(dev, torch.from_numpy(table).cuda(), out_hw, mean, std, channels_last=channels_last)
    _check_values(f"row blocks {shape} {'cl' if channels_last else 'chw'}", y.cpu(), u8, pad, r32, r64, mean, std)


def test_labels(gpu_lib):
    from convkan_amd import ops
    c = _cell("c3_5x7", True)
    images, table = torch.from_numpy(c["images"]).cuda(), torch.from_numpy(c["table"]).cuda()
    labels = (torch.arange(FC.N_IMAGES, dtype=torch.int64) * 7919 - 100000).cuda()               # any int64, negative ones included
    data, target = ops.prepare_batch(images, table, c["out_hw"], c["mean"], c["std"], labels=labels)
    assert target.dtype == torch.int64 and torch.equal(target.cpu(), labels.cpu()[torch.from_numpy(c["table"][:, 0]).long()])
    alone, none = ops.prepare_batch(images, table, c["out_hw"], c["mean"], c["std"])
    assert none is None and torch.equal(alone, data)


def test_bad_index(gpu_lib):
    """Rows with index -1 and N among good rows: an all-zero image (0.0f, not the padding value), target -1, the neighbours untouched, and the
    loss kernels count two bad targets."""
    import convkan_amd as K
    from convkan_amd import ops
    for name, channels_last in (("c3_32x32", True), ("c3_5x7", False)):
        c = _cell(name, channels_last)
        images = torch.from_numpy(c["images"]).cuda()
        labels = torch.arange(FC.N_IMAGES, dtype=torch.int64).cuda() % 10
        good = torch.from_numpy(c["table"][:8]).cuda()
        bad = good.clone()
        bad[2, 0], bad[5, 0] = -1, FC.N_IMAGES
        clean, clean_t = ops.prepare_batch(images, good, c["out_hw"], c["mean"], c["std"], labels=labels, channels_last=channels_last)
        data, target = ops.prepare_batch(images, bad, c["out_hw"], c["mean"], c["std"], labels=labels, channels_last=channels_last)
        keep = [0, 1, 3, 4, 6, 7]
        assert torch.equal(data[keep], clean[keep]) and torch.equal(target[keep], clean_t[keep])
        assert bool((data[[2, 5]] == 0).all()) and target[[2, 5]].tolist() == [-1, -1] and bool((clean[[2, 5]] != 0).any())
        metrics = K.ClassMetrics(10, "cuda")
        ops.cross_entropy(torch.randn(8, 10, device="cuda"), target, metrics)
        assert metrics.buffer[:4].tolist()[1:] == [6, 1, 2]                                       # samples, batches, bad_target
        with pytest.raises(K._lib.KanConvError, match="2 target"):
            metrics.result()
    # the extremes of int32 in every column address nothing either
    wild = torch.tensor([[2 ** 31 - 1, 0, 0, 0], [-2 ** 31, 0, 0, 0], [1, 2 ** 31 - 1, -2 ** 31, 5], [1, -2 ** 31, 2 ** 31 - 1, -1]], dtype=torch.int32)
    data, target = ops.prepare_batch(images, wild.cuda(), c["out_hw"], c["mean"], c["std"], labels=labels, channels_last=channels_last)
    pv = torch.tensor(FC.padding_values(c["mean"], c["std"])).view(1, -1, 1, 1)
    assert target.tolist() == [-1, -1, 1, 1] and bool((data[:2] == 0).all()) and torch.equal(data[2:].cpu(), pv.expand(2, -1, *c["out_hw"]))


def _guarded(n, dtype=torch.float32, shift=0):
    """(buffer, view): n elements of `dtype` (4 or 8 bytes) placed PAD + shift words into a larger int32 buffer filled with a sentinel."""
    words = n * (2 if dtype == torch.int64 else 1)
    buf = torch.full((words + 2 * PAD + shift,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf[PAD + shift:PAD + shift + words].view(dtype)


def _borders_intact(buf, words, shift=0):
    return bool((buf[:PAD + shift] == SENT).all()) and bool((buf[PAD + shift + words:] == SENT).all())


@pytest.mark.parametrize("name,B,shift,image_shift", [("c3_5x7", 8, 0, 0), ("c3_32x32", 5, 0, 0), ("c3_32x32", 5, 1, 0), ("c3_32x32", 5, 0, 1),
                                                        ("c1_28x28", 5, 3, 5)],
                         ids=["105B_images", "B5", "B5_data_off_16B", "B5_images_off_16B", "both_off_16B"])
def test_guarded_outputs_and_determinism(gpu_lib, name, B, shift, image_shift):
    """Through the C ABI, data and target inside sentinel-filled buffers: no word outside them changes, two launches give the same bits, and a
    data or image pointer that is not 16-byte aligned (the scalar-store and byte-load kernels) gives the same values."""
    from convkan_amd import _lib as L
    c = _cell(name, True)
    Cn, (Ho, Wo) = c["C"], c["out_hw"]
    H, W = FC.SHAPES[name][0][1:]
    flat = torch.from_numpy(c["images"]).reshape(-1)
    store = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device="cuda")
    store[image_shift:image_shift + flat.numel()] = flat.cuda()
    labels = torch.arange(FC.N_IMAGES, dtype=torch.int64, device="cuda")
    table = torch.from_numpy(c["table"][:B]).cuda()
    mean, std = (C.c_float * Cn)(*c["mean"]), (C.c_float * Cn)(*c["std"])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        dbuf, data = _guarded(B * Cn * Ho * Wo, shift=shift)
        tbuf, target = _guarded(B, torch.int64)
        L.check(gpu_lib.kan_feed_batch(C.c_void_p(store.data_ptr() + image_shift), C.c_void_p(labels.data_ptr()), C.c_void_p(table.data_ptr()),
                                       FC.N_IMAGES, B, Cn, H, W, Ho, Wo, 1, mean, std, C.c_void_p(data.data_ptr()), C.c_void_p(target.data_ptr()),
                                       st), "kan_feed_batch")
        torch.cuda.synchronize()
        assert _borders_intact(dbuf, B * Cn * Ho * Wo, shift) and _borders_intact(tbuf, 2 * B)
        assert not bool((dbuf[PAD + shift:PAD + shift + B * Cn * Ho * Wo] == SENT).any())            # every output word written
        runs.append((data.clone(), target.clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1], runs[1][1])
    y = runs[0][0].view(B, Cn, Ho, Wo).cpu()
    _check_values(f"guarded {name} B {B} shifts {shift}/{image_shift}", y, c["u8"][:B], c["pad"][:B], c["r32"][:B], c["r64"][:B], c["mean"], c["std"])
    assert torch.equal(runs[0][1].cpu(), torch.from_numpy(c["table"][:B, 0]).long())


def test_out_argument(gpu_lib):
    from convkan_amd import ops
    from convkan_amd._lib import KanConvError
    c = _cell("c3_32x32", True)
    images, table = torch.from_numpy(c["images"]).cuda(), torch.from_numpy(c["table"][:8]).cuda()
    labels = torch.arange(FC.N_IMAGES, dtype=torch.int64, device="cuda")
    want, want_t = ops.prepare_batch(images, table, (32, 32), c["mean"], c["std"], labels=labels)
    data, target = torch.full((8, 3, 32, 32), float("nan"), device="cuda"), torch.full((8,), -7, dtype=torch.int64, device="cuda")
    got, got_t = ops.prepare_batch(images, table, (32, 32), c["mean"], c["std"], labels=labels, out=(data, target))
    assert got is data and got_t is target and torch.equal(data, want) and torch.equal(target, want_t)
    alone, none = ops.prepare_batch(images, table, (32, 32), c["mean"], c["std"], out=(data.zero_(), None))
    assert alone is data and none is None and torch.equal(data, want)
    for bad in ((torch.empty(7, 3, 32, 32, device="cuda"), target), (torch.empty(8, 3, 32, 31, device="cuda"), target),
                (data, torch.empty(9, dtype=torch.int64, device="cuda")), (data.double(), target), (data, target.int()), (data, None),
                (torch.empty(8, 3, 32, 64, device="cuda")[..., ::2], target), (data.cpu(), target)):
        with pytest.raises(KanConvError):
            ops.prepare_batch(images, table, (32, 32), c["mean"], c["std"], labels=labels, out=bad)


def test_device_batches(gpu_lib):
    import convkan_amd as K
    from convkan_amd import ops
    c = _cell("c3_32x32", True)
    N = FC.N_IMAGES
    images, labels = torch.from_numpy(c["images"]), torch.arange(N, dtype=torch.int64)

    def make(seed=0):
        return K.DeviceBatches(images, labels, 8, c["mean"], c["std"], crop=32, padding=4, flip=True, shuffle=True, seed=seed, device="cuda")
    d = make()
    assert len(d) == 5 and d.images.is_cuda and d.labels.is_cuda
    first = list(d)
    assert [x.shape[0] for x, _ in first] == [8, 8, 8, 8, 5] and all(x.is_cuda and t.is_cuda for x, t in first)
    table = d.table.clone()
    targets = torch.cat([t for _, t in first])
    assert sorted(targets.tolist()) == list(range(N)) and torch.equal(targets, table[:, 0].long())
    for i, (x, t) in enumerate(first):
        want, want_t = ops.prepare_batch(d.images, table[8 * i:8 * i + 8].contiguous(), (32, 32), c["mean"], c["std"], labels=d.labels)
        assert torch.equal(x, want) and torch.equal(t, want_t)
    # against the restatement too, through the table the epoch drew
    u8, pad, r32, r64 = FC.restate(c["images"], table.cpu().numpy(), (32, 32), c["mean"], c["std"], True)
    _check_values("DeviceBatches epoch 0", torch.cat([x for x, _ in first]).cpu(), u8, pad, r32, r64, c["mean"], c["std"])
    second = list(d)
    assert not torch.equal(d.table, table) and not torch.equal(torch.cat([t for _, t in second]), targets)
    again = make()
    repeat = list(again)
    assert torch.equal(again.table, table) and all(torch.equal(a, b) and torch.equal(s, t) for (a, s), (b, t) in zip(first, repeat))
    assert not torch.equal(make(seed=1).epoch_table(0), table)
    assert [x.shape[0] for x, _ in K.DeviceBatches(images, labels, 8, c["mean"], c["std"], drop_last=True, device="cuda")] == [8, 8, 8, 8]


def _tiny_model():
    import convkan_amd as K
    torch.manual_seed(0)
    return nn.Sequential(K.KANConv2DLayer(3, 8, 3, padding=1), nn.MaxPool2d(2), nn.Flatten(), nn.Linear(8 * 16 * 16, 10)).cuda()


def _loop_data(N=40):
    images = torch.from_numpy(FC.make_images(3, 32, 32, True, seed=3, n=N)).cuda()
    labels = (torch.arange(N, dtype=torch.int64) * 3 % 10).cuda()
    return images, labels


def test_evaluate_takes_device_batches(gpu_lib):
    import convkan_amd as K
    from convkan_amd import ops
    model = _tiny_model()
    images, labels = _loop_data()
    test = K.device_batches("CIFAR10", False, images, labels, 16)
    got = K.evaluate(model, test)
    listed = [ops.prepare_batch(images, test.table[16 * i:16 * i + 16].contiguous(), (32, 32), FC.CIFAR10_MEAN, FC.CIFAR10_STD, labels=labels)
              for i in range(3)]
    want = K.evaluate(model, listed)
    print("[feed evaluate]", got)
    assert got == want and (got["samples"], got["batches"]) == (40, 3) and math.isfinite(got["loss"])
    assert torch.equal(test.table, torch.tensor([[i, 0, 0, 0] for i in range(40)], dtype=torch.int32, device="cuda"))


def test_train_and_test_models_takes_device_batches(gpu_lib):
    import convkan_amd as K
    model = _tiny_model()
    images, labels = _loop_data()
    train = K.device_batches("CIFAR10", True, images, labels, 16)
    test = K.device_batches("CIFAR10", False, images, labels, 16)
    opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    out = K.train_and_test_models(model, train, test, opt, epochs=2)
    print("[feed loop]", out)
    assert len(out) == 7 and all(len(h) == 2 and all(math.isfinite(v) for v in h) for h in out)
    assert out[1][0] != out[1][1] and train.epoch == 2 and test.epoch == 2
