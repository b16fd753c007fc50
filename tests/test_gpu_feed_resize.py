"""The resized-feed kernel of csrc/kan_feed_resize.hip (ops.prepare_resized_batch), K.ResizedDeviceBatches and the loop on them, on the device.

The reference of every case is the test-side restatement of torchvision's ImageNet-branch pipeline on PIL images in resize_cases.py (PIL's
8-bit bilinear resampling as integer arithmetic, checked against PIL and against the stored PIL bytes by test_feed_resize.py), followed by
feed_cases.to_tensor_normalize (``/ 255``, ``(x - mean) / std``; torch CPU ops, once in fp32 -- r32 -- and once in fp64 -- r64).  Bytes are
exact: with mean 0 and std 1, round(data * 255) equals the restatement's bytes, and the stored PIL bytes for the small cells.  Values follow
the rule of test_gpu_feed.py with no flat term,
    max|y - r64| / max|r64|  <=  4 x max|r32 - r64| / max|r64|.
Every case prints what it measured, including whether the output was bit-identical to r32 (an observation, not an assertion)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import feed_cases as FC
import resize_cases as RC

pytestmark = pytest.mark.gpu

PAD, SENT = 64, 0x7FA5A5A5           # sentinel words on each side of a guarded output (a NaN pattern no kernel writes)


def _norm(oc):
    if oc == 1:
        return FC.MNIST_MEAN, FC.MNIST_STD
    return (RC.IMAGENET_MEAN + (0.5,))[:oc], (RC.IMAGENET_STD + (0.25,))[:oc]


def _check_values(tag, y, u8, mean, std):
    """The value rule on one batch; y on the CPU."""
    r32, r64 = FC.to_tensor_normalize(u8, mean, std, torch.float32), FC.to_tensor_normalize(u8, mean, std, torch.float64)
    scale = float(r64.abs().max())
    err, ref_err = float((y.double() - r64).abs().max()) / scale, float((r32.double() - r64).abs().max()) / scale
    print(f"[feed resize {tag}] err {err:.3e} restatement fp32 err {ref_err:.3e} tol {4 * ref_err:.3e} bit-identical to r32: {torch.equal(y, r32)}")
    assert err <= 4 * ref_err


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(RC.GOLDEN))


def _layout(images, channels_last):
    """The channels_last dataset of a cell in the layout under test."""
    return images if channels_last else np.ascontiguousarray(images.transpose(0, 3, 1, 2))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("name", list(RC.CELLS))
@pytest.mark.parametrize("channels_last", [True, False], ids=["channels_last", "chw"])
def test_cell(gpu_lib, channels_last, name, B):
    from convkan_amd import data as D
    from convkan_amd import ops
    c = RC.cell(name)
    images = torch.from_numpy(_layout(c["images"], channels_last)).cuda()
    oc = c["out_channels"] or c["C"]
    mean, std = _norm(oc)
    H, W = RC.CELLS[name][0][1:]
    coeffs = D.resize_tables(H, W, *c["resized"], *c["out_hw"], device="cuda")
    assert np.array_equal(c["u8"], _golden()[name])                                        # the restatement is PIL's bytes
    for lo, hi in RC.chunks(len(c["table"]), B):
        table = torch.from_numpy(c["table"][lo:hi]).cuda()
        raw, none = ops.prepare_resized_batch(images, table, c["size"], c["out_hw"], (0.0,) * oc, (1.0,) * oc, channels_last=channels_last,
                                              out_channels=c["out_channels"], coeffs=coeffs)
        assert none is None and raw.dtype == torch.float32 and tuple(raw.shape) == (B, oc) + tuple(c["out_hw"]) and raw.is_contiguous()
        placed = torch.round(raw * 255).cpu()
        assert torch.equal(placed, torch.from_numpy(c["u8"][lo:hi]).float()), (name, lo, hi)         # PIL's bytes, exactly
        y, _ = ops.prepare_resized_batch(images, table, c["size"], c["out_hw"], mean, std, channels_last=channels_last,
                                         out_channels=c["out_channels"])                              # builds its own coefficient tables
        _check_values(f"{name} {'cl' if channels_last else 'chw'} rows {lo}:{hi}", y.cpu(), c["u8"][lo:hi], mean, std)


@pytest.mark.parametrize("channels_last", [True, False], ids=["channels_last", "chw"])
def test_both_stages_identity_equals_prepare_batch(gpu_lib, channels_last):
    """No resize and the whole-image box: the bytes of the source, and the very bits ``prepare_batch`` gives."""
    from convkan_amd import ops
    c = RC.cell("c3_8x12_r_none_to_8x12")
    images = torch.from_numpy(_layout(c["images"], channels_last)).cuda()
    index = np.arange(RC.N_IMAGES, dtype=np.int32)
    flip = index % 2
    zero = np.zeros_like(index)
    whole = torch.from_numpy(np.stack((index, zero, zero, zero + 8, zero + 12, flip), axis=1)).cuda()
    plain = torch.from_numpy(np.stack((index, zero, zero, flip), axis=1)).cuda()
    mean, std = _norm(3)
    got, _ = ops.prepare_resized_batch(images, whole, None, (8, 12), mean, std, channels_last=channels_last)
    want, _ = ops.prepare_batch(images, plain, (8, 12), mean, std, channels_last=channels_last)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# the real sizes (blocks of output rows, the 256 -> 224 tables): CIFAR 3 x 32 x 32 -> 256 -> boxes -> 224, and MNIST 28 -> 224 to three channels
@pytest.mark.parametrize("name", ["cifar", "svhn_chw", "mnist"])
def test_real_sizes(gpu_lib, name):
    from convkan_amd import ops
    if name == "mnist":
        images = RC.make_images(1, 28, 28, True)[..., 0]
        table = np.array([(8, 0, 0, 224, 224, 0), (1, 0, 0, 224, 224, 1)], dtype=np.int32)
        size, oc, cl = 224, 3, True
    else:
        cl = name == "cifar"
        images = RC.make_images(3, 32, 32, cl)
        # an upscaled box and a downscaled one (ksize 5) that touches three edges
        table = np.array([(8, 13, 29, 97, 131, 1), (2, 6, 0, 250, 256, 0)], dtype=np.int32)
        size, oc, cl = 256, None, cl
    u8 = RC.pipeline_u8(images, table, size, (224, 224), cl, oc)
    dev, tab = torch.from_numpy(images).cuda(), torch.from_numpy(table).cuda()
    raw, _ = ops.prepare_resized_batch(dev, tab, size, (224, 224), (0.0,) * 3, (1.0,) * 3, channels_last=cl, out_channels=oc)
    assert torch.equal(torch.round(raw * 255).cpu(), torch.from_numpy(u8).float())
    y, _ = ops.prepare_resized_batch(dev, tab, size, (224, 224), RC.IMAGENET_MEAN, RC.IMAGENET_STD, channels_last=cl, out_channels=oc)
    _check_values(name, y.cpu(), u8, RC.IMAGENET_MEAN, RC.IMAGENET_STD)


def test_labels_and_bad_rows(gpu_lib):
    """Rows with a bad index or a bad box among good rows: an all-zero image, target -1, the neighbours untouched; the extremes of int32 in
    every column address nothing."""
    from convkan_amd import ops
    for name, channels_last in (("c3_8x8_r20_to_12x12", True), ("c1_7x5_r10_to_6x6_x3", False)):
        c = RC.cell(name)
        images = torch.from_numpy(_layout(c["images"], channels_last)).cuda()
        labels = (torch.arange(RC.N_IMAGES, dtype=torch.int64) * 7919 - 30000).cuda()            # any int64, negative ones included
        oc = c["out_channels"] or c["C"]
        mean, std = _norm(oc)
        Rh, Rw = c["resized"]
        kw = dict(labels=labels, channels_last=channels_last, out_channels=c["out_channels"])
        good = torch.from_numpy(c["table"][:10]).cuda()
        clean, clean_t = ops.prepare_resized_batch(images, good, c["size"], c["out_hw"], mean, std, **kw)
        assert torch.equal(clean_t.cpu(), labels.cpu()[torch.from_numpy(c["table"][:10, 0]).long()])
        alone, none = ops.prepare_resized_batch(images, good, c["size"], c["out_hw"], mean, std, channels_last=channels_last,
                                                out_channels=c["out_channels"])
        assert none is None and torch.equal(alone, clean)
        bad = good.clone()
        bad[1, 0], bad[3, 0] = -1, RC.N_IMAGES                                                    # index
        bad[5, 1:5] = torch.tensor([1, 0, Rh, Rw])                                                # top + h = Rh + 1
        bad[7, 1:5] = torch.tensor([0, Rw - 1, 1, 2])                                             # left + w = Rw + 1
        bad[8, 3] = 0                                                                             # h = 0
        rows = [1, 3, 5, 7, 8]
        keep = [0, 2, 4, 6, 9]
        data, target = ops.prepare_resized_batch(images, bad, c["size"], c["out_hw"], mean, std, **kw)
        assert torch.equal(data[keep], clean[keep]) and torch.equal(target[keep], clean_t[keep])
        assert bool((data[rows] == 0).all()) and target[rows].tolist() == [-1] * 5 and all(bool((clean[r] != 0).any()) for r in rows)
    big, small = 2 ** 31 - 1, -2 ** 31
    wild = torch.tensor([[big, 0, 0, 1, 1, 0], [small, 0, 0, 1, 1, 0], [1, big, 0, 1, 1, 0], [1, 0, small, 1, 1, 0], [1, 0, 0, big, 1, 0],
                         [1, 0, 0, 1, small, 0], [1, big, big, big, big, 1], [1, 1, 1, small, small, 1], [1, 0, 0, Rh, Rw, small]], dtype=torch.int32)
    data, target = ops.prepare_resized_batch(images, wild.cuda(), c["size"], c["out_hw"], mean, std, **kw)
    assert target.tolist() == [-1] * 8 + [int(labels[1])] and bool((data[:8] == 0).all()) and bool((data[8] != 0).any())


def _guarded(n, dtype=torch.float32, shift=0):
    """(buffer, view): n elements of `dtype` (4 or 8 bytes) placed PAD + shift words into a larger int32 buffer filled with a sentinel."""
    words = n * (2 if dtype == torch.int64 else 1)
    buf = torch.full((words + 2 * PAD + shift,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf[PAD + shift:PAD + shift + words].view(dtype)


def _borders_intact(buf, words, shift=0):
    return bool((buf[:PAD + shift] == SENT).all()) and bool((buf[PAD + shift + words:] == SENT).all())


@pytest.mark.parametrize("name,B,shift,image_shift", [("c3_8x8_r20_to_12x12", 5, 0, 0), ("c3_8x8_r20_to_12x12", 5, 1, 0),
                                                        ("c3_8x8_r20_to_12x12", 5, 0, 1), ("c1_7x5_r10_to_6x6_x3", 14, 3, 5),
                                                        ("c2_9x6_r13x10_to_5x7", 5, 0, 0)],
                         ids=["B5", "B5_data_off_16B", "B5_images_off_16B", "35B_images_both_off_16B", "54B_images"])
def test_guarded_outputs_and_determinism(gpu_lib, name, B, shift, image_shift):
    """Through the C ABI, data and target inside sentinel-filled buffers: no word outside them changes, every word inside is written, two
    launches give the same bits, and a data or image pointer that is not 16-byte aligned (the scalar-store and byte-load kernels) gives the
    same bytes."""
    from convkan_amd import _lib as L
    from convkan_amd import data as D
    c = RC.cell(name)
    Cn, (Ho, Wo), (Rh, Rw) = c["C"], c["out_hw"], c["resized"]
    oc = c["out_channels"] or Cn
    H, W = RC.CELLS[name][0][1:]
    flat = torch.from_numpy(c["images"]).reshape(-1)
    store = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device="cuda")
    store[image_shift:image_shift + flat.numel()] = flat.cuda()
    labels = torch.arange(RC.N_IMAGES, dtype=torch.int64, device="cuda")
    table = torch.from_numpy(c["table"][:B]).cuda()
    mean_v, std_v = _norm(oc)
    mean, std = (C.c_float * oc)(*mean_v), (C.c_float * oc)(*std_v)
    coeffs = D.resize_tables(H, W, Rh, Rw, Ho, Wo, device="cuda")
    ks = [v for t, k in zip(coeffs.tables, coeffs.ksize) for v in (C.c_void_p(t.data_ptr()), k)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        dbuf, data = _guarded(B * oc * Ho * Wo, shift=shift)
        tbuf, target = _guarded(B, torch.int64)
        L.check(gpu_lib.kan_feed_resize_batch(C.c_void_p(store.data_ptr() + image_shift), C.c_void_p(labels.data_ptr()),
                                              C.c_void_p(table.data_ptr()), RC.N_IMAGES, B, Cn, H, W, Rh, Rw, Ho, Wo, 1, oc, *ks, mean, std,
                                              C.c_void_p(data.data_ptr()), C.c_void_p(target.data_ptr()), st), "kan_feed_resize_batch")
        torch.cuda.synchronize()
        assert _borders_intact(dbuf, B * oc * Ho * Wo, shift) and _borders_intact(tbuf, 2 * B)
        assert not bool((dbuf[PAD + shift:PAD + shift + B * oc * Ho * Wo] == SENT).any())            # every output word written
        runs.append((data.clone(), target.clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1], runs[1][1])
    y = runs[0][0].view(B, oc, Ho, Wo).cpu()
    _check_values(f"guarded {name} B {B} shifts {shift}/{image_shift}", y, c["u8"][:B], mean_v, std_v)
    assert torch.equal(runs[0][1].cpu(), torch.from_numpy(c["table"][:B, 0]).long())


def test_out_argument(gpu_lib):
    from convkan_amd import ops
    from convkan_amd._lib import KanConvError
    c = RC.cell("c3_8x8_r20_to_12x12")
    images, table = torch.from_numpy(c["images"]).cuda(), torch.from_numpy(c["table"][:8]).cuda()
    labels = torch.arange(RC.N_IMAGES, dtype=torch.int64, device="cuda")
    mean, std = _norm(3)
    want, want_t = ops.prepare_resized_batch(images, table, 20, (12, 12), mean, std, labels=labels)
    data, target = torch.full((8, 3, 12, 12), float("nan"), device="cuda"), torch.full((8,), -7, dtype=torch.int64, device="cuda")
    got, got_t = ops.prepare_resized_batch(images, table, 20, (12, 12), mean, std, labels=labels, out=(data, target))
    assert got is data and got_t is target and torch.equal(data, want) and torch.equal(target, want_t)
    alone, none = ops.prepare_resized_batch(images, table, 20, (12, 12), mean, std, out=(data.zero_(), None))
    assert alone is data and none is None and torch.equal(data, want)
    for bad in ((torch.empty(7, 3, 12, 12, device="cuda"), target), (torch.empty(8, 3, 12, 11, device="cuda"), target),
                (data, torch.empty(9, dtype=torch.int64, device="cuda")), (data.double(), target), (data, target.int()), (data, None),
                (torch.empty(8, 3, 12, 24, device="cuda")[..., ::2], target), (data.cpu(), target)):
        with pytest.raises(KanConvError):
            ops.prepare_resized_batch(images, table, 20, (12, 12), mean, std, labels=labels, out=bad)


def _loop_data(N=40):
    images = torch.from_numpy(FC.make_images(3, 8, 8, True, seed=3, n=N)).cuda()
    labels = (torch.arange(N, dtype=torch.int64) * 3 % 10).cuda()
    return images, labels


def test_resized_device_batches(gpu_lib):
    """An epoch of random resized crops equals the restatement through the table the epoch drew; epochs differ; a seed repeats."""
    import convkan_amd as K
    from convkan_amd import ops
    images, labels = _loop_data(21)
    mean, std = _norm(3)

    def make(seed=0):
        return K.ResizedDeviceBatches(images, labels, 8, mean, std, resize=20, crop=12, random_resized_crop=True, flip=True, shuffle=True, seed=seed)
    d = make()
    assert len(d) == 3 and d.coeffs.device == images.device
    first = list(d)
    assert [x.shape[0] for x, _ in first] == [8, 8, 5] and all(x.is_cuda and t.is_cuda and tuple(x.shape[1:]) == (3, 12, 12) for x, t in first)
    table = d.table.clone()
    assert torch.equal(torch.cat([t for _, t in first]), labels[table[:, 0].long()])
    for i, (x, t) in enumerate(first):
        want, want_t = ops.prepare_resized_batch(images, table[8 * i:8 * i + 8].contiguous(), 20, (12, 12), mean, std, labels=labels)
        assert torch.equal(x, want) and torch.equal(t, want_t)
    u8 = RC.pipeline_u8(images.cpu().numpy(), table.cpu().numpy(), 20, (12, 12), True)
    _check_values("ResizedDeviceBatches epoch 0", torch.cat([x for x, _ in first]).cpu(), u8, mean, std)
    second = list(d)
    assert not torch.equal(d.table, table) and d.epoch == 2
    again = make()
    repeat = list(again)
    assert torch.equal(again.table, table) and all(torch.equal(a, b) and torch.equal(s, t) for (a, s), (b, t) in zip(first, repeat))
    assert not torch.equal(make(seed=1).epoch_table(0), table)


def test_evaluate_takes_resized_device_batches(gpu_lib):
    """One pass through ``evaluate`` on a tiny model; the iteration itself runs with torch's synchronisation check set to raise."""
    import convkan_amd as K
    from convkan_amd import ops
    torch.manual_seed(0)
    model = nn.Sequential(K.KANConv2DLayer(3, 8, 3, padding=1), nn.MaxPool2d(2), nn.Flatten(), nn.Linear(8 * 16 * 16, 10)).cuda()
    images, labels = _loop_data()
    mean, std = _norm(3)
    test = K.ResizedDeviceBatches(images, labels, 16, mean, std, resize=40, crop=32)
    train = K.ResizedDeviceBatches(images, labels, 16, mean, std, resize=40, crop=32, random_resized_crop=True, flip=True, shuffle=True)
    got = K.evaluate(model, test)
    assert torch.equal(test.table, torch.tensor([[i, 4, 4, 32, 32, 0] for i in range(40)], dtype=torch.int32, device="cuda"))
    listed = [ops.prepare_resized_batch(images, test.table[16 * i:16 * i + 16].contiguous(), 40, (32, 32), mean, std, labels=labels) for i in range(3)]
    want = K.evaluate(model, listed)
    print("[feed resize evaluate]", got)
    assert got == want and (got["samples"], got["batches"]) == (40, 3) and math.isfinite(got["loss"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                               # a host read on the iteration path raises
    try:
        batches = list(test) + list(train)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(batches) == 6 and all(tuple(x.shape[1:]) == (3, 32, 32) for x, _ in batches)
    assert math.isfinite(K.evaluate(model, train)["loss"])
