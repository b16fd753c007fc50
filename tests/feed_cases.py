"""The reference of the batch-preparation tests (test_feed.py, test_gpu_feed.py): a test-side restatement, in numpy / torch on the CPU, of what
torchvision does to one sample in the loader's non-ImageNet branch (utils/dataloader.py:56-90) -- pad the uint8 image with zeros, crop, flip,
ToTensor (``/ 255``), Normalize (``sub_(mean).div_(std)``) -- plus the seeded datasets and the tables the cells run on.  torchvision is not
installed where the tests run, so there is no frozen golden from it; test_feed.py cross-checks the placement half against PIL, the calls
torchvision makes on PIL inputs."""
import numpy as np
import torch

CIFAR10_MEAN, CIFAR10_STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)        # dataloader.py:73
MNIST_MEAN, MNIST_STD = (0.1307,), (0.3081,)                                           # dataloader.py:59
N_IMAGES = 37
ZERO_IMAGE, FULL_IMAGE = 3, 7              # the all-0 and the all-255 image of every dataset

# (C, H, W), (Ho, Wo), padding p of the offset range  top in [-p, H - Ho + p], left in [-p, W - Wo + p]
SHAPES = {
    "c3_32x32": ((3, 32, 32), (32, 32), 4),            # CIFAR: RandomCrop(32, padding=4); 3072-byte images, float4 rows
    "c1_28x28": ((1, 28, 28), (28, 28), 2),            # MNIST's size: 784-byte images
    "c3_5x7": ((3, 5, 7), (5, 7), 1),                  # 105-byte images: no 16-byte stride, Wo % 4 != 0
    "c3_32x32_to_24x20": ((3, 32, 32), (24, 20), 4),   # a crop smaller than the image, Wo % 4 == 0 while the image is wider
    "c2_9x6_to_13x10": ((2, 9, 6), (13, 10), 3),       # the output larger than the source: padding on every side
}


def make_images(C, H, W, channels_last, seed=0, n=N_IMAGES):
    """uint8 [n, H, W, C] or [n, C, H, W], seeded; bytes 0 and 255 in every image, one image all 0 and one all 255."""
    rng = np.random.default_rng(seed + 1000 * C + 10 * H + W)
    a = rng.integers(0, 256, size=(n, C, H, W), dtype=np.uint8)
    a[:, 0, 0, 0], a[:, -1, -1, -1] = 0, 255
    a[ZERO_IMAGE], a[FULL_IMAGE] = 0, 255
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)) if channels_last else a


def corner_table(H, W, Ho, Wo, p, n=N_IMAGES):
    """int32 [11, 4]: every corner of the offset range with flip 0 and with flip 1 on random images whose indices descend and repeat, from the
    last image to the first; then the all-255 and the all-0 image on opposite corners and one row in the middle of the range."""
    tops, lefts = (-p, H - Ho + p), (-p, W - Wo + p)
    index = [n - 1, n - 1, 30, 20, 20, 11, 0, 0]
    corners = [(top, left) for top in tops for left in lefts]
    rows = [(index[4 * flip + i], top, left, flip) for flip in (0, 1) for i, (top, left) in enumerate(corners)]
    rows += [(FULL_IMAGE, tops[0], lefts[0], 1), (ZERO_IMAGE, tops[1], lefts[1], 0), (12, (tops[0] + tops[1]) // 2, (lefts[0] + lefts[1]) // 2, 1)]
    return np.array(rows, dtype=np.int32)


def chunks(n, B):
    """Row ranges of B rows that cover range(n): consecutive, the last one moved back to end at n."""
    return [(min(s, n - B), min(s, n - B) + B) for s in range(0, n, B)]


def gather_u8(images, table, out_hw, channels_last):
    """uint8 [B, C, Ho, Wo]: pad with zeros, slice, reverse W -- torchvision's pad / crop / hflip on the raw bytes.  Also the mask of the
    pixels that came from the padding."""
    a = images if images.ndim == 4 else images[..., None] if channels_last else images[:, None]
    chw = a.transpose(0, 3, 1, 2) if channels_last else a
    n, C, H, W = chw.shape
    Ho, Wo = out_hw
    ph, pw = H + Ho, W + Wo
    out = np.zeros((len(table), C, Ho, Wo), dtype=np.uint8)
    pad = np.zeros_like(out, dtype=bool)
    for b, (index, top, left, flip) in enumerate(np.asarray(table).tolist()):
        assert 0 <= index < n and abs(top) <= ph and abs(left) <= pw
        big = np.pad(chw[index], ((0, 0), (ph, ph), (pw, pw)), constant_values=0)
        inside = np.pad(np.ones((C, H, W), dtype=bool), ((0, 0), (ph, ph), (pw, pw)), constant_values=False)
        win = (slice(None), slice(top + ph, top + ph + Ho), slice(left + pw, left + pw + Wo))
        crop, live = big[win], inside[win]
        if flip:
            crop, live = crop[:, :, ::-1], live[:, :, ::-1]
        out[b], pad[b] = crop, ~live
    return out, pad


def to_tensor_normalize(u8, mean, std, dtype):
    """ToTensor then Normalize with torch CPU ops in torchvision's order: ``.to(dtype).div(255)``, ``.sub_(mean).div_(std)``; mean and std are the
    fp32 values Normalize makes of its arguments (``torch.as_tensor(mean, dtype=tensor.dtype)`` on an fp32 tensor), in both precisions."""
    m = torch.tensor(mean, dtype=torch.float32).to(dtype).view(1, -1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).to(dtype).view(1, -1, 1, 1)
    t = torch.from_numpy(np.ascontiguousarray(u8)).to(dtype).div(255)
    return t.sub_(m).div_(s)


def restate(images, table, out_hw, mean, std, channels_last):
    """(u8 gather, padding mask, r32, r64) for a table of good rows."""
    u8, pad = gather_u8(images, table, out_hw, channels_last)
    return u8, pad, to_tensor_normalize(u8, mean, std, torch.float32), to_tensor_normalize(u8, mean, std, torch.float64)


def padding_values(mean, std):
    """(0 - mean[c]) / std[c] in fp32, operation by operation."""
    m, s = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    return (np.float32(0) / np.float32(255) - m) / s
