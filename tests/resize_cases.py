"""The reference of the resized-feed tests (test_feed_resize.py, test_gpu_feed_resize.py): a test-side restatement, in plain Python floats and
numpy integers, of what torchvision does to one sample in the loader's ImageNet branch (utils/dataloader.py:26-54) on PIL images --
``Resize`` (PIL's 8-bit BILINEAR resampling: a horizontal pass into a uint8 image, then a vertical pass), crop, ``Resize`` of the box, flip,
``Grayscale(3)`` on a one-channel image (a plain copy) -- plus the seeded datasets and the tables the cells run on.  It is independent of
``data.resample_coeffs``: the coefficients are computed here output by output, as Resample.c's ``precompute_coeffs`` and
``normalize_coeffs_8bpc`` do, in Python floats (IEEE doubles, one rounding per operation).  test_feed_resize.py checks it against PIL itself
where PIL is installed, and against tests/golden/feed_resize/feed_resize_pil.npz (PIL's bytes, made by tests/golden/make_golden_resize.py) everywhere."""
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feed_resize", "feed_resize_pil.npz")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)             # dataloader.py:9-10
N_IMAGES = 9
ZERO_IMAGE, FULL_IMAGE = 3, 7              # the all-0 and the all-255 image of every dataset


@functools.lru_cache(maxsize=None)
def coeffs(n, m):
    """(xmin [m], count [m], k [m][ksize]) of one bilinear pass from n to m samples over the whole axis, as Python lists."""
    scale = n / m
    fs = scale if scale > 1.0 else 1.0
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmins, counts, ks = [], [], []
    for xx in range(m):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)                 # C's (int): truncation
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > n:
            xmax = n
        xmax -= xmin
        w, ww = [], 0.0
        for x in range(xmax):
            t = (x + xmin - center + 0.5) * ss
            if t < 0.0:
                t = -t
            v = 1.0 - t if t < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]
        xmins.append(xmin), counts.append(xmax), ks.append(k + [0] * (ksize - xmax))
    return xmins, counts, ks


def resample_last_axis(a, m):
    """uint8 [..., n] -> uint8 [..., m]: one pass, int32 arithmetic."""
    n = a.shape[-1]
    xmins, counts, ks = coeffs(n, m)
    src = a.astype(np.int32)
    out = np.empty(a.shape[:-1] + (m,), dtype=np.uint8)
    for xx in range(m):
        acc = np.full(a.shape[:-1], 1 << 21, dtype=np.int32)
        for t in range(counts[xx]):
            acc = acc + src[..., xmins[xx] + t] * np.int32(ks[xx][t])
        out[..., xx] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def resize(chw, Rh, Rw):
    """uint8 [C, H, W] -> [C, Rh, Rw]: the horizontal pass, a uint8 image, the vertical pass."""
    hor = resample_last_axis(chw, Rw)
    return np.ascontiguousarray(resample_last_axis(hor.transpose(0, 2, 1), Rh).transpose(0, 2, 1))


def resized_hw(H, W, size):
    """``Resize(size)``: an int makes the smaller edge ``size`` and the longer ``int(size * long / short)``; a pair is (Rh, Rw)."""
    if size is None:
        return H, W
    if isinstance(size, int):
        return (size, int(size * W / H)) if H <= W else (int(size * H / W), size)
    return tuple(size)


def to_chw(images, channels_last):
    a = images if images.ndim == 4 else images[..., None] if channels_last else images[:, None]
    return a.transpose(0, 3, 1, 2) if channels_last else a


def pipeline_u8(images, table, size, out_hw, channels_last, out_channels=None):
    """uint8 [B, out_channels, Ho, Wo] for a table of good rows (index, top, left, h, w, flip)."""
    chw = to_chw(images, channels_last)
    n, C, H, W = chw.shape
    Rh, Rw = resized_hw(H, W, size)
    OC = C if out_channels is None else out_channels
    out = np.zeros((len(table), OC) + tuple(out_hw), dtype=np.uint8)
    stage1 = {}
    for b, (index, top, left, h, w, flip) in enumerate(np.asarray(table).tolist()):
        assert 0 <= index < n and h >= 1 and w >= 1 and 0 <= top <= Rh - h and 0 <= left <= Rw - w
        if index not in stage1:
            stage1[index] = resize(chw[index], Rh, Rw)
        img = resize(stage1[index][:, top:top + h, left:left + w], *out_hw)
        if flip:
            img = img[:, :, ::-1]
        out[b] = img if OC == C else np.repeat(img, OC, axis=0)
    return out


def make_images(C, H, W, channels_last, seed=0, n=N_IMAGES):
    """uint8 [n, H, W, C] or [n, C, H, W], seeded; bytes 0 and 255 in every image, one image all 0 and one all 255."""
    rng = np.random.default_rng(seed + 1000 * C + 10 * H + W)
    a = rng.integers(0, 256, size=(n, C, H, W), dtype=np.uint8)
    a[:, 0, 0, 0], a[:, -1, -1, -1] = 0, 255
    a[ZERO_IMAGE], a[FULL_IMAGE] = 0, 255
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)) if channels_last else a


def box_table(Rh, Rw, Ho, Wo, n=N_IMAGES):
    """int32 [rows, 6] of (index, top, left, h, w, flip) on a stage-1 image of Rh x Rw: the whole image plain and flipped, the centre crop
    (stage 2 the identity) where it fits, a box smaller than the output, 1 x 1 boxes inside and in the last corner, a box on each corner
    (touching two edges each), a one-column and a one-row box of full extent, and the all-255 and all-0 images."""
    hs, ws = max(1, min(Rh, Ho // 2 - 1)), max(1, min(Rw, Wo // 2))
    hc, wc = min(Rh, 3), min(Rw, 5)
    rows = [(n - 1, 0, 0, Rh, Rw, 0), (0, 0, 0, Rh, Rw, 1)]
    if Ho <= Rh and Wo <= Rw:
        rows.append((5, int(round((Rh - Ho) / 2.0)), int(round((Rw - Wo) / 2.0)), Ho, Wo, 0))
    rows += [(4, min(1, Rh - hs), min(2, Rw - ws), hs, ws, 1), (2, Rh // 2, Rw // 3, 1, 1, 0), (6, Rh - 1, Rw - 1, 1, 1, 1),
             (1, 0, 0, hc, wc, 0), (1, 0, Rw - wc, hc, wc, 1), (8, Rh - hc, 0, hc, wc, 1), (8, Rh - hc, Rw - wc, hc, wc, 0),
             (5, 0, Rw // 2, Rh, 1, 0), (2, Rh // 2, 0, 1, Rw, 1), (FULL_IMAGE, 0, 0, Rh, Rw, 1), (ZERO_IMAGE, 0, 0, max(1, Rh - 1), Rw, 0)]
    return np.array(rows, dtype=np.int32)


# name: (C, H, W), Resize argument, (Ho, Wo), out_channels
CELLS = {
    "c3_8x8_r20_to_12x12": ((3, 8, 8), 20, (12, 12), None),            # both stages resample; the whole-image box downscales with ksize 5
    "c1_7x5_r10_to_6x6_x3": ((1, 7, 5), 10, (6, 6), 3),                # Resize(10): 14 x 10; one channel to three; Wo % 4 != 0; ksize 7
    "c3_8x8_r8_to_12x12": ((3, 8, 8), None, (12, 12), None),           # stage 1 the identity
    "c3_8x8_r20_to_20x20": ((3, 8, 8), 20, (20, 20), None),            # the whole-image box: stage 2 the identity
    "c3_8x12_r_none_to_8x12": ((3, 8, 12), None, (8, 12), None),       # both the identity on the whole-image box
    "c2_9x6_r13x10_to_5x7": ((2, 9, 6), (13, 10), (5, 7), None),       # a pair for Resize, 54-byte images, two channels
}


def chunks(n, B):
    """Row ranges of B rows that cover range(n): consecutive, the last one moved back to end at n."""
    return [(min(s, n - B), min(s, n - B) + B) for s in range(0, n, B)]


@functools.lru_cache(maxsize=None)
def cell(name):
    """The channels_last dataset, the table and the restated bytes of one cell, computed once."""
    (C, H, W), size, out_hw, oc = CELLS[name]
    images = make_images(C, H, W, channels_last=True)
    Rh, Rw = resized_hw(H, W, size)
    table = box_table(Rh, Rw, *out_hw)
    return dict(images=images, table=table, size=size, resized=(Rh, Rw), out_hw=out_hw, out_channels=oc, C=C,
                u8=pipeline_u8(images, table, size, out_hw, True, oc))


# the comparisons against PIL: (mode, (H, W), Resize or None, box (top, left, h, w) of the resized image or None, (Ho, Wo))
PIL_CASES = [
    ("RGB", (32, 32), (256, 256), None, (256, 256)),
    ("RGB", (32, 32), (256, 256), (17, 40, 200, 180), (224, 224)),
    ("RGB", (32, 32), (256, 256), (0, 0, 256, 256), (224, 224)),
    ("RGB", (32, 32), (256, 256), (100, 3, 20, 27), (224, 224)),
    ("RGB", (32, 32), (256, 256), (3, 60, 250, 190), (224, 224)),
    ("RGB", (32, 32), (256, 256), (16, 16, 224, 224), (224, 224)),
    ("RGB", (32, 32), (256, 256), (255, 255, 1, 1), (224, 224)),
    ("RGB", (32, 32), (256, 256), (0, 131, 256, 97), (224, 224)),
    ("L", (28, 28), (224, 224), None, (224, 224)),
    ("RGB", (5, 7), (12, 9), None, (12, 9)),
    ("RGB", (13, 11), (7, 5), None, (7, 5)),
    ("RGB", (256, 256), None, None, (224, 224)),
]
PIL_LENGTHS = (1, 2, 3, 31, 32, 33, 223, 224, 225, 255, 256)           # source lengths n -> 224, on both axes


def pil_case_image(mode, hw, seed):
    C = 3 if mode == "RGB" else 1
    a = np.random.default_rng(seed).integers(0, 256, size=(C,) + tuple(hw), dtype=np.uint8)
    a[:, 0, 0], a[:, -1, -1] = 0, 255
    return a


def length_image(n):
    """uint8 [1, 4, n]: four rows of n seeded bytes, for one horizontal pass n -> 224."""
    a = np.random.default_rng(7000 + n).integers(0, 256, size=(1, 4, n), dtype=np.uint8)
    a[0, 0, 0], a[0, -1, -1] = 0, 255
    return a
