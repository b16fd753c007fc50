#!/usr/bin/env python3
"""Writes tests/golden/feed_resize/feed_resize_pil.npz: PIL's own bytes for the small cells of tests/resize_cases.py and for one horizontal pass n -> 224 of
every length in PIL_LENGTHS, so that the restatement can be held against PIL where PIL is not installed.  Only PIL computes here: the calls
are the ones torchvision makes on PIL images (``Image.resize(size, BILINEAR)``, ``Image.crop``, ``Image.transpose(FLIP_LEFT_RIGHT)``;
``Grayscale(3)`` on a mode-L image is ``np.dstack`` of three copies).

    python tests/golden/make_golden_resize.py        (needs Pillow; made with 12.2.0)"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_cases as RC   # noqa: E402


def _to_pil(chw):
    return Image.fromarray(np.ascontiguousarray(chw.transpose(1, 2, 0))) if chw.shape[0] == 3 else [Image.fromarray(np.ascontiguousarray(p)) for p in chw]


def _resize(img, hw):
    """``Resize`` on a PIL image, or on a list of mode-L images (channel counts PIL has no mode for: every band is resampled alone anyway)."""
    if isinstance(img, list):
        return [_resize(p, hw) for p in img]
    return img.resize((hw[1], hw[0]), Image.BILINEAR)


def _apply(img, fn):
    return [fn(p) for p in img] if isinstance(img, list) else fn(img)


def _to_chw(img):
    if isinstance(img, list):
        return np.stack([np.asarray(p) for p in img])
    return np.asarray(img).transpose(2, 0, 1)


def pil_pipeline_u8(images, table, size, out_hw, channels_last, out_channels=None):
    """uint8 [B, out_channels, Ho, Wo]: Resize, crop, Resize of the box, flip, Grayscale(3), by PIL."""
    chw = RC.to_chw(images, channels_last)
    _, C, H, W = chw.shape
    Rh, Rw = RC.resized_hw(H, W, size)
    out = []
    for index, top, left, h, w, flip in np.asarray(table).tolist():
        img = _resize(_to_pil(chw[index]), (Rh, Rw))
        img = _apply(img, lambda p: p.crop((left, top, left + w, top + h)))
        img = _resize(img, out_hw)
        if flip:
            img = _apply(img, lambda p: p.transpose(Image.FLIP_LEFT_RIGHT))
        a = _to_chw(img)
        out.append(a if out_channels in (None, C) else np.repeat(a, out_channels, axis=0))
    return np.stack(out)


def pil_length_pass(n, m=224):
    a = RC.length_image(n)
    return np.asarray(Image.fromarray(a[0]).resize((m, a.shape[1]), Image.BILINEAR))[None]


def build():
    arrays = {}
    for name, ((C, H, W), size, out_hw, oc) in RC.CELLS.items():
        c = RC.cell(name)
        arrays[name] = pil_pipeline_u8(c["images"], c["table"], size, out_hw, True, oc)
    for n in RC.PIL_LENGTHS:
        arrays[f"len_{n}"] = pil_length_pass(n)
    return arrays


if __name__ == "__main__":
    arrays = build()
    np.savez_compressed(RC.GOLDEN, **arrays)
    print(RC.GOLDEN, os.path.getsize(RC.GOLDEN), "bytes,", len(arrays), "arrays")
