#!/usr/bin/env python3
"""CPU emulation (numpy) of the half-plane row-block tile of the halo forward on 8x8 planes (k_conv_fwd_halo<FAST, 4, 8, 4, 4>, csrc/kanconv.hip):
tile <-> pixel, halo cell, shifted read, dead blocks.  3x3 / stride 1 / pad 1, B a multiple of 4.  A tile is 4 images x 4 rows x 8 columns, its 128
pixel columns are ordered n = (row, image, column), so a 32-pixel MFMA block is ONE plane row of the 4 images; the block of plane row 0 is dead under
tap row 0 and the block of plane row 7 under tap row 2 (every product reads the zero border), which depends on the tile's first row h0.
tests/test_rowblock8_forward_order.py checks this against F.conv2d.  python tools/probe/rowblk8_emul.py"""
import numpy as np

PLANE, W, R, NIMG, TP = 8, 8, 4, 4, 128   # plane side, row length, rows / images per tile, pixels per tile (4 blocks of 32)
HW_ = W + 2                               # halo row length: a zero column on either side
HIMG = (R + 2) * HW_                      # halo cells per image: the tile's rows plus one above and one below
HALO = NIMG * HIMG                        # cells per plane of the halo tile (240; two channels of a pair = 480 <= 512 threads)
TAPS = [(r, t) for r in range(3) for t in range(3)]


def tile_of(tile):
    """tile index -> (first image, first plane row): the two halves of a 4-image group are neighbours; B / 2 tiles as with whole planes of 2 images."""
    return (tile >> 1) * NIMG, (tile & 1) * R


def pixel_of(tile, n):
    """Tile column n = (row, image, column) -> (image, plane row, column)."""
    b0, h0 = tile_of(tile)
    row, rem = divmod(n, NIMG * W)
    img, col = divmod(rem, W)
    return b0 + img, h0 + row, col


def block_dead(tile, block, r):
    """The kernel's `dead` test: wave half w_p = block >> 1 owns tile rows 2 w_p and 2 w_p + 1 (its blocks q = 0, 1)."""
    _, h0 = tile_of(tile)
    w_p, q = block >> 1, block & 1
    dead = 0 if (r == 0 and w_p == 0 and h0 == 0) else 1 if (r == 2 and w_p == 1 and h0 + R == PLANE) else -1
    return dead == q


def halo_fill(x, tile, c):
    """The halo plane of channel c (the identity 'expansion'): cell = image * HIMG + (plane row - h0 + 1) * HW_ + (column + 1); cells outside the plane stay zero."""
    b0, h0 = tile_of(tile)
    sH = np.zeros(HALO, dtype=x.dtype)
    real = np.zeros(HALO, dtype=bool)
    for cell in range(HALO):
        img, rc = divmod(cell, HIMG)
        hr, hc = divmod(rc, HW_)
        h, w = h0 - 1 + hr, hc - 1
        if 0 <= h < PLANE and 0 <= w < W:
            sH[cell], real[cell] = x[b0 + img, c, h, w], True
    return sH, real


def read_addr(n, r, t):
    """Word address (relative to the first halo cell) that column n reads under tap (r, t): base(n) + shift(tap).  Dead blocks would read there too."""
    row, rem = divmod(n, NIMG * W)
    img, col = divmod(rem, W)
    return img * HIMG + (row + 1) * HW_ + (col + 1) + (r - 1) * HW_ + (t - 1)


def emul_fwd(x, wgt):
    """conv2d(x, wgt, padding=1) on [B][C][8][8] through the tile: per (tile, channel) one halo fill, nine shifted reads, dead blocks skipped.
    Returns (y, lowest address read, highest address read, number of real cells a dead block would have read) -- dead blocks included in the range."""
    B, C = x.shape[:2]
    O = wgt.shape[0]
    y = np.zeros((B, O, PLANE, PLANE), dtype=x.dtype)
    lo, hi, dead_real = HALO, 0, 0
    for tile in range(B // 2):
        for c in range(C):
            sH, real = halo_fill(x, tile, c)
            for r, t in TAPS:
                for blk in range(4):
                    addrs = [read_addr(blk * 32 + i, r, t) for i in range(32)]
                    lo, hi = min(lo, *addrs), max(hi, *addrs)
                    if block_dead(tile, blk, r):
                        dead_real += int(real[addrs].sum())
                        continue
                    for i, a in enumerate(addrs):
                        b, h, w = pixel_of(tile, blk * 32 + i)
                        y[b, :, h, w] += wgt[:, c, r, t] * sH[a]
    return y, lo, hi, dead_real


if __name__ == "__main__":
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    x, wgt = rng.standard_normal((8, 3, 8, 8)), rng.standard_normal((5, 3, 3, 3))
    y, lo, hi, dead_real = emul_fwd(x, wgt)
    ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(wgt), padding=1)
    print("forward  max |err|", float(np.abs(y - ref.numpy()).max()), " reads in [%d, %d] of [0, %d]; real cells under dead blocks: %d" % (lo, hi, HALO - 1, dead_real))
    dead = sum(block_dead(tile, blk, r) for tile in range(2) for blk in range(4) for r, _ in TAPS)
    print("dead (block, tap) pairs", dead, "of", 2 * 4 * 9)
