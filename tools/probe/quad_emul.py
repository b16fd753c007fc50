#!/usr/bin/env python3
"""CPU emulation (numpy) of the quadrant tile's index arithmetic on 4x4 planes: tile <-> pixel, halo cell, shifted read, live table, dz gather.
3x3 / stride 1 / pad 1, B a multiple of 32.  The forward half is what k_conv_fwd_halo QUAD (csrc/kanconv.hip) runs, line by line, with the
"rows" pairing of the blocks; the bwd-data half (diagonal pairing, per-tap dz gather from NCHW) restates the first variant of k_conv_bwd_data<.., RB = 2>,
which was measured and not shipped; the shipped one keeps this tile and pairing and copies dz from its position-major copy
(tools/probe/quad_bwd_emul.py).  tests/test_quadrant_order.py checks both against F.conv2d.  python tools/probe/quad_emul.py"""
import numpy as np

PLANE, NIMG, TP = 4, 32, 128          # plane side, images per tile, pixels per tile (4 blocks of 32)
HW_, HIMG = 3, 9                      # halo row length and cells per image: the 3x3 input cells a quadrant reaches
HALO = NIMG * HIMG                    # cells per plane of the halo tile (288, as the 8 x 6x6 tile of the row-block order)
HPAD = 4                              # words in front of and behind the halo planes: where a dead block's reads may land
TAPS = [(r, t) for r in range(3) for t in range(3)]


def tile_of(tile):
    """tile index -> (first image, quadrant row, quadrant column): the four quadrants of one 32-image group are neighbours."""
    return (tile >> 2) * NIMG, (tile >> 1) & 1, tile & 1


def block_pos(block, qh, qw, pairing="rows"):
    """Plane position of a 32-pixel block of quadrant (qh, qw); pixel half 0 = blocks {0, 1}, half 1 = blocks {2, 3}.
    "rows" (the forward): half = row of the quadrant, block & 1 = its column -- a lane's two blocks are neighbours in memory (8-byte stores),
    and with one wave of each half on every SIMD the pairing does not matter for the balance.
    "diagonal": block 0 = the plane's corner, 1 = the interior position diagonal to it, 2 / 3 = the edge positions (corner row / corner
    column) -- the halves then skip alike in every tap but one, which is what one wave per SIMD needs."""
    if pairing == "rows":
        return 2 * qh + (block >> 1), 2 * qw + (block & 1)
    h = 3 * qh if block in (0, 2) else 1 + qh
    w = 3 * qw if block in (0, 3) else 1 + qw
    return h, w


def pixel_of(tile, n, pairing="rows"):
    """Tile column n = block * 32 + image -> (image, row, column)."""
    b0, qh, qw = tile_of(tile)
    h, w = block_pos(n >> 5, qh, qw, pairing)
    return b0 + (n & 31), h, w


def live_fwd(h, w, r, t):
    """Forward: output position (h, w) reads a real pixel under tap (r, t)."""
    return 0 <= h + r - 1 < PLANE and 0 <= w + t - 1 < PLANE


def live_bwd(h, w, r, t):
    """bwd-data: input position (h, w) has a source (an output it fed) under tap (r, t): the forward rule with r -> 2 - r, t -> 2 - t."""
    return 0 <= h + 1 - r < PLANE and 0 <= w + 1 - t < PLANE


def live_mask(block, qh, qw, live=live_fwd, pairing="rows"):
    """The kernel's per-block 9-bit mask: bit tap = r * 3 + t."""
    h, w = block_pos(block, qh, qw, pairing)
    return sum(1 << (r * 3 + t) for r, t in TAPS if live(h, w, r, t))


def live_table(live=live_fwd, pairing="rows"):
    """[quadrant][tap][block] -> bool."""
    return np.array([[[bool(live_mask(blk, q >> 1, q & 1, live, pairing) >> tap & 1) for blk in range(4)] for tap in range(9)] for q in range(4)])


# ---------------------------------------------------------------------------------------------------------------- forward
def halo_fill(x, tile, c):
    """The halo plane of channel c (the identity 'expansion'): cell = image * 9 + (input row - qh) * 3 + (input column - qw), all real inputs.
    Returned with its pads of HPAD words (NaN: nothing live may read them)."""
    b0, qh, qw = tile_of(tile)
    sH = np.full(HALO + 2 * HPAD, np.nan, dtype=x.dtype)
    for cell in range(HALO):
        img, rc = divmod(cell, HIMG)
        hr, hc = divmod(rc, HW_)
        sH[HPAD + cell] = x[b0 + img, c, qh + hr, qw + hc]
    return sH


def read_addr(tile, n, r, t):
    """Word address (relative to the first halo cell) that column n reads under tap (r, t): base(n) + shift(tap).  Dead blocks read too."""
    _, qh, qw = tile_of(tile)
    h, w = block_pos(n >> 5, qh, qw)
    return (n & 31) * HIMG + (h - qh) * HW_ + (w - qw) + (r - 1) * HW_ + (t - 1)


def emul_fwd(x, wgt):
    """conv2d(x, wgt, padding=1) on [B][C][4][4] through the tile: per (tile, channel) one halo fill, nine shifted reads, dead blocks skipped.
    Returns (y, lowest address read, highest address read) -- dead blocks included in the address range."""
    B, C = x.shape[:2]
    O = wgt.shape[0]
    y = np.zeros((B, O, PLANE, PLANE), dtype=x.dtype)
    lo, hi = 0, 0
    for tile in range(B // 8):
        _, qh, qw = tile_of(tile)
        for c in range(C):
            sH = halo_fill(x, tile, c)
            for tap, (r, t) in enumerate(TAPS):
                for blk in range(4):
                    addrs = [read_addr(tile, blk * 32 + i, r, t) for i in range(32)]
                    lo, hi = min(lo, *addrs), max(hi, *addrs)
                    if not (live_mask(blk, qh, qw) >> tap) & 1:
                        continue
                    for i, a in enumerate(addrs):
                        b, h, w = pixel_of(tile, blk * 32 + i)
                        y[b, :, h, w] += wgt[:, c, r, t] * sH[HPAD + a]
    return y, lo, hi


# ---------------------------------------------------------------------------------------------------------------- bwd-data
def gather_offset(tile, n, r, t):
    """Element offset into dz[b][o = 0] of the output that input pixel (column n) fed under tap (r, t), or None (the buffer load's
    out-of-bounds offset: the lane reads zero) -- per thread and tap, the per-step output offset is added on the scalar side."""
    b, h, w = pixel_of(tile, n, "diagonal")
    ho, wo = h + 1 - r, w + 1 - t
    if not (0 <= ho < PLANE and 0 <= wo < PLANE):
        return None
    return b, ho * PLANE + wo


def emul_bwd_data(dz, wgt):
    """Transpose of emul_fwd: dx[b][c][h][w] = sum over (o, r, t) of wgt[o][c][r][t] * dz[b][o][h + 1 - r][w + 1 - t], dead blocks skipped."""
    B, O = dz.shape[:2]
    C = wgt.shape[1]
    dzf = dz.reshape(B, O, PLANE * PLANE)
    dx = np.zeros((B, C, PLANE, PLANE), dtype=dz.dtype)
    for tile in range(B // 8):
        _, qh, qw = tile_of(tile)
        for tap, (r, t) in enumerate(TAPS):
            for blk in range(4):
                alive = (live_mask(blk, qh, qw, live_bwd, "diagonal") >> tap) & 1
                for i in range(32):
                    n = blk * 32 + i
                    src = gather_offset(tile, n, r, t)
                    assert (src is not None) == bool(alive), "a block is wholly live or wholly dead"
                    if src is None:
                        continue
                    b, h, w = pixel_of(tile, n, "diagonal")
                    dx[b, :, h, w] += wgt[:, :, r, t].T @ dzf[src[0], :, src[1]]
    return dx


if __name__ == "__main__":
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    x, wgt = rng.standard_normal((64, 3, 4, 4)), rng.standard_normal((5, 3, 3, 3))
    y, lo, hi = emul_fwd(x, wgt)
    ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(wgt), padding=1)
    print("forward  max |err|", float(np.abs(y - ref.numpy()).max()), " reads in [%d, %d] of [%d, %d]" % (lo, hi, -HPAD, HALO + HPAD - 1))
    dz = rng.standard_normal((64, 5, 4, 4))
    dref = F.conv_transpose2d(torch.from_numpy(dz), torch.from_numpy(wgt), padding=1)
    print("bwd-data max |err|", float(np.abs(emul_bwd_data(dz, wgt) - dref.numpy()).max()))
    tab = live_table(pairing="diagonal")
    print("live blocks", int(tab.sum()), "of", tab.size, " per-step maxima over the halves:",
          int(sum(max(tab[0, tap, :2].sum(), tab[0, tap, 2:].sum()) for tap in range(9))), "of 18")
