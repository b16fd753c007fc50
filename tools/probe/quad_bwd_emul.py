#!/usr/bin/env python3
"""CPU emulation (numpy) of the quadrant tile of bwd-data on 4x4 planes fed from the position-major copy of dz (k_conv_bwd_data<.., RB = 2>,
csrc/kanconv.hip): tile <-> pixel with the diagonal pairing, the bwd live table, the 16-byte LDS-DMA copies of dz_pm into sG[block][16 outputs][32 images],
the B-operand reads, the contraction.  3x3 / stride 1 / pad 1, B a multiple of 32, O a multiple of 16.  The tile and the pairing are those of
tools/probe/quad_emul.py (imported: one definition); what is new here is the staging.  tests/test_quadrant_bwd_data_order.py checks it against
F.conv_transpose2d.  python tools/probe/quad_bwd_emul.py"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("quad_emul", os.path.join(os.path.dirname(os.path.abspath(__file__)), "quad_emul.py"))
Q = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(Q)

PLANE, NIMG, TP, TAPS = Q.PLANE, Q.NIMG, Q.TP, Q.TAPS
KD = 16                                # outputs per depth step
SG = 4 * KD * NIMG                     # words of the dz tile sG[block][output][image]


def tile_of(tile):
    """tile index -> (first image, quadrant row, quadrant column): the four quadrants of one 32-image group are neighbours."""
    return Q.tile_of(tile)


def block_hw(block, qh, qw):
    """Plane position (h * 4 + w) of a block: 0 = the plane's corner, 1 = the interior position diagonal to it, 2 / 3 = the edge positions in the
    corner's row / column.  Pixel half 0 = blocks {0, 1}, half 1 = blocks {2, 3}."""
    h, w = Q.block_pos(block, qh, qw, "diagonal")
    return h * PLANE + w


def pixel_of(tile, n):
    """Tile column n = block * 32 + image -> (image, row, column)."""
    return Q.pixel_of(tile, n, "diagonal")


def live_mask(hw):
    """The kernel's q_mask: bit tap = r * 3 + t set when input position hw has a source (an output it fed) under the tap."""
    h, w = divmod(hw, PLANE)
    return sum(1 << (r * 3 + t) for r, t in TAPS if 0 <= h + 1 - r < PLANE and 0 <= w + 1 - t < PLANE)


def live_table():
    """[quadrant][tap][block] -> bool."""
    return np.array([[[bool(live_mask(block_hw(blk, q >> 1, q & 1)) >> tap & 1) for blk in range(4)] for tap in range(9)] for q in range(4)])


def copy_plan(tile, tap, o0, B):
    """The dz copies of one step: a list of (wave, instruction j, lane, source element offset into dz_pm, destination word in sG), 4 elements (16 bytes)
    each.  Wave w copies block w: two instructions of 8 outputs; a dead block's copies are not issued.  The source offset is the per-lane fixed part
    (lane = 8 outputs x 8 chunks of 4 images) plus the scalar part (output block, source position, image group)."""
    b0, qh, qw = tile_of(tile)
    r, t = TAPS[tap]
    out = []
    for wave in range(4):
        hw = block_hw(wave, qh, qw)
        if not (live_mask(hw) >> tap) & 1:
            continue
        so = (o0 * 16 + hw + (1 - r) * 4 + (1 - t)) * B + b0
        for j in range(2):
            for lane in range(64):
                voff = (lane >> 3) * 16 * B + (lane & 7) * 4
                out.append((wave, j, lane, voff + so + j * 8 * 16 * B, wave * 512 + j * 256 + lane * 4))
    return out


def read_word(n, k):
    """Word of sG that tile column n reads as its B operand for output k of the step: block * 512 + k * 32 + image."""
    return (n >> 5) * 512 + k * 32 + (n & 31)


def emul_bwd_data(dz, wgt):
    """dx[b][c][h][w] = sum over (o, r, t) of wgt[o][c][r][t] * dz[b][o][h + 1 - r][w + 1 - t] through the tile: per step the copies of copy_plan land in
    sG (NaN before: a read of a word no copy wrote shows), live blocks read read_word and contract, dead blocks are skipped.  Returns (dx, issued copy
    instructions, (lowest, highest) dz_pm element touched)."""
    B, O = dz.shape[:2]
    C = wgt.shape[1]
    dz_pm = np.ascontiguousarray(dz.reshape(B, O * PLANE * PLANE).T).reshape(-1)          # [(o * 16 + position)][image]
    dx = np.zeros((B, C, PLANE, PLANE), dtype=dz.dtype)
    issued, lo, hi = 0, dz_pm.size, -1
    for tile in range(B // 8):
        _, qh, qw = tile_of(tile)
        for tap, (r, t) in enumerate(TAPS):
            for o0 in range(0, O, KD):
                sG = np.full(SG, np.nan, dtype=dz.dtype)
                plan = copy_plan(tile, tap, o0, B)
                issued += len({(w, j) for w, j, *_ in plan})
                for _, _, _, src, dst in plan:
                    assert src % 4 == 0 and dst % 4 == 0 and 0 <= src and src + 4 <= dz_pm.size and 0 <= dst and dst + 4 <= SG
                    sG[dst:dst + 4] = dz_pm[src:src + 4]
                    lo, hi = min(lo, src), max(hi, src + 3)
                for blk in range(4):
                    if not (live_mask(block_hw(blk, qh, qw)) >> tap) & 1:
                        continue
                    for i in range(NIMG):
                        n = blk * 32 + i
                        b, h, w = pixel_of(tile, n)
                        g = sG[[read_word(n, k) for k in range(KD)]]
                        dx[b, :, h, w] += wgt[o0:o0 + KD, :, r, t].T @ g
    return dx, issued, (lo, hi)


if __name__ == "__main__":
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    dz, wgt = rng.standard_normal((64, 32, 4, 4)), rng.standard_normal((32, 3, 3, 3))
    dx, issued, (lo, hi) = emul_bwd_data(dz, wgt)
    ref = F.conv_transpose2d(torch.from_numpy(dz), torch.from_numpy(wgt), padding=1)
    print("bwd-data max |err|", float(np.abs(dx - ref.numpy()).max()), " copy instructions", issued, "of", 8 * 9 * 2 * 8, " dz_pm elements in [%d, %d] of %d" % (lo, hi, dz.size))
    tab = live_table()
    print("live blocks", int(tab[0].sum()), "of", tab[0].size, " per-step maxima over the halves:",
          int(sum(max(tab[0, tap, :2].sum(), tab[0, tap, 2:].sum()) for tap in range(9))), "of 18")
