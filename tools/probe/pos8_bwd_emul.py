#!/usr/bin/env python3
"""CPU emulation (numpy) of the row-segment tile of bwd-data on 8x8 planes fed from the position-major copy of dz (k_conv_bwd_data<.., RB = 3>,
csrc/kanconv.hip): dispatch slot -> tile, tile <-> pixel, the live tap rows (whole steps) and tap columns (blocks), the 16-byte LDS-DMA copies of dz_pm
into sG[block][16 outputs][32 images], the B-operand reads, the split ranges over the live steps, the contraction.  3x3 / stride 1 / pad 1, B a
multiple of 32, O a multiple of 16.  tests/test_pos8_bwd_data_order.py checks it against a brute-force transposed-convolution index computation and
F.conv_transpose2d.  python tools/probe/pos8_bwd_emul.py"""
import numpy as np

PLANE, NIMG, TP, KD = 8, 32, 128, 16
TAPS = [(r, t) for r in range(3) for t in range(3)]
SG = 4 * KD * NIMG                     # words of the dz tile sG[block][output][image]


def n_tiles(B):
    return B // 2                      # 16 per 32-image group


def dispatch_tile(slot, tiles):
    """Dispatch slot (blockIdx.x) -> tile: the twelve 9-tap tiles (rows 1-6) of every image group first, then all h = 0 tiles, then all h = 7 tiles;
    inside a class the image group is slot % groups (workgroups go to the 8 XCDs round-robin: with 8 groups an XCD works on one group's dz_pm and x)."""
    ng = tiles >> 4
    nmid = 12 * ng
    if slot < nmid:
        k = slot // ng
        return (slot - k * ng) * 16 + 2 + k
    y = slot - nmid
    cls = 1 if y >= 2 * ng else 0
    y2 = y - cls * 2 * ng
    k = y2 // ng
    return (y2 - k * ng) * 16 + cls * 14 + k


def tile_of(tile):
    """tile -> (first image, plane row h, first column w0): tile = image group * 16 + 2 h + w0 / 4."""
    return (tile >> 4) * 32, (tile >> 1) & 7, (tile & 1) * 4


def pixel_of(tile, n):
    """Tile column n = block * 32 + image -> (image, row, column); block j is position (h, w0 + j)."""
    b0, h, w0 = tile_of(tile)
    return b0 + (n & 31), h, w0 + (n >> 5)


def tap_mask(tile):
    """The kernel's tapmask: bit tap set when the tap's source row h + 1 - r lies in the plane (dead tap rows are skipped as whole steps)."""
    _, h, _ = tile_of(tile)
    return sum(7 << (3 * r) for r in range(3) if 0 <= h + 1 - r < PLANE)


def block_live(tile, tap, block):
    """A block of a LIVE step is issued unless its source column w0 + block + 1 - t leaves the plane."""
    _, _, w0 = tile_of(tile)
    return 0 <= w0 + block + 1 - TAPS[tap][1] < PLANE


def mfma_flags(tile, tap):
    """(l0, l3) as the kernel forms them: block 0 is dead under t = 2 in the w0 = 0 tiles, block 3 under t = 0 in the w0 = 4 tiles; blocks 1, 2 always live."""
    _, _, w0 = tile_of(tile)
    t = tap % 3
    return not (w0 == 0 and t == 2), not (w0 == 4 and t == 0)


def issued(tile, tap, block):
    """The block's MFMAs are issued: the step is live and the block's flag is set."""
    l0, l3 = mfma_flags(tile, tap)
    return bool(tap_mask(tile) >> tap & 1) and (l0 if block == 0 else l3 if block == 3 else True)


def source_position(tile, tap, block):
    """Source position (ho * 8 + wo) of a block under a tap, as the scalar offset of its copy forms it (valid only where issued)."""
    _, h, w0 = tile_of(tile)
    r, t = TAPS[tap]
    return (h + 1 - r) * PLANE + (w0 + block + 1 - t)


def split_range(tile, z, S, n_ob):
    """Steps [(tap, output block)] of slab z of S: the tile's live steps in order, cut into S equal shares (live_step_pos)."""
    live = [tap * n_ob + ob for tap in range(9) if tap_mask(tile) >> tap & 1 for ob in range(n_ob)]
    L = len(live)
    S_eff = min(S, max(1, L))
    if z >= S_eff:
        return []
    return live[L * z // S_eff:L * (z + 1) // S_eff]


def copy_plan(tile, tap, o0, B):
    """The dz copies of one live step: (wave, instruction j, lane, source element offset into dz_pm, destination word in sG), 4 elements (16 bytes) each.
    Wave w copies block w: two instructions of 8 outputs; a dead block's copies are not issued.  Source = per-lane fixed part (lane = 8 outputs x 8 chunks
    of 4 images, 64 positions per output) + scalar part (output block, source position, image group)."""
    b0, h, w0 = tile_of(tile)
    r, t = TAPS[tap]
    out = []
    for wave in range(4):
        col = w0 + wave
        if not 0 <= col + 1 - t < PLANE:
            continue
        so = (o0 * 64 + (h + 1 - r) * 8 + (col + 1 - t)) * B + b0
        for j in range(2):
            for lane in range(64):
                voff = (lane >> 3) * 64 * B + (lane & 7) * 4
                out.append((wave, j, lane, voff + so + j * 8 * 64 * B, wave * 512 + j * 256 + lane * 4))
    return out


def read_word(n, k):
    """Word of sG that tile column n reads as its B operand for output k of the step: block * 512 + k * 32 + image."""
    return (n >> 5) * 512 + k * 32 + (n & 31)


def emul_bwd_data(dz, wgt, splits=1):
    """dx[b][c][h][w] = sum over (o, r, t) of wgt[o][c][r][t] * dz[b][o][h + 1 - r][w + 1 - t] through the tile, slab by slab: per live step the copies of
    copy_plan land in sG (NaN before: a read of a word no copy wrote shows), issued blocks read read_word and contract.  Returns (dx, issued (block, step)
    count, (lowest, highest) dz_pm element touched)."""
    B, O = dz.shape[:2]
    n_ob = O // KD
    dz_pm = np.ascontiguousarray(dz.reshape(B, O * PLANE * PLANE).T).reshape(-1)          # [(o * 64 + position)][image]
    dx = np.zeros((B,) + wgt.shape[1:2] + (PLANE, PLANE), dtype=dz.dtype)
    blocks, lo, hi = 0, dz_pm.size, -1
    tiles = n_tiles(B)
    for slot in range(tiles):
        tile = dispatch_tile(slot, tiles)
        for z in range(splits):
            for step in split_range(tile, z, splits, n_ob):
                tap, ob = divmod(step, n_ob)
                r, t = TAPS[tap]
                sG = np.full(SG, np.nan, dtype=dz.dtype)
                for _, _, _, src, dst in copy_plan(tile, tap, ob * KD, B):
                    assert src % 4 == 0 and dst % 4 == 0 and 0 <= src and src + 4 <= dz_pm.size and 0 <= dst and dst + 4 <= SG
                    sG[dst:dst + 4] = dz_pm[src:src + 4]
                    lo, hi = min(lo, src), max(hi, src + 3)
                for blk in range(4):
                    if not issued(tile, tap, blk):
                        continue
                    blocks += 1
                    for i in range(NIMG):
                        n = blk * 32 + i
                        b, h, w = pixel_of(tile, n)
                        g = sG[[read_word(n, k) for k in range(KD)]]
                        dx[b, :, h, w] += wgt[ob * KD:(ob + 1) * KD, :, r, t].T @ g
    return dx, blocks, (lo, hi)


if __name__ == "__main__":
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    dz, wgt = rng.standard_normal((64, 32, 8, 8)), rng.standard_normal((32, 3, 3, 3))
    dx, blocks, (lo, hi) = emul_bwd_data(dz, wgt, splits=2)
    ref = F.conv_transpose2d(torch.from_numpy(dz), torch.from_numpy(wgt), padding=1)
    print("bwd-data max |err|", float(np.abs(dx - ref.numpy()).max()), " issued blocks", blocks, "of", 2 * 576 * 2,
          " dz_pm elements in [%d, %d] of %d" % (lo, hi, dz.size))
    per_group = sum(issued(tile, tap, blk) for tile in range(16) for tap in range(9) for blk in range(4))
    print("live blocks per image group", per_group, "of", 16 * 9 * 4)
