#!/usr/bin/env python3
"""CPU restatement (numpy) of the index arithmetic of k_conv_fwd_pmdma_wq (csrc/kanconv.hip): the expanded forward on 2x2 planes under
3x3 / stride 1 / pad 1 / dilation 1 with the four output positions on the weight side of a tile.  Tile -> (outputs, images), sW column
<-> (output, position), per-lane LDS-DMA source in wp, accumulator register -> (output, position), split ranges; and, for comparison, the
live-step sequence of k_conv_fwd_pmdma (one output position per tile), which the new order must reproduce per output element.
tests/test_fwd_weight_side_order.py checks them.  python tools/probe/fwd_wq_emul.py"""
import numpy as np

KC, P, HW, T = 18, 9, 4, 9            # rows per step (a channel pair), planes per channel, plane positions, taps
TO, TP = 128, 128                     # A rows (32 outputs x 4 positions) and images per tile
NQ = KC // 2                          # 1-KiB wave copies per operand and step: two rows of 128 floats each


def tap_of(q, p):
    """The one tap under which output position q reads input position p (always inside the 3x3 kernel on a 2x2 plane)."""
    return ((p >> 1) - (q >> 1) + 1) * 3 + ((p & 1) - (q & 1) + 1)


def tile_of(bx, by, B, tiles_o):
    """Block (x, y) of one group -> (first output, first image): grid.x = 4 output sub-tiles x B / 128 image tiles, grid.y = Opad / 128."""
    tiles_b = B // TP
    sub = bx // tiles_b
    return ((by % tiles_o) * 4 + sub) * 32, (bx - sub * tiles_b) * TP


def col_of(o_l, q):
    """sW column of output o_l (0 .. 31) of the tile at output position q."""
    return (o_l >> 4) * 64 + q * 16 + (o_l & 15)


def col_inv(col):
    return (col >> 6) * 16 + (col & 15), (col >> 4) & 3


def dma_w_source(copy, lane, p, pair, C, Opad, o_tile0):
    """Float index into one group's wp of the 16-byte chunk that lane `lane` of wave copy `copy` (0 .. NQ - 1) fetches in step (p, pair), and the
    float index into sW[KC][TO] it lands on.  per-lane part (voffset) + wave-uniform part (soffset), as the kernel splits them."""
    pairs = C // 2
    col = (lane & 31) * 4
    o_l, q = col_inv(col)
    tap0 = (1 - (q >> 1)) * 3 + (1 - (q & 1))                              # tap_of(q, 0)
    voff = (tap0 * pairs * KC + (lane >> 5)) * Opad + o_l
    soff = (((3 * (p >> 1) + (p & 1)) * pairs + pair) * KC) * Opad + o_tile0 + copy * 2 * Opad
    return voff + soff, copy * 256 + lane * 4


def dma_e_source(copy, lane, p, pair, B, b0):
    """Float index into one group's e_pm[((c * HW + pos) * P + plane) * B + b] of the chunk of lane `lane`, copy `copy`, and its place in sE."""
    r = min(2 * copy + (lane >> 5), KC - 1)
    cl, pp = divmod(r, P)
    voff = ((cl * HW) * P + pp) * B + (lane & 31) * 4
    soff = ((2 * pair * HW + p) * P) * B + b0
    return voff + soff, copy * 256 + lane * 4


def wp_index(tap, c, plane, o, C, Opad):
    """Packed forward layout of the expanded route (tap-major items, IPC = 2, KC = 18): wp[k][o]."""
    item = tap * C + c
    return ((item // 2) * KC + (item % 2) * P + plane) * Opad + o


def mfma_row(reg, lane):
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)


def acc_owner(w_o, w_p, mi, ni, reg, lane):
    """Accumulator acc[mi][ni][reg] of lane `lane` in wave (w_o, w_p) -> (output of the tile, position, image of the tile): A row = sW column."""
    o_l, q = col_inv(w_o * 64 + mi * 32 + mfma_row(reg, lane))
    return o_l, q, w_p * 64 + ni * 32 + (lane & 31)


def store_group(w_o, w_p, ni, r, lane):
    """The r-th (0 .. 7) 16-byte store of a lane for image block ni: (output of the tile, image of the tile, the four (mi, reg) it packs, in
    position order)."""
    return w_o * 16 + mfma_row(r, lane), w_p * 64 + ni * 32 + (lane & 31), [(0, r), (0, r + 8), (1, r), (1, r + 8)]


def split_range(z, C, n_splits, target):
    """Steps [s0, s1) of split z (of the grid's n_splits) over the 4 * C / 2 steps in (p, pair) order."""
    L = HW * (C // 2)
    S = min(n_splits, max(1, -(-L // target)))
    if z >= S:
        return L, L
    return L * z // S, (L if z == S - 1 else L * (z + 1) // S)


def k_sequence(q, z, C, n_splits, target):
    """(tap, pair) of the steps split z adds to the outputs at position q, in order: the weight-side kernel."""
    pairs = C // 2
    s0, s1 = split_range(z, C, n_splits, target)
    return [(tap_of(q, s // pairs), s % pairs) for s in range(s0, s1)]


def k_sequence_one_position(q, z, C, n_splits, target):
    """The same for k_conv_fwd_pmdma on a tile of output position q: steps are (tap, pair) over ALL nine taps, dead taps skipped, split ranges
    cut over live steps by live_step_pos."""
    pairs = C // 2
    live = [tap for tap in range(T) if 0 <= (q >> 1) + tap // 3 - 1 < 2 and 0 <= (q & 1) + tap % 3 - 1 < 2]
    n_chunks = T * pairs

    def pos(target_live):
        acc = 0
        for tap in live:
            if target_live < acc + pairs:
                return tap * pairs + (target_live - acc)
            acc += pairs
        return n_chunks

    L = len(live) * pairs
    S = min(n_splits, max(1, -(-L // target)))
    if z >= S:
        return []
    ch0 = 0 if z == 0 else pos(L * z // S)
    ch1 = n_chunks if z == S - 1 else pos(L * (z + 1) // S)
    return [(ch // pairs, ch % pairs) for ch in range(ch0, ch1) if ch // pairs in live]


def lds_bank(float_index):
    return float_index % 32


if __name__ == "__main__":
    for C, S, tgt in ((6, 2, 8), (512, 32, 32)):
        for q in range(4):
            for z in range(S):
                assert k_sequence(q, z, C, S, tgt) == k_sequence_one_position(q, z, C, S, tgt)
    print("k sequences agree; tap table:", [[tap_of(q, p) for p in range(4)] for q in range(4)])
