"""Numpy restatement of the index arithmetic of k_conv_bwd_weight_pos8 (csrc/kanconv.hip): the weight gradient of the default B-spline specs on 8x8
planes under 3x3 / stride 1 / pad 1, with exact tap skipping.

  row group gi      32 consecutive (c, p) pairs q = c*9 + p, q in [32 gi, 32 gi + 32); a workgroup = one group x 128 outputs, a wave = the group under all
                    nine taps x 32 outputs; block row m of tap `tap` lands in slab row (c*9 + tap)*9 + p
  band              two whole images; a step is one plane row h of both, a k-pair one column w: the two depth rows of the MFMA are images 0 and 1
  halo tile         sH[(ch*9 + p) * PS + img*100 + (h + 1)*10 + (w + 1)], ch = c - c0, c0 = 32 gi // 9: at most 5 channels; borders stay zero
  A operand         lane (m = lane & 31, k = lane >> 5) under tap (r, t) at (h, w): word (32 gi + m - 9 c0)*PS + k*100 + (h + r)*10 + (w + t)
  dz tile           sZ[buffer][o][16 words], word = px ^ ((o >> 1) & 15), px = 2*w + img; written by 4-byte LDS-DMA (lane i of a 64-lane copy lands at
                    base + 4 i, so the swizzle is applied to the SOURCE a lane reads), read by lane (n = lane & 31, k) of wave wv at column w as
                    o = 32 wv + n, word (2 w + k) ^ ((o >> 1) & 15)
  live taps         tap row r is dead on plane row 0 (r = 0) and 7 (r = 2), tap column t on column 0 (t = 0) and 7 (t = 2): neither its ds_read nor its
                    MFMA is emitted -- 484 of the 576 (position, tap) blocks of a plane remain

Used by tests/test_pos8_bwd_weight_order.py; run as a script it prints the bank sets of every read instruction."""
import numpy as np

W, HWC, HIMG, CELLS = 8, 10, 100, 200
PS = CELLS + 1                    # plane stride in words (odd)
P, T, NCH = 9, 9, 5
TAPS = [(r, t) for r in range(3) for t in range(3)]
ZB = 16 * 128                     # words per dz buffer
HB = NCH * P * PS                 # words of the halo tile
NT = 256


def n_groups(C):
    return -(-C * P // 32)


def group_pair(gi, m, C):
    """(c, p) of block row m of row group gi, or None past the last pair."""
    q = 32 * gi + m
    return (q // P, q % P) if q < C * P else None


def slab_row(c, tap, p):
    return (c * T + tap) * P + p


def c0_of(gi):
    return 32 * gi // P


def halo_word(gi, c, p, img, h, w):
    """Where the expansion of x[img][c][h][w] writes plane p (stage_unit: column base + p * PS)."""
    return ((c - c0_of(gi)) * P + p) * PS + img * HIMG + (h + 1) * HWC + (w + 1)


def a_word(gi, lane, h, w, tap):
    r, t = TAPS[tap]
    base = (32 * gi + (lane & 31) - c0_of(gi) * P) * PS + (lane >> 5) * HIMG        # the lane's register
    return base + h * HWC + (r * HWC + t + w)                                      # + row of the step + the immediate


def row_kind(h):
    return 0 if h == 0 else 2 if h == W - 1 else 1


def live_taps(h, w):
    """Taps whose read and MFMA the kernel emits at position (h, w): the row bodies drop a tap row, pos8_col_live a tap column."""
    rk = row_kind(h)
    r0, r1 = (1 if rk == 0 else 0), (1 if rk == 2 else 2)
    return [r * 3 + t for r in range(r0, r1 + 1) for t in range(3) if 0 <= w + t - 1 < W]


def col_reads(w, rows):
    """ds_reads of column w (the B word + the live taps): the lgkmcnt the previous column waits with."""
    return 1 + rows * (2 if w in (0, W - 1) else 3)


def dma_plan(o_tile0, O, ybs):
    """Per (wave, copy j, lane): (LDS word inside a buffer, source offset in floats relative to dz[first image of the band][0][plane row][0], or None)."""
    out = []
    for wave in range(4):
        for j in range(8):
            for lane in range(64):
                ol = 4 * (wave * 8 + j) + (lane >> 4)
                q = (lane & 15) ^ ((ol >> 1) & 15)
                src = (o_tile0 + ol) * 64 + (q >> 1) + (q & 1) * ybs if o_tile0 + ol < O else None
                out.append((wave, j, lane, wave * 512 + j * 64 + lane, src))
    return out


def b_word(wave, lane, w):
    ol = wave * 32 + (lane & 31)
    return ol * 16 + ((2 * w + (lane >> 5)) ^ ((ol >> 1) & 15))


def split_bands(n_bands, splits):
    bps = -(-n_bands // splits)
    return [list(range(z * bps, min(n_bands, z * bps + bps))) for z in range(splits)]


def expansion_units(gi, C):
    """(channel, image, h, w) of every expansion a workgroup makes per band: unit idx = thread + 256 k."""
    units = []
    for idx in range(NCH * 2 * 64):
        ch, img, pos = idx >> 7, (idx >> 6) & 1, idx & 63
        if c0_of(gi) + ch < C:
            units.append((c0_of(gi) + ch, img, pos >> 3, pos & 7))
    return units


def banks(words):
    """Largest number of distinct words on one of the 32 banks of a ds_read_b32 lane half."""
    worst = 0
    for bank in range(32):
        worst = max(worst, len({w for w in words if w % 32 == bank}))
    return worst


def a_read_conflicts(gi, h, w, tap):
    return [banks([a_word(gi, lane, h, w, tap) for lane in range(half * 32, half * 32 + 32)]) for half in (0, 1)]


def b_read_conflicts(wave, w):
    return [banks([b_word(wave, lane, w) for lane in range(half * 32, half * 32 + 32)]) for half in (0, 1)]


def emul_bwd_weight(planes, dz, splits, O=None):
    """planes[B][C][9][8][8] (the expanded inputs, any numbers), dz[B][Ot][8][8] of which the first O (default: all) are the layer's.  Walks
    workgroups, splits, bands, steps, k-pairs and live taps through the LDS images exactly as the kernel addresses them.
    Returns (slabs[splits][C*81][Opad], issued blocks per (group, output tile, band))."""
    B, C = planes.shape[:2]
    O = dz.shape[1] if O is None else O
    ybs = dz[0].size
    Opad = -(-O // 64) * 64
    flat = dz.reshape(-1)
    slabs = np.full((splits, C * T * P, Opad), np.nan)
    lanes = np.arange(64)
    issued = {}
    for gi in range(n_groups(C)):
        for ot in range(-(-Opad // 128)):
            plan = dma_plan(ot * 128, O, ybs)
            lds_w = np.array([p[3] for p in plan])
            src = np.array([-1 if p[4] is None else p[4] for p in plan])
            for z, bands in enumerate(split_bands(B // 2, splits)):
                acc = np.zeros((T, 4, 32, 32))                                         # [tap][wave][row m][output n]
                sH = np.zeros(HB)
                for band in bands:
                    for c, img, h, w in expansion_units(gi, C):
                        for p in range(P):
                            sH[halo_word(gi, c, p, img, h, w)] = planes[2 * band + img, c, p, h, w]
                    count = 0
                    for h in range(W):
                        sZ = np.full(ZB, np.nan)
                        soff = 2 * band * ybs + h * W
                        sZ[lds_w] = np.where(src >= 0, flat[np.clip(src + soff, 0, flat.size - 1)], 0.0)
                        for w in range(W):
                            for tap in live_taps(h, w):
                                a = sH[[a_word(gi, lane, h, w, tap) for lane in lanes]]      # [64]: lane -> A[m][k]
                                for wave in range(4):
                                    b = sZ[[b_word(wave, lane, w) for lane in lanes]]
                                    acc[tap, wave] += np.outer(a[:32], b[:32]) + np.outer(a[32:], b[32:])
                                count += 1
                    issued[(gi, ot, band)] = count
                for m in range(32):
                    cp = group_pair(gi, m, C)
                    if cp is None:
                        continue
                    for tap in range(T):
                        for wave in range(4):
                            o0 = ot * 128 + wave * 32
                            n = max(0, min(32, Opad - o0))
                            slabs[z, slab_row(cp[0], tap, cp[1]), o0:o0 + n] = acc[tap, wave, m, :n]
    return slabs, issued


def reference(planes, dz):
    """dw[(c*9 + tap)*9 + p][o] = sum over images and output positions of planes[b][c][p][h + r - 1][w + t - 1] * dz[b][o][h][w]."""
    B, C = planes.shape[:2]
    O = dz.shape[1]
    pad = np.zeros((B, C, P, W + 2, W + 2))
    pad[..., 1:-1, 1:-1] = planes
    out = np.zeros((C * T * P, O))
    for tap, (r, t) in enumerate(TAPS):
        win = pad[..., r:r + W, t:t + W]
        d = np.einsum("bcphw,bohw->cpo", win, dz)
        for c in range(C):
            out[[slab_row(c, tap, p) for p in range(P)]] = d[c]
    return out


if __name__ == "__main__":
    worst_a = max(max(a_read_conflicts(gi, h, w, tap)) for gi in range(9) for h in range(W) for w in range(W) for tap in live_taps(h, w))
    worst_b = max(max(b_read_conflicts(wave, w)) for wave in range(4) for w in range(W))
    print(f"plane stride {PS}: A reads {worst_a}-way at worst, B reads {worst_b}-way; halo tile {HB * 4} bytes, dz 2 x {ZB * 4} bytes")
    print("live (position, tap) blocks per plane:", sum(len(live_taps(h, w)) for h in range(W) for w in range(W)), "of", 64 * 9)
