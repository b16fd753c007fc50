"""The quadrant tile on 4x4 planes (32 images x a 2x2 quadrant, 3x3 / stride 1 / pad 1): its index arithmetic as restated in numpy by
tools/probe/quad_emul.py -- live table, forward gather through the halo, bwd-data gather, LDS read range.  No GPU."""
import functools
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=1)
def _emul():
    spec = importlib.util.spec_from_file_location("quad_emul", os.path.join(ROOT, "tools", "probe", "quad_emul.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=1)
def _case():
    """One random problem (64 images = two 32-image groups, 3 channels, 5 outputs) and its emulated / reference results, shared by the tests."""
    Q = _emul()
    rng = np.random.default_rng(7)
    x, wgt, dz = rng.standard_normal((64, 3, 4, 4)), rng.standard_normal((5, 3, 3, 3)), rng.standard_normal((64, 5, 4, 4))
    y, lo, hi = Q.emul_fwd(x, wgt)
    return dict(x=x, wgt=wgt, dz=dz, y=y, lo=lo, hi=hi, dx=Q.emul_bwd_data(dz, wgt))


def test_every_pixel_of_a_group_sits_in_exactly_one_tile_column():
    Q = _emul()
    for pairing in ("rows", "diagonal"):
        seen = set()
        for tile in range(8):                     # two 32-image groups x four quadrants
            for n in range(Q.TP):
                b, h, w = Q.pixel_of(tile, n, pairing)
                assert tile // 4 * 32 <= b < tile // 4 * 32 + 32 and h // 2 == (tile >> 1) & 1 and w // 2 == tile & 1
                seen.add((b, h, w))
        assert len(seen) == 8 * Q.TP == 64 * 16


def test_live_table_equals_the_product_touches_a_real_pixel():
    Q = _emul()
    for live, sign, pairing in ((Q.live_fwd, +1, "rows"), (Q.live_fwd, +1, "diagonal"), (Q.live_bwd, -1, "diagonal")):
        tab = Q.live_table(live, pairing)
        for q in range(4):
            for tap, (r, t) in enumerate(Q.TAPS):
                for blk in range(4):
                    h, w = Q.block_pos(blk, q >> 1, q & 1, pairing)
                    hs, ws = h + sign * (r - 1), w + sign * (t - 1)          # forward: the input read; bwd-data: the output that was fed
                    assert tab[q, tap, blk] == (0 <= hs < 4 and 0 <= ws < 4), (q, tap, blk)


def test_totals_25_of_36_live_and_13_of_18_per_step_maxima():
    Q = _emul()
    for q in range(4):
        assert Q.live_table(Q.live_fwd, "rows")[q].sum() == 25             # the forward's pairing: the same 25 of 36, two blocks of a row per wave
    for live in (Q.live_fwd, Q.live_bwd):
        tab = Q.live_table(live, "diagonal")
        for q in range(4):
            assert tab[q].sum() == 25                                      # of 36 (tap, block) pairs
            assert tab[q, :, :2].sum() == 13 and tab[q, :, 2:].sum() == 12  # half 0 = {corner, interior}, half 1 = the two edges
            per_step = [max(tab[q, tap, :2].sum(), tab[q, tap, 2:].sum()) for tap in range(9)]
            assert sum(per_step) == 13                                     # of 18: one wave per SIMD waits for the slower half
            assert sum(tab[q, tap, :2].sum() != tab[q, tap, 2:].sum() for tap in range(9)) == 1      # the halves skip alike in every step but one


def test_emulated_forward_gather_reproduces_conv2d():
    c = _case()
    ref = F.conv2d(torch.from_numpy(c["x"]), torch.from_numpy(c["wgt"]), padding=1).numpy()
    assert np.isfinite(c["y"]).all()               # no live read touched the (NaN) pads
    np.testing.assert_allclose(c["y"], ref, rtol=0, atol=1e-12)


def test_emulated_bwd_data_gather_reproduces_the_transpose():
    c = _case()
    ref = F.conv_transpose2d(torch.from_numpy(c["dz"]), torch.from_numpy(c["wgt"]), padding=1).numpy()
    np.testing.assert_allclose(c["dx"], ref, rtol=0, atol=1e-12)


def test_a_lanes_two_blocks_are_neighbours_in_the_planes_row():
    """The forward stores a lane's two outputs as one 8-byte word: block 1 (3) sits one column right of block 0 (2), at an even column."""
    Q = _emul()
    for q in range(4):
        for half in range(2):
            (h0, w0), (h1, w1) = Q.block_pos(2 * half, q >> 1, q & 1), Q.block_pos(2 * half + 1, q >> 1, q & 1)
            assert h0 == h1 and w1 == w0 + 1 and w0 % 2 == 0


def test_no_lds_read_leaves_the_padded_tile_dead_blocks_included():
    Q, c = _emul(), _case()
    assert -Q.HPAD <= c["lo"] and c["hi"] <= Q.HALO + Q.HPAD - 1
    # and live reads stay inside the reading image's own nine cells
    for tile in range(4):
        _, qh, qw = Q.tile_of(tile)
        for n in range(Q.TP):
            for tap, (r, t) in enumerate(Q.TAPS):
                if (Q.live_mask(n >> 5, qh, qw) >> tap) & 1:
                    a = Q.read_addr(tile, n, r, t)
                    assert (n & 31) * Q.HIMG <= a < (n & 31) * Q.HIMG + Q.HIMG
