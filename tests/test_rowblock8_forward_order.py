"""The half-plane row-block tile of the halo forward on 8x8 planes (4 images x 4 rows x 8 columns, pixels ordered (row, image, column), 3x3 / stride 1 /
pad 1): its index arithmetic as restated in numpy by tools/probe/rowblk8_emul.py -- tile <-> pixel, the dead blocks that depend on the tile's first
row (top-half and bottom-half tiles), the shifted halo reads.  No GPU."""
import functools
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=1)
def _emul():
    spec = importlib.util.spec_from_file_location("rowblk8_emul", os.path.join(ROOT, "tools", "probe", "rowblk8_emul.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=1)
def _case():
    """One random problem (8 images = two 4-image groups = four tiles, top and bottom halves; 3 channels, 5 outputs), emulated once for all tests."""
    Q = _emul()
    rng = np.random.default_rng(8)
    x, wgt = rng.standard_normal((8, 3, 8, 8)), rng.standard_normal((5, 3, 3, 3))
    y, lo, hi, dead_real = Q.emul_fwd(x, wgt)
    return dict(x=x, wgt=wgt, y=y, lo=lo, hi=hi, dead_real=dead_real)


def test_every_pixel_of_a_group_sits_in_exactly_one_tile_column():
    Q = _emul()
    seen = set()
    for tile in range(4):                         # two 4-image groups x two halves
        for n in range(Q.TP):
            b, h, w = Q.pixel_of(tile, n)
            assert tile // 2 * 4 <= b < tile // 2 * 4 + 4 and h // 4 == tile & 1 and 0 <= w < 8
            seen.add((b, h, w))
    assert len(seen) == 4 * Q.TP == 8 * 64


def test_a_block_is_one_plane_row_of_the_four_images_and_a_lanes_run_is_one_image_row():
    Q = _emul()
    for tile in range(4):
        for blk in range(4):
            px = [Q.pixel_of(tile, blk * 32 + i) for i in range(32)]
            assert {h for _, h, _ in px} == {Q.tile_of(tile)[1] + blk}
            for i in range(0, 32, 8):             # 8 consecutive lanes: 8 consecutive columns of one image row (a 32-byte run of the store)
                assert [w for _, _, w in px[i:i + 8]] == list(range(8)) and len({b for b, _, _ in px[i:i + 8]}) == 1


def test_dead_blocks_are_exactly_the_blocks_whose_source_row_leaves_the_plane():
    """... which depends on the tile's first row: only plane row 0 (top-half tiles) and plane row 7 (bottom-half tiles) ever die."""
    Q = _emul()
    for tile in range(4):
        _, h0 = Q.tile_of(tile)
        for blk in range(4):
            for r in range(3):
                assert Q.block_dead(tile, blk, r) == (not 0 <= h0 + blk + r - 1 < Q.PLANE), (tile, blk, r)


def test_every_tile_skips_one_block_in_three_of_nine_taps():
    """1/12 of the MFMA blocks, every tile alike, and always in one pixel half: half 0 of a top-half tile, half 1 of a bottom-half tile."""
    Q = _emul()
    for tile in range(4):
        per_tap = [[Q.block_dead(tile, blk, r) for blk in range(4)] for r, _ in Q.TAPS]
        assert sum(map(sum, per_tap)) == 3 and all(sum(p) <= 1 for p in per_tap)                 # 3 of 36 = 1/12
        halves = {blk >> 1 for p in per_tap for blk in range(4) if p[blk]}
        assert halves == {tile & 1}


def test_dead_blocks_read_only_the_zero_border_and_no_read_leaves_the_tile():
    Q, c = _emul(), _case()
    assert c["dead_real"] == 0                                       # exact: every skipped product multiplies a zero cell
    assert 0 <= c["lo"] and c["hi"] <= Q.HALO - 1                    # dead blocks included
    assert 2 * Q.HALO <= 512                                         # one cell of the channel pair per thread


def test_emulated_forward_reproduces_conv2d_top_and_bottom_tiles():
    c = _case()
    ref = F.conv2d(torch.from_numpy(c["x"]), torch.from_numpy(c["wgt"]), padding=1).numpy()
    np.testing.assert_allclose(c["y"], ref, rtol=0, atol=1e-12)
