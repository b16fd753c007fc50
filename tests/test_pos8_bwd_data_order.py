"""The row-segment tile of bwd-data on 8x8 planes fed from the position-major copy of dz (32 images x 4 adjacent columns of one plane row, 3x3 /
stride 1 / pad 1; k_conv_bwd_data<.., RB = 3>): its index arithmetic as restated in numpy by tools/probe/pos8_bwd_emul.py -- dispatch slot -> tile,
tile <-> pixel, live tap rows and columns, source positions, the 16-byte copies of dz_pm, the split ranges, the contraction -- against a brute-force
transposed-convolution index computation; and where kan_tile_orders reports the route.  No GPU."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, O, C = 64, 32, 3                               # two 32-image groups, two 16-output depth blocks


@functools.lru_cache(maxsize=1)
def _emul():
    spec = importlib.util.spec_from_file_location("pos8_bwd_emul", os.path.join(ROOT, "tools", "probe", "pos8_bwd_emul.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=1)
def _case():
    """One random problem and its emulated results (one slab, three slabs), shared by the tests."""
    E = _emul()
    rng = np.random.default_rng(23)
    dz, wgt = rng.standard_normal((B, O, 8, 8)), rng.standard_normal((O, C, 3, 3))
    dx1, blocks1, span = E.emul_bwd_data(dz, wgt, 1)
    dx3, blocks3, _ = E.emul_bwd_data(dz, wgt, 3)
    return dict(dz=dz, wgt=wgt, dx1=dx1, dx3=dx3, blocks1=blocks1, blocks3=blocks3, span=span)


def _brute_source(h, w, r, t):
    """Transposed convolution, by the forward's rule: output (ho, wo) reads input (ho - 1 + r, wo - 1 + t); input (h, w) therefore receives, under
    tap (r, t), from the one output with ho - 1 + r == h and wo - 1 + t == w, if it exists."""
    for ho in range(8):
        for wo in range(8):
            if ho - 1 + r == h and wo - 1 + t == w:
                return ho * 8 + wo
    return None


def test_source_position_and_liveness_of_every_tile_tap_block_equal_the_brute_force():
    E = _emul()
    for tile in range(E.n_tiles(B)):
        b0, h, w0 = E.tile_of(tile)
        assert b0 == tile // 16 * 32 and 0 <= h < 8 and w0 in (0, 4)
        for tap, (r, t) in enumerate(E.TAPS):
            for blk in range(4):
                want = _brute_source(h, w0 + blk, r, t)
                assert E.issued(tile, tap, blk) == (want is not None), (tile, tap, blk)
                # the copy's liveness (its own column test inside a live step) and the MFMA flags agree
                if E.tap_mask(tile) >> tap & 1:
                    assert E.block_live(tile, tap, blk) == E.issued(tile, tap, blk)
                if want is not None:
                    assert E.source_position(tile, tap, blk) == want


def test_live_blocks_per_image_group_are_484_of_576_and_edge_rows_hold_two_thirds_of_the_steps():
    E = _emul()
    for grp in range(B // 32):
        tiles = range(grp * 16, grp * 16 + 16)
        assert sum(E.issued(tile, tap, blk) for tile in tiles for tap in range(9) for blk in range(4)) == 484
        for tile in tiles:
            h = E.tile_of(tile)[1]
            assert bin(E.tap_mask(tile)).count("1") == (6 if h in (0, 7) else 9)
    c = _case()
    assert c["blocks1"] == c["blocks3"] == 484 * (B // 32) * (O // 16)


def test_every_plane_position_of_every_image_is_covered_once():
    E = _emul()
    seen = set()
    for tile in range(E.n_tiles(B)):
        for n in range(E.TP):
            p = E.pixel_of(tile, n)
            assert p not in seen
            seen.add(p)
    assert seen == {(b, h, w) for b in range(B) for h in range(8) for w in range(8)}


@pytest.mark.parametrize("batch", [32, 64, 256])
def test_dispatch_order_is_a_permutation_longest_first_with_each_edge_class_contiguous(batch):
    E = _emul()
    tiles = E.n_tiles(batch)
    order = [E.dispatch_tile(s, tiles) for s in range(tiles)]
    assert sorted(order) == list(range(tiles))
    rows = [E.tile_of(t)[1] for t in order]
    ng = tiles // 16
    assert all(1 <= h <= 6 for h in rows[:12 * ng]) and rows[12 * ng:14 * ng] == [0] * (2 * ng) and rows[14 * ng:] == [7] * (2 * ng)
    assert all(E.tile_of(t)[0] // 32 == s % ng for s, t in enumerate(order))          # image group = slot % groups (one group per XCD when there are 8)


@pytest.mark.parametrize("S", [1, 2, 3, 4, 5])
def test_split_ranges_partition_the_live_steps_evenly(S):
    E = _emul()
    n_ob = 3
    for tile in (0, 1, 2, 9, 14, 15):
        parts = [E.split_range(tile, z, S, n_ob) for z in range(S)]
        live = [tap * n_ob + ob for tap in range(9) if E.tap_mask(tile) >> tap & 1 for ob in range(n_ob)]
        assert sum(parts, []) == live
        assert max(map(len, parts)) - min(map(len, parts)) <= 1


def test_dz_pm_source_of_every_block_output_row_is_128_contiguous_aligned_bytes_inside_the_tensor():
    E = _emul()
    for tile in (0, 1, 6, 15, 16, 30, 31):
        b0, h, w0 = E.tile_of(tile)
        for tap, (r, t) in enumerate(E.TAPS):
            if not E.tap_mask(tile) >> tap & 1:
                continue
            plan = E.copy_plan(tile, tap, 16, B)
            rows = {}
            for wave, j, lane, src, dst in plan:
                rows.setdefault((wave, j * 8 + (lane >> 3)), []).append((src, dst))
            for (blk, o), parts in rows.items():
                parts.sort()
                srcs, dsts = [s for s, _ in parts], [d for _, d in parts]
                first = ((16 + o) * 64 + (h + 1 - r) * 8 + (w0 + blk + 1 - t)) * B + b0      # dz_pm[(output * 64 + source position) * B + first image]
                assert srcs == list(range(first, first + 32, 4)) and first % 4 == 0           # 8 x 16 bytes = 128 contiguous bytes, 16-byte aligned
                assert 0 <= first and first + 32 <= B * O * 64
                assert dsts == list(range(blk * 512 + o * 32, blk * 512 + o * 32 + 32, 4))    # sG[block][output][image]
            assert len(rows) == 16 * sum(E.issued(tile, tap, blk) for blk in range(4))
    for n in range(E.TP):
        for k in range(E.KD):
            assert 0 <= E.read_word(n, k) < E.SG
    assert sorted(E.read_word(2 * 32 + i, 5) % 32 for i in range(32)) == list(range(32))    # a block's 32 lanes hit 32 banks
    c = _case()
    assert 0 <= c["span"][0] and c["span"][1] < B * O * 64


def test_emulated_copies_and_contraction_reproduce_conv_transpose2d():
    c = _case()
    ref = F.conv_transpose2d(torch.from_numpy(c["dz"]), torch.from_numpy(c["wgt"]), padding=1).numpy()
    for dx in (c["dx1"], c["dx3"]):
        assert np.isfinite(dx).all()               # no issued block read a word that no copy wrote (NaN)
        np.testing.assert_allclose(dx, ref, rtol=0, atol=1e-12)


def _orders(layer, batch, C_, O_, H=8, W=8):
    from convkan_amd import ops
    _, _, plan = ops._plan_cached(layer.conv_spec(), batch, C_, H, W, O_, C_, O_)
    return plan


def test_kan_tile_orders_reports_the_route_exactly_on_its_scope():
    import convkan_amd as K
    from convkan_amd import _lib as L
    bit = L.ORDER_POS8_BWD_DATA
    assert bit == 16
    for act in (nn.SiLU, nn.GELU):
        for C_, O_, batch in [(8, 16, 32), (14, 16, 32), (20, 48, 32), (16, 32, 64), (128, 256, 256), (256, 256, 256)]:
            plan = _orders(K.KANConv2DLayer(C_, O_, 3, padding=1, base_activation=act), batch, C_, O_)
            assert plan.tile_orders & bit and not plan.dz_pm_wanted, (C_, O_, batch)
    lay = K.KANConv2DLayer(16, 32, 3, padding=1, base_activation=nn.SiLU)
    assert not _orders(lay, 48, 16, 32).tile_orders & bit                                       # no whole 32-image groups
    assert not _orders(K.KANConv2DLayer(16, 24, 3, padding=1, base_activation=nn.SiLU), 32, 16, 24).tile_orders & bit      # O % 16 != 0
    assert not _orders(lay, 32, 16, 32, 4, 4).tile_orders & bit                                 # 4x4 planes: the quadrant route's
    assert not _orders(lay, 32, 16, 32, 16, 16).tile_orders & bit
    assert not _orders(K.KANConv2DLayer(16, 32, 3, padding=1, stride=2, base_activation=nn.SiLU), 32, 16, 32, 15, 15).tile_orders & bit   # 8x8 outputs, stride 2
    assert not _orders(K.KANConv2DLayer(16, 32, 3, padding=1, stride=2, base_activation=nn.SiLU), 32, 16, 32).tile_orders & bit
    assert not _orders(K.FastKANConv2DLayer(16, 32, 3, padding=1), 32, 16, 32).tile_orders & bit                         # two-tensor spec
