"""The quadrant tile of bwd-data on 4x4 planes fed from the position-major copy of dz (32 images x a 2x2 quadrant, diagonal pairing, 3x3 / stride 1 /
pad 1): its index arithmetic as restated in numpy by tools/probe/quad_bwd_emul.py -- tile <-> pixel, live table, the 16-byte copies of dz_pm into
sG[block][output][image], the B-operand reads, the contraction.  No GPU."""
import functools
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, O, C = 64, 32, 3                               # two 32-image groups, two 16-output depth blocks


@functools.lru_cache(maxsize=1)
def _emul():
    spec = importlib.util.spec_from_file_location("quad_bwd_emul", os.path.join(ROOT, "tools", "probe", "quad_bwd_emul.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=1)
def _case():
    """One random problem and its emulated result, shared by the tests."""
    E = _emul()
    rng = np.random.default_rng(17)
    dz, wgt = rng.standard_normal((B, O, 4, 4)), rng.standard_normal((O, C, 3, 3))
    dx, issued, span = E.emul_bwd_data(dz, wgt)
    return dict(dz=dz, wgt=wgt, dx=dx, issued=issued, span=span)


def test_every_pixel_of_a_group_sits_in_exactly_one_tile_column():
    E = _emul()
    seen = set()
    for tile in range(8):                         # two 32-image groups x four quadrants
        for n in range(E.TP):
            b, h, w = E.pixel_of(tile, n)
            assert tile // 4 * 32 <= b < tile // 4 * 32 + 32 and h // 2 == (tile >> 1) & 1 and w // 2 == tile & 1
            assert h * 4 + w == E.block_hw(n >> 5, (tile >> 1) & 1, tile & 1)
            seen.add((b, h, w))
    assert len(seen) == 8 * E.TP == 64 * 16


def test_live_table_equals_the_product_touches_a_real_output_and_sums_to_25_of_36():
    E = _emul()
    tab = E.live_table()
    for q in range(4):
        for tap, (r, t) in enumerate(E.TAPS):
            for blk in range(4):
                h, w = divmod(E.block_hw(blk, q >> 1, q & 1), 4)
                assert tab[q, tap, blk] == (0 <= h + 1 - r < 4 and 0 <= w + 1 - t < 4), (q, tap, blk)
        assert tab[q].sum() == 25                                          # of 36 (tap, block) pairs


def test_per_barrier_maxima_sum_to_13_of_18():
    """Pixel half 0 = {corner, interior}, half 1 = {edge, edge}: 2/2 live blocks in four taps, 1/1 in four, 1/0 in one."""
    E = _emul()
    tab = E.live_table()
    for q in range(4):
        pairs = sorted((int(tab[q, tap, :2].sum()), int(tab[q, tap, 2:].sum())) for tap in range(9))
        assert pairs == [(1, 0)] + [(1, 1)] * 4 + [(2, 2)] * 4
        assert sum(max(p) for p in pairs) == 13                            # of 18: one wave per SIMD waits for the slower half


def test_dz_pm_source_of_every_block_output_row_is_128_contiguous_aligned_bytes_inside_the_tensor():
    E = _emul()
    for tile in (0, 3, 5, 6):
        b0, qh, qw = E.tile_of(tile)
        for tap, (r, t) in enumerate(E.TAPS):
            plan = E.copy_plan(tile, tap, 16, B)
            rows = {}
            for wave, j, lane, src, dst in plan:
                rows.setdefault((wave, j * 8 + (lane >> 3)), []).append((src, dst))
            for (blk, o), parts in rows.items():
                parts.sort()
                srcs, dsts = [s for s, _ in parts], [d for _, d in parts]
                h, w = divmod(E.block_hw(blk, qh, qw), 4)
                first = ((16 + o) * 16 + (h + 1 - r) * 4 + (w + 1 - t)) * B + b0            # dz_pm[(output * 16 + source position) * B + first image]
                assert srcs == list(range(first, first + 32, 4)) and first % 4 == 0         # 8 x 16 bytes = 128 contiguous bytes, 16-byte aligned
                assert 0 <= first and first + 32 <= B * O * 16
                assert dsts == list(range(blk * 512 + o * 32, blk * 512 + o * 32 + 32, 4))  # sG[block][output][image]
            assert len(rows) == 16 * sum((E.live_mask(E.block_hw(blk, qh, qw)) >> tap) & 1 for blk in range(4))


def test_no_dead_blocks_copy_is_issued_and_no_lds_read_leaves_the_tile():
    E, c = _emul(), _case()
    tab = E.live_table()
    # two wave instructions per live (block, step); 8 tiles x 2 output blocks
    assert c["issued"] == 2 * 2 * sum(int(tab[tile & 3].sum()) for tile in range(8)) == 2 * 2 * 8 * 25
    assert max(E.copy_plan(0, 4, 0, B), key=lambda e: e[1])[1] == 1 and len({(w, j) for w, j, *_ in E.copy_plan(0, 4, 0, B)}) <= 8
    for n in range(E.TP):
        for k in range(E.KD):
            assert 0 <= E.read_word(n, k) < E.SG
    lanes = [E.read_word(blk * 32 + i, 5) % 32 for blk in range(4) for i in range(32)]
    assert sorted(lanes[:32]) == list(range(32))                          # a block's 32 lanes hit 32 banks
    assert 0 <= c["span"][0] and c["span"][1] < B * O * 16


def test_emulated_gather_and_contraction_reproduce_conv_transpose2d():
    c = _case()
    ref = F.conv_transpose2d(torch.from_numpy(c["dz"]), torch.from_numpy(c["wgt"]), padding=1).numpy()
    assert np.isfinite(c["dx"]).all()              # no live read touched a word that no copy wrote (NaN)
    np.testing.assert_allclose(c["dx"], ref, rtol=0, atol=1e-12)
