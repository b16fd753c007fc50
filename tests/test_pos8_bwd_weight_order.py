"""The weight gradient on 8x8 planes with exact tap skipping (k_conv_bwd_weight_pos8: row groups of 32 (channel, plane) pairs under all nine taps, bands
of two images, a k-pair = one plane position of both): its index arithmetic as restated in numpy by tools/probe/pos8_bw_emul.py -- row group -> slab
row, lane -> halo word under each tap, dz DMA and swizzle -> B word, the live tap set of every position, the split ranges -- against a brute-force
weight gradient; the bank sets of every read instruction; and where the planner takes the route.  No GPU."""
import functools
import importlib.util
import os

import numpy as np
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, O, OT = 6, 5, 40, 44                        # three bands; 45 pairs = one full and one partial row group; a 64-output slab inside a 44-channel dz


@functools.lru_cache(maxsize=1)
def _emul():
    spec = importlib.util.spec_from_file_location("pos8_bw_emul", os.path.join(ROOT, "tools", "probe", "pos8_bw_emul.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=1)
def _case():
    """One random problem and its emulated slabs (one split, two splits of 2 + 1 bands), shared by the tests."""
    E = _emul()
    rng = np.random.default_rng(31)
    planes, dz = rng.standard_normal((B, C, 9, 8, 8)), rng.standard_normal((B, OT, 8, 8))
    s1, n1 = E.emul_bwd_weight(planes, dz, 1, O)
    s2, n2 = E.emul_bwd_weight(planes, dz, 2, O)
    return dict(ref=E.reference(planes, dz[:, :O]), s1=s1, s2=s2, n1=n1, n2=n2)


def test_every_slab_row_and_output_is_covered_exactly_once():
    E = _emul()
    for channels in (4, 5, 8, 11, 32):
        seen = {}
        for gi in range(E.n_groups(channels)):
            for m in range(32):
                cp = E.group_pair(gi, m, channels)
                if cp is None:
                    assert 32 * gi + m >= channels * 9
                    continue
                for tap in range(9):
                    row = E.slab_row(cp[0], tap, cp[1])
                    assert row not in seen
                    seen[row] = (gi, m, tap)
        assert sorted(seen) == list(range(channels * 81))                      # rows (c*9 + tap)*9 + p: the halo kernel's channel-major slab
    c = _case()
    assert np.isfinite(c["s1"]).all() and np.isfinite(c["s2"]).all()           # every (row, output < Opad) of every slab was stored (NaN-filled before)
    assert c["s1"].shape == (1, C * 81, 64)


def test_live_taps_equal_the_brute_force_and_count_484_of_576():
    E = _emul()
    total = 0
    for h in range(8):
        for w in range(8):
            want = [r * 3 + t for r in range(3) for t in range(3) if 0 <= h + r - 1 < 8 and 0 <= w + t - 1 < 8]
            assert E.live_taps(h, w) == want, (h, w)
            corner, edge = (h in (0, 7)) and (w in (0, 7)), (h in (0, 7)) != (w in (0, 7))
            assert len(want) == (4 if corner else 6 if edge else 9)
            total += len(want)
            # the lgkmcnt a column waits with = the reads of the next column: one B word + its live taps
            rows = 2 if h in (0, 7) else 3
            assert E.col_reads(w, rows) == 1 + len(want)
    assert total == 484
    c = _case()
    assert set(c["n1"].values()) == {484} and set(c["n2"].values()) == {484}     # per (row group, output tile, band): every live block, no dead one
    assert len(c["n1"]) == E.n_groups(C) * 1 * (B // 2)


def test_halo_words_stay_inside_the_tile_and_taps_read_what_the_expansion_wrote_or_a_border():
    E = _emul()
    for channels in (5, 11):
        for gi in range(E.n_groups(channels)):
            written = {}
            for c, img, h, w in E.expansion_units(gi, channels):
                for p in range(9):
                    word = E.halo_word(gi, c, p, img, h, w)
                    assert 0 <= word < E.HB and word not in written
                    written[word] = (c, p, img, h, w)
            assert E.CELLS not in written                                         # the dump word (pad word of plane 0)
            for lane in range(64):
                cp = E.group_pair(gi, lane & 31, channels)
                for h in range(8):
                    for w in range(8):
                        for tap in range(9):
                            r, t = E.TAPS[tap]
                            word = E.a_word(gi, lane, h, w, tap)
                            assert 0 <= word < E.HB and word != E.CELLS
                            hi, wi = h + r - 1, w + t - 1
                            if cp is None:
                                continue                                           # rows past the last pair: any word of the tile, discarded at the store
                            if 0 <= hi < 8 and 0 <= wi < 8:
                                assert written[word] == (cp[0], cp[1], lane >> 5, hi, wi)
                            else:
                                assert word not in written                          # a zero border cell: what a dead tap would have multiplied


def test_dz_copies_fill_a_buffer_once_and_the_b_reads_find_their_pixel():
    E = _emul()
    ybs = OT * 64
    for o_tile0, outs in ((0, O), (0, 200), (128, 200)):
        plan = E.dma_plan(o_tile0, outs, ybs)
        words = [p[3] for p in plan]
        assert sorted(words) == list(range(E.ZB))                                 # 4 waves x 8 copies x 64 lanes: every word of the buffer once
        at = {p[3]: p[4] for p in plan}
        for wave, j, lane, word, src in plan:
            assert word == (wave * 8 + j) * 64 + lane                             # LDS-DMA: lane i lands at base + 4 i
        for wave in range(4):
            for lane in range(64):
                o = o_tile0 + wave * 32 + (lane & 31)
                for w in range(8):
                    src = at[E.b_word(wave, lane, w)]
                    if o < outs:
                        assert src == o * 64 + w + (lane >> 5) * ybs              # column w of the plane row, image = the lane's k-half
                    else:
                        assert src is None                                        # outputs past O: out-of-range loads, zeros
        # a 64-byte line of the copy = 16 lanes = one output row: two 32-byte runs, one per image
        for wave, j, lane, word, src in plan:
            if src is not None and lane % 16 == 0:
                line = sorted(at[word + i] for i in range(16))
                base = min(line)
                assert line == list(range(base, base + 8)) + list(range(base + ybs, base + ybs + 8))


def test_bank_sets_of_every_read_instruction_are_conflict_free():
    """Bound chosen: no conflict at all (the issue allows 2-way).  ds_read_b32 banks are word % 32 per 32-lane half; the halves never conflict."""
    E = _emul()
    assert E.PS % 2 == 1 and E.PS > E.CELLS
    for gi in range(9):                                                            # every residue of 32 gi mod 9
        for h in range(8):
            for w in range(8):
                for tap in E.live_taps(h, w):
                    assert E.a_read_conflicts(gi, h, w, tap) == [1, 1]
    for wave in range(4):
        for w in range(8):
            assert E.b_read_conflicts(wave, w) == [1, 1]


def test_splits_take_whole_bands_and_leave_none_empty():
    E = _emul()
    for n_bands, splits in ((3, 2), (3, 1), (128, 7), (16, 8), (1, 1)):
        parts = E.split_bands(n_bands, splits)
        assert sum(parts, []) == list(range(n_bands)) and all(parts)
    assert [len(p) for p in E.split_bands(3, 2)] == [2, 1]                       # the uneven boundary of the C = 11, B = 6 GPU case


def test_emulated_walk_reproduces_the_weight_gradient():
    c = _case()
    np.testing.assert_allclose(c["s1"][0, :, :O], c["ref"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(c["s2"].sum(0)[:, :O], c["ref"], rtol=0, atol=1e-11)
    assert (c["s1"][0, :, O:] == 0).all() and (c["s2"][:, :, O:] == 0).all()     # pad outputs of the slab: exact zeros


def _plan(layer, batch, C_, O_, H=8, W=8):
    from convkan_amd import ops
    return ops._plan_cached(layer.conv_spec(), batch, C_, H, W, O_, C_, O_)[2]


def test_the_entry_is_offered_exactly_on_its_scope_with_slabs_that_fill_its_512_slots():
    import convkan_amd as K
    from convkan_amd import _lib as L
    bit = L.ORDER_POS8_BWD_WEIGHT
    assert bit == 32
    for act in (nn.SiLU, nn.GELU):
        for C_, O_, batch, slabs in [(4, 32, 2, 1), (8, 160, 4, 1), (11, 128, 6, 2), (128, 256, 256, None), (256, 256, 256, None)]:
            plan = _plan(K.KANConv2DLayer(C_, O_, 3, padding=1, base_activation=act), batch, C_, O_)
            assert plan.tile_orders & bit and not plan.dz_pm_wanted, (C_, O_, batch)
            assert 1 <= plan.pos8_bw_slabs <= batch // 2                      # whole image pairs per slab, none empty
            bps = -(-(batch // 2) // plan.pos8_bw_slabs)
            assert -(-(batch // 2) // bps) == plan.pos8_bw_slabs
            if slabs is not None:
                assert plan.pos8_bw_slabs == slabs, (C_, O_, batch, plan.pos8_bw_slabs)
            else:                                     # the bench layers: two workgroups per CU are resident, 512 and not 1024
                wgs = -(-C_ * 9 // 32) * (O_ // 128) * plan.pos8_bw_slabs
                assert 448 <= wgs <= 512 or 896 <= wgs <= 1024, wgs
    lay = K.KANConv2DLayer(16, 32, 3, padding=1, base_activation=nn.SiLU)

    def off(plan):
        return not plan.tile_orders & bit and plan.pos8_bw_slabs == 0
    assert off(_plan(lay, 5, 16, 32))                                                                        # odd B: no whole image pairs
    assert off(_plan(lay, 4, 16, 32, 4, 4)) and off(_plan(lay, 4, 16, 32, 16, 16))                           # other planes
    assert off(_plan(K.KANConv2DLayer(16, 32, 3, padding=1, stride=2, base_activation=nn.SiLU), 4, 16, 32, 15, 15))
    assert off(_plan(K.KANConv2DLayer(16, 32, 3, padding=2, dilation=2, base_activation=nn.SiLU), 4, 16, 32))
    assert off(_plan(K.KANConv2DLayer(16, 32, 5, padding=2, base_activation=nn.SiLU), 4, 16, 32))
    assert off(_plan(K.FastKANConv2DLayer(16, 32, 3, padding=1), 4, 16, 32))                                 # two-tensor spec
    assert off(_plan(K.ReLUKANConv2DLayer(16, 32, 3, padding=1), 4, 16, 32))                                 # another single-tensor halo spec
    # more than 8 bands but under one workgroup per CU at the slab count: left to the plan's route, which cuts finer
    assert off(_plan(K.KANConv2DLayer(16, 128, 3, padding=1), 32, 16, 128))
