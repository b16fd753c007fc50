"""The weight-side tile of the expanded forward on 2x2 planes (32 outputs x 4 positions x 128 images; k_conv_fwd_pmdma_wq): its index
arithmetic as restated in numpy by tools/probe/fwd_wq_emul.py.  No GPU."""
import functools
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=1)
def _emul():
    spec = importlib.util.spec_from_file_location("fwd_wq_emul", os.path.join(ROOT, "tools", "probe", "fwd_wq_emul.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_output_element_is_produced_exactly_once_and_stored_in_whole_groups():
    E = _emul()
    B, Opad = 256, 256
    tiles_o, tiles_x = Opad // 128, 4 * (B // E.TP)
    seen = set()
    for by in range(tiles_o):
        for bx in range(tiles_x):
            o0, b0 = E.tile_of(bx, by, B, tiles_o)
            assert o0 % 32 == 0 and o0 + 32 <= Opad and b0 % E.TP == 0 and b0 + E.TP <= B
            for w_o in range(2):
                for w_p in range(2):
                    for lane in range(64):
                        for ni in range(2):
                            for r in range(8):
                                o_l, b_l, regs = E.store_group(w_o, w_p, ni, r, lane)
                                for q, (mi, reg) in enumerate(regs):       # the four floats of the 16-byte store: positions 0 .. 3 of ONE (b, o)
                                    assert E.acc_owner(w_o, w_p, mi, ni, reg, lane) == (o_l, q, b_l)
                                    key = (b0 + b_l, o0 + o_l, q)
                                    assert key not in seen
                                    seen.add(key)
    assert len(seen) == B * Opad * 4
    # the 16 accumulator registers of a block are the eight stores' two registers each: nothing is left unstored
    assert sorted(reg for r in range(8) for (mi, reg) in E.store_group(0, 0, 0, r, 0)[2] if mi == 0) == list(range(16))
    # a wave's store instruction r: registers r & 3 of the two lane halves tile 8 consecutive outputs = one 128-byte line of z[b][o][0..3] per four stores
    for half in (0, 1):
        outs = sorted(E.store_group(0, 0, 0, r, 32 * half)[0] for r in range(4))
        assert outs == [4 * half + i for i in range(4)]


@pytest.mark.parametrize("C", [2, 6, 64, 512])
@pytest.mark.parametrize("S", [1, 3, 32])
def test_k_sequence_per_output_equals_the_one_position_kernels_live_steps(C, S):
    E = _emul()
    for target in (1, 8, 32):
        for q in range(4):
            total = []
            for z in range(S):
                seq = E.k_sequence(q, z, C, S, target)
                assert seq == E.k_sequence_one_position(q, z, C, S, target), (q, z, target)
                total += seq
            live = sorted({t for t, _ in total})
            assert len(live) == 4 and total == [(t, pr) for t in live for pr in range(C // 2)]      # every live (tap, pair) once, ascending


def test_tap_table_matches_the_convolution():
    E = _emul()
    for q in range(4):
        for p in range(4):
            tap = E.tap_of(q, p)
            r, t = divmod(tap, 3)
            assert 0 <= tap < 9 and ((q >> 1) + r - 1, (q & 1) + t - 1) == (p >> 1, p & 1)


def test_a_reads_of_32_lanes_hit_32_banks():
    E = _emul()
    for w_o in range(2):
        for mi in range(2):
            for kk in range(E.KC // 2):
                for kh2 in range(2):
                    banks = {E.lds_bank((2 * kk + kh2) * E.TO + w_o * 64 + mi * 32 + lane) for lane in range(32)}
                    assert len(banks) == 32


@pytest.mark.parametrize("C,Opad,o_tile0", [(2, 128, 96), (6, 128, 32), (512, 512, 480)])
def test_dma_chunks_are_aligned_and_fetch_the_right_rows(C, Opad, o_tile0):
    E = _emul()
    B, b0 = 256, 128
    for p in range(4):
        for pair in sorted({0, C // 2 - 1}):
            dst_w, dst_e = set(), set()
            for copy in range(E.NQ):
                for lane in range(64):
                    src, dst = E.dma_w_source(copy, lane, p, pair, C, Opad, o_tile0)
                    assert src % 4 == 0 and dst % 4 == 0                   # 16-byte chunks on both sides
                    row, col = divmod(dst, E.TO)
                    o_l, q = E.col_inv(col)
                    assert E.col_of(o_l, q) == col and o_l % 4 == 0
                    want = E.wp_index(E.tap_of(q, p), 2 * pair + row // E.P, row % E.P, o_tile0 + o_l, C, Opad)
                    assert src == want and src + 3 < (9 * C // 2) * E.KC * Opad
                    dst_w.add(dst)
                    src, dst = E.dma_e_source(copy, lane, p, pair, B, b0)
                    assert src % 4 == 0 and dst % 4 == 0
                    row, col = divmod(dst, E.TP)
                    assert src == (((2 * pair + row // E.P) * E.HW + p) * E.P + row % E.P) * B + b0 + col
                    dst_e.add(dst)
            assert dst_w == set(range(0, E.KC * E.TO, 4)) and dst_e == set(range(0, E.KC * E.TP, 4))
