"""CPU half of the packed-weight cache checks (tests/pack_cells.py; the GPU half is tests/test_gpu_pack_cache.py).

(1) the fingerprint reference checks itself on inputs small enough to work out by hand; (2) kan_pack_cacheable, restated from the public plan,
agrees with the library over a grid of geometries and is 0 wherever the packed forward layout has rows no weight maps to (those need the clear
that a cached pack cannot skip), and every PACK_CASES row is what its name says; (3) what each of the two sums can and cannot see, pinned with
the reference (DESIGN.md section 2 states the same in words)."""
import numpy as np
import pytest
import torch

from golden.make_plan_snapshot import basis_specs, geom, make_structs
from pack_cells import (BIG_ROW, CLASS_ROWS, FWD_CLASSES, LOOP_ELEMS, M32, PACK_CASES, RAGGED_ROWS, cacheable, counts, fingerprint_ref,
                        fingerprint_ref_torch, ring_totals, structs)
from route_cells import dw_direct, plan_of, route_key


def _u32(values):
    return np.array(values, dtype=np.uint32)


def _plain(bits, positions):
    """The two sums over explicit (bits, position) pairs, in Python integers."""
    h1 = sum(int(w) * (2 * p + 1) for w, p in zip(bits, positions)) & M32
    h2 = sum(((int(w) << (p & 31)) | (int(w) >> (32 - (p & 31)))) & M32 for w, p in zip(bits, positions)) & M32
    return h1, h2


# ------------------------------------------------------------------------------------------------ (1) the reference checks itself
def test_reference_closed_forms():
    assert fingerprint_ref(None, _u32([1] * 5)) == (25, 31)                          # sum of the first five odd numbers; 1 + 2 + 4 + 8 + 16
    assert fingerprint_ref(_u32([1, 1]), _u32([1, 1, 1])) == (25, 31)                # positions run on from the base into the basis
    assert fingerprint_ref(_u32([]), _u32([1] * 5)) == (25, 31)                      # an absent base branch contributes and shifts nothing
    assert fingerprint_ref(_u32([0]), _u32([0x80000000])) == (0x80000000, 1)         # position 1: 3 * 2^31 mod 2^32; the top bit rotates into bit 0
    assert fingerprint_ref(None, _u32([0] * 33 + [0x80000000])) == ((67 << 31) & M32, 1)      # position 33 rotates by 33 mod 32 = 1
    assert fingerprint_ref(None, _u32([M32] * 4)) == ((-16) & M32, (4 * M32) & M32)  # both sums wrap mod 2^32
    assert fingerprint_ref(None, np.array([-0.0], dtype=np.float32)) == (0x80000000, 0x80000000)      # bits, not values: -0.0 is not 0.0


def test_reference_stride_one_is_the_plain_sum_and_strides_sample_whole_groups():
    rng = np.random.default_rng(5)
    for na, nb in ((0, 37), (7, 22), (2, 16), (13, 3), (4, 4)):
        a, b = rng.integers(0, 2 ** 32, na, dtype=np.uint32), rng.integers(0, 2 ** 32, nb, dtype=np.uint32)
        assert fingerprint_ref(a, b) == _plain(list(a) + list(b), range(na + nb)), (na, nb)
        for stride in (2, 3, 7):
            pairs = []
            for t, n, base in ((a, na, 0), (b, nb, na)):
                keep = [i for i in range(n) if (i < n // 4 * 4 and (i // 4) % stride == 0) or i >= n // 4 * 4]
                pairs += [(t[i], base + i) for i in keep]
            assert fingerprint_ref(a, b, stride) == _plain([w for w, _ in pairs], [p for _, p in pairs]), (na, nb, stride)
    b = rng.integers(0, 2 ** 32, 22, dtype=np.uint32)                                 # 5 whole groups + 2: stride 2 keeps groups 0, 2, 4 and the tail
    assert fingerprint_ref(None, b, 2) == _plain([b[i] for i in (0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 20, 21)], (0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 20, 21))


def test_torch_twin_and_ring_totals():
    rng = np.random.default_rng(6)
    for na, nb in ((0, 10), (2, 16), (594, 4752), (126, 504), (0, 70001)):
        a, b = rng.integers(0, 2 ** 32, na, dtype=np.uint32), rng.integers(0, 2 ** 32, nb, dtype=np.uint32)
        ta, tb = torch.from_numpy(a.view(np.int32).copy()), torch.from_numpy(b.view(np.int32).copy())
        for stride in (1, 2, 3, 7):
            assert fingerprint_ref_torch(ta if na else None, tb, stride) == fingerprint_ref(a, b, stride), (na, nb, stride)
        assert fingerprint_ref_torch(ta.view(torch.float32), tb.view(torch.float32)) == fingerprint_ref(a, b)      # fp32 tensors are read as their bits
    ring = np.zeros(192, dtype=np.uint64)
    ring[64 + 3] = (np.uint64(1) << np.uint64(32)) | np.uint64(M32)                   # slot 1: low halves 2^32 - 1 twice, high halves 1 and 7
    ring[64 + 63] = (np.uint64(7) << np.uint64(32)) | np.uint64(M32)
    ring[128] = np.uint64(5)
    assert ring_totals(ring, 0) == (0, 0)
    assert ring_totals(ring, 1) == (M32 - 1, 8)                                      # no carry from the low sum into the high one
    assert ring_totals(torch.from_numpy(ring.view(np.int64)), 2) == (5, 0)


# ------------------------------------------------------------------------------------------------ (2) where cached packing is offered
def cacheable_ref(g, b, p):
    """kan_pack_cacheable from the public plan: one group, not the depthwise direct route, element positions that fit 32 bits (counted with a
    base branch whether or not there is one), and no row of the packed forward layout that needs clearing -- a step (KC rows) holds IPC whole
    items of P planes with no pad row, and the last step is full: of channels in band order, of (channel, tap) items otherwise."""
    T = g.kh * g.kw
    if p is None or max(g.groups, 1) != 1 or dw_direct(g, b) or g.O * g.C * (b.n_basis + 1) * T >= 2 ** 31:
        return 0
    items = g.C if p.fwd_band else g.C * T
    return int(p.KC == p.IPC * p.P and items % p.IPC == 0)


def _grid():
    shapes = {"3x3": dict(k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1)), "1x1": dict(k=(1, 1), s=(1, 1), p=(0, 0), d=(1, 1)),
              "s2": dict(k=(3, 3), s=(2, 2), p=(1, 1), d=(1, 1)), "5x5s2": dict(k=(5, 5), s=(2, 2), p=(2, 2), d=(1, 1)),
              "1x1p1": dict(k=(1, 1), s=(1, 1), p=(1, 1), d=(1, 1)), "1x3": dict(k=(1, 3), s=(1, 1), p=(0, 1), d=(1, 1))}
    for name, bl in sorted(basis_specs().items()):
        for sk in shapes.values():
            for hw in (2, 3, 4, 8, 16, 32):
                for B in (1, 17, 128):
                    for C_ in (1, 2, 3, 5, 16, 128):
                        for O in (1, 2, 33, 96, 128, 256):
                            for G in ((1, 2) if C_ <= 2 else (1,)):
                                yield name, geom(B, C_, hw, hw, O, G=G, **sk), bl
        for n in (15360, 15488):                      # 1x1, n x n channels: n^2 (n_basis + 1) on either side of 2^31 for the 8-plane bases
            yield name, geom(1, n, 2, 2, n, k=(1, 1), p=(0, 0)), bl


def test_pack_cacheable_restated_over_a_grid():
    import convkan_amd
    lib = convkan_amd._lib.load()
    seen = {0: 0, 1: 0}
    over_bound = unwritten = 0
    classes = set()
    for name, gl, bl in _grid():
        g, b = make_structs(gl, bl)
        p = plan_of(g, b)
        got, want = cacheable(lib, g, b), cacheable_ref(g, b, p)
        assert got == want, f"{name} {gl}: kan_pack_cacheable = {got}, restated {want}"
        seen[got] += 1
        if p is None:
            continue
        T = g.kh * g.kw
        over_bound += g.O * g.C * (b.n_basis + 1) * T >= 2 ** 31
        if p.Kpad != g.C * T * p.P:
            # C * T * P weights of an output fill C * T * P distinct rows of wp: with more rows than that, some are written by nobody and
            # kan_pack_weights clears before it packs -- a clear the cached call cannot make conditional
            unwritten += 1
            assert got == 0, f"{name} {gl}: cached packing offered although wp has {p.Kpad} rows for {g.C * T * p.P} weights per output"
        if got:
            classes.add(route_key(g, b, p)[1])
    assert seen[0] > 1000 and seen[1] > 1000 and over_bound >= 2 and unwritten > 1000, (seen, over_bound, unwritten)
    assert classes == set(FWD_CLASSES), classes       # the grid reaches every forward route class the cache serves, and only those


@pytest.mark.parametrize("name", list(PACK_CASES))
def test_pack_case_is_cacheable_and_plans_to_its_key(name):
    import convkan_amd
    g, b, p = structs(name)
    assert cacheable(convkan_amd._lib.load(), g, b) == 1 and cacheable_ref(g, b, p) == 1
    assert route_key(g, b, p) == PACK_CASES[name]["key"], route_key(g, b, p)
    assert g.groups == 1 and b.kind != convkan_amd._lib.BASIS_RELU                     # what ops._pack caches: one group, no phase table


def test_pack_cases_cover_what_they_are_for():
    import convkan_amd
    assert {c["key"][1] for c in CLASS_ROWS.values()} == set(FWD_CLASSES)
    assert {n: counts(*structs(n)[:2]) for n in RAGGED_ROWS} == {"cheby_nb10": (0, 10), "cheby_nb270": (0, 270), "kan_na2": (2, 16),
                                                                 "kan_na594": (594, 4752), "lucas_na126": (126, 504)}
    assert any(counts(*structs(n)[:2])[0] == 0 for n in CLASS_ROWS)                   # a layer without a base branch on the MFMA routes too
    na, nb = counts(*structs("band_1m")[:2])
    assert ((na + 3) // 4 + (nb + 3) // 4 + 2047) // 2048 > 64                        # more blocks than a ring slot has words
    for n in PACK_CASES:
        na, nb = counts(*structs(n)[:2])
        assert (nb > LOOP_ELEMS and na + nb < 2 ** 31) if n == BIG_ROW else na + nb < 10_000_000, (n, na, nb)
    assert convkan_amd._lib.KAN_FP_WORDS == 192


# ------------------------------------------------------------------------------------------------ (3) what each sum sees
def _split(n, seed):
    """n random weights as a ragged base tensor (n // 4 + 2 elements) and the basis tensor behind it."""
    w = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    na = n // 4 + 2
    return w[:na].copy(), w[na:].copy()


@pytest.mark.parametrize("n", [96, 4096, 65568])
def test_the_two_sums_are_complementary(n):
    a, b = _split(n, n)
    h1, h2 = fingerprint_ref(a, b)
    # doubling every weight adds 2^23 to every word: h1 moves by 2^23 * sum (2 i + 1) = 2^23 n^2, which is 0 mod 2^32 whenever 32 | n;
    # negating adds 2^31 to every word: 2^31 n^2, 0 whenever n is even.  Only the rotated sum sees either.
    for name, (a2, b2) in (("mul 2", (a * 2, b * 2)), ("negation", (-a, -b))):
        g1, g2 = fingerprint_ref(a2, b2)
        assert g1 == h1, f"{name}, n = {n}: h1 moved"
        assert g2 != h2, f"{name}, n = {n}: h2 did not move"
    assert fingerprint_ref(None, np.concatenate([a, b]) * 2)[0] == fingerprint_ref(None, np.concatenate([a, b]))[0]      # one tensor: the same
    # the odd multiplier of h1 is invertible mod 2^32: one changed element always moves it, wherever it is
    for name, t, i in (("first", 0, 0), ("tail of the base", 0, len(a) - 1), ("last", 1, len(b) - 1)):
        pair = [a.copy(), b.copy()]
        pair[t].view(np.uint32)[i] += 1                                              # 1 ulp
        assert fingerprint_ref(*pair)[0] != h1, f"1 ulp on the {name} element, n = {n}: h1 did not move"
        if t == 0:                                                                   # group 0 and the ragged tail are in every sample
            assert fingerprint_ref(*pair, stride=3)[0] != fingerprint_ref(a, b, stride=3)[0], f"stride 3, {name}"
    if n > 32768:
        # the joint blind spot: two weights whose low 16 bits are zero (every bf16 value), 32768 positions apart, swapped.  h1 moves by
        # (x - y) * 2 * 32768 = a multiple of 2^32; both rotate by the same count, so h2 keeps its terms.
        w = np.concatenate([a, b])
        bits = w.view(np.uint32)
        i, j = 1234, 1234 + 32768
        bits[i] &= 0xFFFF0000
        bits[j] &= 0xFFFF0000
        assert bits[i] != bits[j]
        sw = w.copy()
        sw[i], sw[j] = w[j], w[i]
        assert fingerprint_ref(None, sw) == fingerprint_ref(None, w), "the bf16 swap at distance 32768 is seen"
        for di, dj, what in ((0, 32767, "another distance"), (1, 32769, "fp32 values")):      # the blind spot is no wider than stated
            sw = w.copy()
            sw[i + di], sw[i + dj] = w[i + dj], w[i + di]
            assert fingerprint_ref(None, sw)[0] != fingerprint_ref(None, w)[0], what
