"""What the tests of the persistent packed weights share (ops._PACKED, kan_pack_weights_cached).

fingerprint_ref restates the content fingerprint from the description of kan_pack_weights_cached in include/kanconv.h, in numpy
integers; fingerprint_ref_torch is the same in torch int64 for the one case too large for a CPU round trip; ring_totals reads a slot
of the 3-slot ring the way the pack kernels compare it.  PACK_CASES holds layers for which kan_pack_cacheable is 1 (checked on the CPU
by tests/test_pack_cache.py), at least one per forward route class the cache serves.  tests/test_pack_cache.py uses the host half,
tests/test_gpu_pack_cache.py all of it."""
import ctypes

import numpy as np
import torch

from route_cells import ROUTE_CASES, case_structs, row

M32 = 0xFFFFFFFF
FP_LANES = 64                                          # 64-bit words per ring slot: KAN_FP_WORDS / 3 (include/kanconv.h)


# ------------------------------------------------------------------------------------------------ the fingerprint, restated
def _sampled(n, stride):
    """Element indices of one tensor that enter the fingerprint: every `stride`-th WHOLE group of four, from group 0, plus the ragged
    tail (the n % 4 elements behind the last whole group)."""
    groups = np.arange(0, n // 4, stride, dtype=np.int64)
    whole = (groups[:, None] * 4 + np.arange(4, dtype=np.int64)[None, :]).reshape(-1)
    return np.concatenate([whole, np.arange(n // 4 * 4, n, dtype=np.int64)])


def fingerprint_ref(base_bits, basis_bits, stride=1):
    """(h1, h2) of kan_pack_weights_cached: h1 = sum bits_i * (2 i + 1), h2 = sum rotl(bits_i, i mod 32), both mod 2^32, i = the
    element's position in (base elements, then basis elements); `base_bits` None or empty: no base branch, the basis starts at 0."""
    h1 = h2 = np.uint64(0)
    pos0 = 0
    with np.errstate(over="ignore"):
        for bits in (base_bits, basis_bits):
            if bits is None or len(bits) == 0:
                continue
            bits = np.ascontiguousarray(bits).reshape(-1).view(np.uint32).astype(np.uint64)
            idx = _sampled(len(bits), stride)
            w, p = bits[idx], (idx + pos0).astype(np.uint64)
            h1 = h1 + np.sum(w * ((np.uint64(2) * p + np.uint64(1)) & np.uint64(M32)), dtype=np.uint64)     # wraps mod 2^64: keeps mod 2^32
            s = p & np.uint64(31)
            h2 = h2 + np.sum(((w << s) | (w >> (np.uint64(32) - s))) & np.uint64(M32), dtype=np.uint64)     # s = 0: w >> 32 = 0
            pos0 += len(bits)
    return int(h1) & M32, int(h2) & M32


def fingerprint_ref_torch(base, basis, stride=1):
    """fingerprint_ref on fp32 (or int32) torch tensors of any device, in int64.  Every term is cut to 32 bits before the sum and a tensor
    has fewer than 2^31 elements, so no sum leaves 63 bits; a wrap would keep the value mod 2^32 all the same."""
    h1 = h2 = 0
    pos0 = 0
    for t in (base, basis):
        if t is None or t.numel() == 0:
            continue
        bits = t.reshape(-1).view(torch.int32).to(torch.int64) & M32
        n = bits.numel()
        groups = torch.arange(0, n // 4, stride, device=t.device, dtype=torch.int64)
        idx = torch.cat([(groups[:, None] * 4 + torch.arange(4, device=t.device, dtype=torch.int64)[None, :]).reshape(-1),
                         torch.arange(n // 4 * 4, n, device=t.device, dtype=torch.int64)])
        w, p = bits[idx], idx + pos0
        h1 += int((((w * ((2 * p + 1) & M32)) & M32).sum()).item())                 # w * m < 2^64 wraps mod 2^64: the low 32 bits hold
        s = p & 31
        h2 += int(((((w << s) | (w >> (32 - s))) & M32).sum()).item())
        pos0 += n
    return h1 & M32, h2 & M32


def ring_totals(ring, slot):
    """(h1, h2) held by slot `slot` of a fingerprint ring (KAN_FP_WORDS 64-bit words, tensor or array): the low and the high 32-bit
    halves of the slot's 64 words, each summed mod 2^32."""
    words = ring.detach().cpu().numpy() if isinstance(ring, torch.Tensor) else np.asarray(ring)
    words = words.reshape(-1).view(np.uint64)[slot * FP_LANES:(slot + 1) * FP_LANES]
    return int(np.sum(words & np.uint64(M32), dtype=np.uint64)) & M32, int(np.sum(words >> np.uint64(32), dtype=np.uint64)) & M32


# ------------------------------------------------------------------------------------------------ the case table
def _route_row(key, layer, shape):
    """The G == 1 row of route_cells.ROUTE_CASES with this key, layer and conv shape."""
    hits = [c for c in ROUTE_CASES if c["key"] == tuple(key.split()) and c["layer"] == layer and c["shape"] == shape and c["G"] == 1]
    assert len(hits) == 1, (key, layer, shape, len(hits))
    return dict(hits[0])


# name -> row (route_cells.row).  CLASS_ROWS: one row per forward route class the cache serves, taken from the route matrix; RAGGED_ROWS:
# element counts that are no multiple of four and layers of a handful of weights (all on the band kernels), with and without a base branch.
CLASS_ROWS = {
    "band_1m": _route_row("FAST_BSPLINE_GELU BAND TAP EXPANDED", "kan_gelu", "3x3"),               # 128 -> 96, 3x3: 995 328 elements, 122 blocks
    "halo": _route_row("FAST_BSPLINE_SILU HALO TAP HALO", "kan_silu", "3x3"),
    "halo_cheby": _route_row("FAST_CHEBY4 HALO TAP TAP-PM", "cheby_d3", "3x3"),                     # no base branch
    "halo_rb": _route_row("FAST_BSPLINE_GELU HALO+RB TAP HALO", "kan_gelu", "3x3"),
    "halo_rb_poly": _route_row("FAST_POLY4 HALO+RB TAP TAP", "bersnstein_d3", "3x3"),
    "expanded": _route_row("FAST_BSPLINE_GELU EXPANDED TAP-PM TAP-PM", "kan_gelu", "3x3"),
    "tap_pm": _route_row("FAST_BSPLINE_SILU TAP-PM TAP-PM EXPANDED", "kan_silu", "3x3"),
    "tap": _route_row("FAST_BSPLINE_SILU TAP TAP-PM EXPANDED", "kan_silu", "1x1p1"),
}
RAGGED_ROWS = {
    "cheby_nb10": row("FAST_CHEBY5 BAND TAP BAND", "cheby_d4", "1x1", 1, 2, 1, 2),                  # na = 0, nb = 10
    "cheby_nb270": row("FAST_CHEBY5 BAND TAP BAND", "cheby_d4", "3x3", 2, 2, 3, 4),                 # na = 0, nb = 270
    "kan_na2": row("FAST_BSPLINE_SILU BAND TAP BAND", "kan_silu", "1x1", 2, 2, 1, 4),               # na = 2, nb = 16
    "kan_na594": row("FAST_BSPLINE_SILU BAND TAP BAND", "kan_silu", "3x3", 2, 2, 33, 4),            # na = 594, nb = 4752
    "lucas_na126": row("FAST_POLY4 BAND TAP TAP", "lucas_d3", "3x3", 2, 2, 7, 4),                   # na = 126, nb = 504
}
# 1024 -> 512, 3x3: 4 718 592 + 37 748 736 elements.  The fingerprint's grid is capped at 4096 blocks of 256 lanes with 8 groups of four in
# flight each, so a tensor of more than 33 554 432 elements makes its grid-stride loop iterate; nothing else here or in the models does.
BIG_ROW = "big_42m"
PACK_CASES = dict(CLASS_ROWS, **RAGGED_ROWS)
PACK_CASES[BIG_ROW] = row("FAST_BSPLINE_SILU HALO TAP TAP", "kan_silu", "3x3", 2, 1024, 512, 8)
FWD_CLASSES = ("BAND", "HALO", "HALO+RB", "EXPANDED", "TAP-PM", "TAP")
LOOP_ELEMS = 4096 * 256 * 8 * 4                       # elements of one tensor one sweep of the fingerprint's grid covers


def counts(g, b):
    """(na, nb): elements of the base and of the basis weights of one group."""
    T = g.kh * g.kw
    return (g.O * g.C * T if b.act != -1 else 0), g.O * g.C * b.n_basis * T


def structs(name):
    """(KanGeom, KanBasis, KanPlan) of a PACK_CASES row."""
    return case_structs(PACK_CASES[name])


def cacheable(lib, g, b):
    return int(lib.kan_pack_cacheable(ctypes.byref(g), ctypes.byref(b)))
