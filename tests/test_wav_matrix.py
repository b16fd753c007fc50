"""CPU: the Wav-KAN cell matrix (tests/wav_cells.py) stays in step with `kan_wav_route`, the function the four kan_wav_* entry
points dispatch from.

(a) every WAV_CASES row routes to exactly its three declared keys (the `refuse` row: the forward does not fit), so a moved threshold
    fails here instead of silently leaving a kernel path without its fp64 check;
(b) every key the route reaches over the committed grid of geometries (wav_cells.sweep) has a row, and every row's key is reached
    by the grid; every kernel x wavelet pair has a row; both sides of every switch point are there, at exactly the neighbouring
    sizes (9 | 10, 18 | 19 and 27 | 28 taps; the widest 2-row plane whose 3x3 band fits LDS and the next width; a 16 x 16 tile's
    region of at most / just above 1792 cells); the edge rows the table is specified to hold are there; and every row is needed:
    the table without it lacks one of these -- so deleting any row fails here;
(c) kan_wav_param_workspace == chunks * O * C * (T + 2) for every row;
(d) the reference is pinned independently of the oracle: on two tiny cases (one with every geometry parameter asymmetric) its fp64
    forward equals a literal Python loop over (b, o, ho, wo, c, r, t) of the formula in include/kanconv.h;
(e) every Meyer row keeps the share of redrawn input elements under wav_cells.REDRAW_CAP."""
import ctypes
import functools
import math

import pytest
import torch

import convkan_amd as K
from wav_cells import (BI, REDRAW_CAP, WAV_CASES, WAVELETS, _draw, _pair, case_geom, case_id, case_ids, case_keys, redraw_share, route_of, row,
                       run_reference, sweep, geom_of)

REGION_CELLS = 1792        # kan_wav_route's cap on a forward tile's input region
NEAR = 64                  # "just under / just over": within this many cells


@pytest.fixture(scope="module", autouse=True)
def _library():
    K.build_library()


def T_of(c):
    return _pair(c["k"])[0] * _pair(c["k"])[1]


def first_region(c):
    """Input region of the forward's first tile (min(Wo, 16) wide, up to 256 pixels), before any shrinking."""
    g = case_geom(c)
    tw = min(g.Wo, 16)
    th = min(g.Ho, 256 // tw)
    return ((th - 1) * g.sh + (g.kh - 1) * g.dh + 1) * ((tw - 1) * g.sw + (g.kw - 1) * g.dw + 1)


@functools.lru_cache(maxsize=1)
def band_limit():
    """W: the widest 2-row plane on which a 3x3 layer still takes the tiled parameter kernel (W + 1 takes the per-pixel one)."""
    kernel = [route_of(geom_of(1, 3, 5, 2, W, 3, 1, 1, 1)).params_kernel for W in range(1, 400)]
    flips = [W for W in range(1, 399) if kernel[W - 1] != kernel[W]]
    assert len(flips) == 1 and kernel[flips[0] - 1] == 0, flips
    return flips[0]


def kernels_of(c):
    """The six kernels' names a row runs."""
    return {"fwd", c["bi"][3:], c["par"].split("-")[1]}


def shortfalls(cases):
    """What the table `cases` lacks, as a list of sentences (empty: complete)."""
    out = []
    live = [c for c in cases if c["kind"] != "refuse"]
    have = {c[s] for c in live for s in ("fwd", "bi", "par")}
    reach = set(sweep())
    out += [f"reachable key without a row: {k}" for k in sorted(reach - have)]
    out += [f"row key no grid launch reaches: {k}" for k in sorted(have - reach)]
    for kern in ("fwd",) + BI + ("TILED", "PIXEL"):
        for wt in WAVELETS:
            if not any(kern in kernels_of(c) and c["wavelet"] == wt for c in live):
                out.append(f"no row runs kernel {kern} with wavelet {wt}")
    asym = lambda c, n: _pair(c[n])[0] != _pair(c[n])[1]
    reach_h = lambda c: (_pair(c["k"])[0] - 1) * _pair(c["d"])[0]
    named = {
        "9 taps": lambda c: T_of(c) == 9, "10 taps": lambda c: T_of(c) == 10, "18 taps": lambda c: T_of(c) == 18, "19 taps": lambda c: T_of(c) == 19,
        "27 taps": lambda c: T_of(c) == 27, "28 taps": lambda c: T_of(c) == 28,
        f"a 3x3 layer on the 2 x {band_limit()} plane (tiled)": lambda c: (c["H"], c["W"], c["k"], c["d"]) == (2, band_limit(), 3, 1) and "TILED" in c["par"],
        f"a 3x3 layer on the 2 x {band_limit() + 1} plane (per-pixel)": lambda c: (c["H"], c["W"], c["k"], c["d"]) == (2, band_limit() + 1, 3, 1) and "PIXEL" in c["par"],
        "a first tile region just under 1792 cells, not shrunk": lambda c: REGION_CELLS - NEAR < first_region(c) <= REGION_CELLS and "shrunk" not in c["fwd"],
        "a first tile region just over 1792 cells, shrunk": lambda c: REGION_CELLS < first_region(c) <= REGION_CELLS + NEAR and "shrunk" in c["fwd"],
        "kernel, stride, padding and dilation all asymmetric": lambda c: all(asym(c, n) for n in "kspd"),
        "padding beyond the kernel's reach": lambda c: _pair(c["p"])[0] > reach_h(c) > 0,
        "padding 0": lambda c: _pair(c["p"]) == (0, 0),
        "Shannon with one channel": lambda c: c["wavelet"] == "shannon" and c["C"] == 1,
        "Shannon with two channels": lambda c: c["wavelet"] == "shannon" and c["C"] == 2,
        "B H W no multiple of 256": lambda c: (c["B"] * c["H"] * c["W"]) % 256 != 0,
        "negative scales": lambda c: c["neg"], "inputs times 3": lambda c: c["x3"],
    }
    for n, what in zip("kspd", ("kernel", "stride", "padding", "dilation")):
        named[f"only the {what} asymmetric"] = lambda c, n=n: asym(c, n) and not any(asym(c, m) for m in "kspd" if m != n)
    # every kernel indexes with the h and the w member of each pair separately: each pair differs on every kernel (stride 1 x 1 defines STRIDE1)
    for kern in ("fwd",) + BI + ("TILED", "PIXEL"):
        for n, what in zip("spd", ("stride", "padding", "dilation")):
            if (kern, n) != ("STRIDE1", "s"):
                named[f"an asymmetric {what} on kernel {kern}"] = lambda c, kern=kern, n=n: asym(c, n) and kern in kernels_of(c)
    for O in (1, 3, 5, 17):
        named[f"O = {O}"] = lambda c, O=O: c["O"] == O
    for Cn in (1, 2, 5, 17):
        named[f"C = {Cn}"] = lambda c, Cn=Cn: c["C"] == Cn
    for kern in ("fwd",) + BI + ("TILED", "PIXEL"):
        named[f"a batch-strided row on kernel {kern}"] = lambda c, kern=kern: c["kind"] == "bstride" and kern in kernels_of(c)
    out += [f"no row with {what}" for what, pred in named.items() if not any(pred(c) for c in live)]
    if not any(c["kind"] == "refuse" for c in cases):
        out.append("no row the forward refuses")
    return out


@pytest.mark.parametrize("case", WAV_CASES, ids=case_ids(WAV_CASES))
def test_wav_case_routes_to_its_keys(case):
    got = case_keys(case)
    assert got == (case["fwd"], case["bi"], case["par"]), f"row {case_id(case)} now routes to {got}"
    r = route_of(case_geom(case))
    assert (r.fwd_fits == 0) == (case["kind"] == "refuse")
    assert r.fwd_lds_bytes <= 64 * 1024 or not r.fwd_fits
    assert r.lds_bytes <= 56 * 1024


def test_switch_points_are_where_the_rows_stand():
    """The tap counts at which the route changes kernel or pass count, from the route itself."""
    taps = lambda n, s: route_of(geom_of(1, 3, 5, 4, 64, (1, n), s, (0, n), 1))
    assert [n for n in range(1, 40) if taps(n, 2).bwd_input_kernel != taps(n + 1, 2).bwd_input_kernel] == [9]
    assert (taps(9, 2).bwd_input_kernel, taps(10, 2).bwd_input_kernel, taps(10, 1).bwd_input_kernel) == (0, 2, 1)
    assert [n for n in range(1, 40) if taps(n, 1).passes != taps(n + 1, 1).passes] == [9, 18, 27, 36]
    assert 200 < band_limit() < 256


def test_table_is_complete():
    lacks = shortfalls(WAV_CASES)
    assert not lacks, "\n".join(lacks)


@pytest.mark.parametrize("idx", range(len(WAV_CASES)), ids=case_ids(WAV_CASES))
def test_every_row_is_needed(idx):
    """The table without this row lacks something: no row can be deleted unnoticed."""
    assert shortfalls(WAV_CASES[:idx] + WAV_CASES[idx + 1:]), f"nothing asks for row {case_id(WAV_CASES[idx])}"


@pytest.mark.parametrize("case", WAV_CASES, ids=case_ids(WAV_CASES))
def test_workspace_matches_chunks(case):
    from convkan_amd import _lib as L
    g = case_geom(case)
    r = route_of(g)
    assert L.load().kan_wav_param_workspace(ctypes.byref(g)) == r.chunks * case["O"] * case["C"] * (T_of(case) + 2)
    if r.params_kernel == L.WAV_PAR_TILED:
        assert r.chunks == -(-r.items // r.items_per_chunk) and r.items == -(-g.B // r.NI) * r.bands and r.px_per_chunk == 0
    else:
        assert r.chunks * r.px_per_chunk >= g.B * g.H * g.W and r.BH == r.items == r.lds_bytes == 0
    assert r.passes == -(-T_of(case) // 9)


# ------------------------------------------------------------------------------------------ the reference, pinned
def _psi_literal(u, kind, c, Cn):
    """The five wavelets (the comment at the top of csrc/wavkan.inc), on one float."""
    if kind == "mexican_hat":
        return 2 / (math.sqrt(3) * math.pi ** 0.25) * (u * u - 1) * math.exp(-u * u / 2)
    if kind == "morlet":
        return math.exp(-u * u / 2) * math.cos(5 * u)
    if kind == "dog":
        return -u * math.exp(-u * u / 2)
    if kind == "meyer":
        v = abs(u)
        t = 2 * v - 1
        aux = 1.0 if v <= 0.5 else 0.0 if v >= 1 else math.cos(math.pi / 2 * t ** 4 * (35 - 84 * t + 70 * t * t - 20 * t ** 3))
        return math.sin(math.pi * v) * aux
    window = 1.0 if Cn == 1 else 0.54 - 0.46 * math.cos(2 * math.pi * c / (Cn - 1))
    return (math.sin(u) / u if u != 0 else 1.0) * window


TINY = [row("", "", "", 2, 2, 3, 5, 4, (2, 3), (2, 1), (1, 2), (1, 2), wavelet="meyer", neg=True),
        row("", "", "", 1, 3, 2, 4, 4, 3, 1, 1, 1, wavelet="shannon"),
        row("", "", "", 1, 2, 2, 3, 5, (3, 1), 1, 3, 1, wavelet="mexican_hat"),
        row("", "", "", 1, 1, 2, 4, 3, 2, 2, 0, 1, wavelet="morlet"),
        row("", "", "", 1, 2, 1, 3, 3, (1, 2), 1, 1, 2, wavelet="dog", x3=True)]


@pytest.mark.parametrize("case", TINY, ids=case_ids(TINY))
def test_reference_matches_literal_loop(case):
    _, x, scale, trans, w, du = _draw(case, 7)
    ref = run_reference(case, (x, scale, trans, w, du), torch.float64)
    g = case_geom(case)
    want = torch.zeros(g.B, g.O, g.Ho, g.Wo, dtype=torch.float64)
    for b in range(g.B):
        for o in range(g.O):
            for ho in range(g.Ho):
                for wo in range(g.Wo):
                    acc = 0.0
                    for c in range(g.C):
                        for r in range(g.kh):
                            for t in range(g.kw):
                                hi, wi = ho * g.sh - g.ph + r * g.dh, wo * g.sw - g.pw + t * g.dw
                                if 0 <= hi < g.H and 0 <= wi < g.W:          # (zero padding applies to the wavelet values)
                                    acc += float(w[o, c, r, t]) * _psi_literal((float(x[b, c, hi, wi]) - float(trans[o, c])) / float(scale[o, c]),
                                                                              case["wavelet"], c, g.C)
                    want[b, o, ho, wo] = acc
    assert ref["u"].shape == want.shape and float(want.abs().max()) > 0
    assert float((ref["u"] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert ref["dx"].shape == x.shape and ref["dw"].shape == w.shape and ref["dscale"].shape == ref["dtrans"].shape == scale.shape


@pytest.mark.parametrize("case", [c for c in WAV_CASES if c["wavelet"] == "meyer" and c["kind"] != "refuse"], ids=case_id)
def test_meyer_redraw_share_under_cap(case):
    share = redraw_share(case)
    print(f"[wav redraw] {case_id(case)}: {share:.2e} of the input elements drawn again")
    assert share <= REDRAW_CAP, f"{case_id(case)}: {share:.3%} of the inputs were redrawn (cap {REDRAW_CAP:.0%}): give the row another seed"
