"""The cell matrix of the Wav-KAN wavelet stage (csrc/wavkan.inc): which kernels `kan_wav_route` picks for a geometry and with what
launch shapes, one row per reachable cell of each of its three stages and per side of every switch point, and the plain-torch
reference the rows are judged against.

A cell is what `kan_wav_route` (the function kan_wav_fwd / _bwd_input / _bwd_params / _param_workspace dispatch from) decides.
`wav_key` spells a route as three strings, one per stage:
  forward     fwd-{multi|single}[-shrunk][-cut][-grid][-ragged]     multi: several images per workgroup (NIMG > 1); shrunk: the tile was
              halved to get its input region under 1792 cells; cut: that cap lowered NIMG; grid: more than one tile per image; ragged:
              Ho % TH, Wo % TW or B % NIMG is non-zero (threads or images past the end).  fwd-refuse: the tile does not fit 64 KB.
  bwd-input   bi-{TAPS9|STRIDE1|STRIDED}
  bwd-params  par-TILED-p{passes}[-chunked]-items{1|2}[-raggedband][-raggedimg]   chunked: more than one partial-sum slab; items2: a
              workgroup loops over several work items (the LDS bands are restaged); raggedband: H % BH; raggedimg: B % NI
              par-PIXEL-p{passes}[-chunked][-raggedchunk]                         raggedchunk: B H W % px_per_chunk
tests/test_wav_matrix.py keeps the table complete on the CPU (against `sweep()`, the committed grid of geometries);
tests/test_gpu_wav_matrix.py runs every row against `reference(case, torch.float64)`.

Inputs: x ~ N(0, 1) (times 3 on the `x3` rows), |scale| ~ U[0.5, 1.6] (negative on a quarter of the (o, c) pairs of the `neg` rows),
translation ~ N(0, 0.5), taps ~ N(0, 1) / sqrt(C kh kw), du ~ N(0, 1).  Conditioning, from the fp64 reference alone: Meyer's
derivative jumps at u = 0 (sign(u)), so on Meyer rows an input element with |u| < 1e-5 for some output is drawn again before
the row is frozen; at most REDRAW_CAP of a row's input elements may be redrawn (a row over the cap gets another seed).  No other
wavelet has a kink (the kernels' Shannon series switch at |u| = 0.3 is smooth)."""
import ctypes
import functools
import math

import torch
import torch.nn.functional as F

WAVELETS = ("mexican_hat", "morlet", "dog", "meyer", "shannon")          # index = KAN_WAV_*
BI = ("TAPS9", "STRIDE1", "STRIDED")
MEYER_KINK = 1e-5
REDRAW_CAP = 0.01
CHUNK_ELEMS = 1 << 23            # wavelet values [b, O, C, H, W] evaluated at once by the reference (64 MB in fp64, a few times that with the graph)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def geom_of(B, C, O, H, W, k, s=1, p=0, d=1, wavelet=0, xbs=None, ubs=None):
    """KanWavGeom of a dense launch (ops._WavStage._geom), or with the batch strides given; None when the output is empty."""
    from convkan_amd import _lib as L
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(k), _pair(s), _pair(p), _pair(d)
    Ho, Wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if Ho < 1 or Wo < 1:
        return None
    return L.KanWavGeom(B, C, H, W, O, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, int(wavelet), xbs or C * H * W, ubs or O * Ho * Wo)


def route_of(g):
    from convkan_amd import _lib as L
    r = L.KanWavRoute()
    L.check(L.load().kan_wav_route(ctypes.byref(g), ctypes.byref(r)), "kan_wav_route")
    return r


def wav_key(r, g):
    """(forward, bwd-input, bwd-params) ids of KanWavRoute `r` for KanWavGeom `g`."""
    if not r.fwd_fits:
        fwd = "fwd-refuse"
    else:
        fwd = "fwd-" + ("multi" if r.NIMG > 1 else "single") + ("-shrunk" if r.fwd_shrunk else "") + ("-cut" if r.fwd_nimg_cut else "") + \
            ("-grid" if r.tiles_h * r.tiles_w > 1 else "") + ("-ragged" if g.Ho % r.TH or g.Wo % r.TW or g.B % r.NIMG else "")
    par = f"-p{r.passes}" + ("-chunked" if r.chunks > 1 else "")
    if r.params_kernel == 0:
        par = "par-TILED" + par + f"-items{1 if r.items_per_chunk == 1 else 2}" + ("-raggedband" if g.H % r.BH else "") + ("-raggedimg" if g.B % r.NI else "")
    else:
        par = "par-PIXEL" + par + ("-raggedchunk" if (g.B * g.H * g.W) % r.px_per_chunk else "")
    return fwd, "bi-" + BI[r.bwd_input_kernel], par


def keys_of(B, C, O, H, W, k, s=1, p=0, d=1):
    g = geom_of(B, C, O, H, W, k, s, p, d)
    return wav_key(route_of(g), g) if g is not None else None


def case_geom(case, xbs=None, ubs=None):
    return geom_of(*(case[n] for n in ("B", "C", "O", "H", "W", "k", "s", "p", "d")), WAVELETS.index(case["wavelet"]), xbs, ubs)


def case_keys(case):
    g = case_geom(case)
    return wav_key(route_of(g), g)


# ------------------------------------------------------------------------------------------ the committed grid
KERNELS = (1, (1, 3), (3, 1), 3, (2, 5), 5, 7)
PASS_KERNELS = ((3, 6), (1, 19), (3, 9), (4, 7))                          # 18 | 19 and 27 | 28 taps: the pass counts' switch points
SQUARES = tuple((n, n) for n in range(1, 49))
RECTS = tuple((h, w) for h in (1, 2, 3, 8, 20, 48) for w in (32, 56, 129, 223, 224, 255, 256, 257, 260))
BATCHES = (1, 2, 3, 17, 129, 645)
CHANNELS = (1, 3, 5, 17, 64)


@functools.lru_cache(maxsize=1)
def sweep():
    """{key: first (B, C, O, H, W, k, s, p, d) of the grid that reaches it}, over all three stages.  The forward and the bwd-input
    routes do not look at C and O, the bwd-params route does not look at stride and padding: two sweeps instead of their product."""
    seen = {}

    def visit(stages, *a):
        keys = keys_of(*a)
        if keys is not None:
            for i in stages:
                seen.setdefault(keys[i], a)
    for H, W in SQUARES + RECTS:
        for k in KERNELS + PASS_KERNELS:
            for d in (1, 2):
                for s in (1, 2, 3):
                    for p in range(7):
                        for B in BATCHES[:4] if (H, W) in RECTS else BATCHES:
                            visit((0, 1), B, 3, 3, H, W, k, s, p, d)
                for B in BATCHES:
                    for Cn in CHANNELS:
                        for O in CHANNELS:
                            visit((2,), B, Cn, O, H, W, k, 1, 6, d)
    return seen


# ------------------------------------------------------------------------------------------ the table
def row(fwd, bi, par, B, C, O, H, W, k, s=1, p=0, d=1, wavelet="mexican_hat", kind=None, neg=False, x3=False, seed=0):
    """k, s, p, d: an int or an (h, w) pair.  kind: "bstride" x / du / u / dx laid out with a batch stride larger than dense, through
    the C ABI | "refuse" the forward must refuse (host-side).  neg: negative scales on a quarter of the (o, c) pairs; x3: inputs times 3."""
    return dict(fwd=fwd, bi=bi, par=par, B=B, C=C, O=O, H=H, W=W, k=k, s=s, p=p, d=d, wavelet=wavelet, kind=kind, neg=neg, x3=x3, seed=seed)


# fmt: off
WAV_CASES = [
    # the tiled parameter kernel, 1 pass (<= 9 taps): one work item | several | a ragged last band | a ragged last image group | a workgroup looping over
    # several items, plain / ragged band / ragged image group (pairs of 16 x 16 (o, c) = 1, so more than 2048 items)
    row("fwd-multi", "bi-TAPS9", "par-TILED-p1-items1", 2, 3, 5, 5, 7, 3, 1, (2, 1), wavelet="mexican_hat"),
    row("fwd-multi-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items1", 3, 5, 3, 16, 16, 3, (1, 2), 1, wavelet="morlet"),
    row("fwd-single-grid-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items1-raggedband", 2, 3, 5, 20, 32, 3, 1, 1, kind="bstride", wavelet="dog"),
    row("fwd-multi-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items1-raggedimg", 17, 2, 17, 5, 5, (1, 3), 1, (0, 1), neg=True, wavelet="meyer"),
    row("fwd-single", "bi-TAPS9", "par-TILED-p1-chunked-items2", 2049, 2, 3, 16, 16, 3, 1, 1, wavelet="shannon"),
    row("fwd-single-grid-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items2-raggedband", 1025, 2, 3, 17, 17, (3, 1), 1, (1, 0), wavelet="mexican_hat"),
    row("fwd-multi-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items2-raggedimg", 8193, 3, 2, 8, 8, 1, neg=True, wavelet="morlet"),
    # the same cells at 2 passes (10 ... 18 taps; the ragged band is the 33 x 56 row at the end)
    row("fwd-single", "bi-STRIDE1", "par-TILED-p2-items1", 1, 1, 1, 4, 6, (2, 5), 1, (1, 2), wavelet="shannon"),
    row("fwd-multi-ragged", "bi-STRIDED", "par-TILED-p2-chunked-items1", 4, 5, 5, 16, 16, (3, 6), 2, (1, 3), wavelet="mexican_hat"),
    row("fwd-multi-ragged", "bi-STRIDE1", "par-TILED-p2-chunked-items1-raggedimg", 9, 17, 3, 6, 6, (2, 5), 1, (1, 2), wavelet="shannon"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p2-chunked-items2", 2049, 3, 2, 16, 16, (3, 6), 1, (1, 3), wavelet="mexican_hat"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p2-chunked-items2-raggedband", 1025, 2, 3, 17, 17, (2, 5), 1, (1, 2), neg=True, wavelet="morlet"),
    row("fwd-multi", "bi-STRIDE1", "par-TILED-p2-chunked-items2-raggedimg", 8193, 2, 3, 8, 8, (2, 5), 1, (1, 2), wavelet="dog"),
    # 3 passes (19 ... 27 taps); the 10245-image row: LDS holds NI = 5 images per item, 2049 items on 1025 chunks
    row("fwd-single", "bi-STRIDE1", "par-TILED-p3-items1", 2, 3, 5, 7, 7, 5, 1, 5, wavelet="meyer"),
    row("fwd-multi-ragged", "bi-STRIDED", "par-TILED-p3-chunked-items1", 3, 3, 5, 16, 16, (3, 9), (1, 2), (2, 4), (2, 1), wavelet="morlet"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p3-chunked-items1-raggedband", 2, 5, 3, 20, 32, (1, 19), 1, (0, 9), neg=True, wavelet="mexican_hat"),
    row("fwd-multi-ragged", "bi-STRIDE1", "par-TILED-p3-chunked-items1-raggedimg", 17, 3, 5, 5, 5, 5, 1, 4, (1, 2), wavelet="morlet"),
    row("fwd-multi-cut-ragged", "bi-STRIDE1", "par-TILED-p3-chunked-items2", 10245, 2, 3, 4, 4, 5, 1, 4, 2, wavelet="dog"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p3-chunked-items2-raggedband", 1025, 3, 2, 17, 17, 5, 1, 2, wavelet="meyer"),
    row("fwd-multi-ragged", "bi-STRIDE1", "par-TILED-p3-chunked-items2-raggedimg", 8193, 2, 3, 8, 8, 5, 1, 2, x3=True, wavelet="shannon"),
    # 4 passes (28 taps)
    row("fwd-single", "bi-STRIDE1", "par-TILED-p4-items1", 1, 2, 3, 5, 8, (4, 7), 1, (2, 3), neg=True, wavelet="mexican_hat"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p4-chunked-items1", 2, 3, 5, 16, 16, (4, 7), 1, (2, 3), wavelet="morlet"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p4-chunked-items1-raggedband", 1, 5, 3, 20, 32, (4, 7), 1, (2, 3), wavelet="dog"),
    row("fwd-multi-ragged", "bi-STRIDE1", "par-TILED-p4-chunked-items1-raggedimg", 9, 3, 5, 6, 6, (4, 7), 1, (2, 3), wavelet="meyer"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p4-chunked-items2", 2049, 2, 3, 16, 16, (4, 7), 1, (2, 3), neg=True, wavelet="shannon"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p4-chunked-items2-raggedband", 1025, 2, 3, 17, 17, (4, 7), 1, (2, 3), wavelet="mexican_hat"),
    row("fwd-multi", "bi-STRIDE1", "par-TILED-p4-chunked-items2-raggedimg", 8193, 2, 3, 8, 8, (4, 7), 1, (2, 3), wavelet="morlet"),
    # 6 passes (7 x 7)
    row("fwd-single", "bi-STRIDE1", "par-TILED-p6-items1", 1, 3, 5, 7, 9, 7, 1, 3, wavelet="dog"),
    row("fwd-single", "bi-STRIDE1", "par-TILED-p6-chunked-items1", 2, 5, 3, 16, 16, 7, 1, 3, neg=True, wavelet="meyer"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p6-chunked-items1-raggedband", 1, 3, 5, 20, 32, 7, 1, 3, wavelet="shannon"),
    row("fwd-multi-ragged", "bi-STRIDE1", "par-TILED-p6-chunked-items1-raggedimg", 9, 3, 5, 6, 6, 7, 1, 3, wavelet="mexican_hat"),
    row("fwd-single", "bi-STRIDE1", "par-TILED-p6-chunked-items2", 2049, 2, 3, 16, 16, 7, 1, 3, wavelet="morlet"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-TILED-p6-chunked-items2-raggedband", 1025, 2, 3, 17, 17, 7, 1, 3, wavelet="dog"),
    row("fwd-multi-ragged", "bi-STRIDE1", "par-TILED-p6-chunked-items2-raggedimg", 8194, 2, 3, 8, 8, 7, 1, 3, neg=True, wavelet="meyer"),
    # the per-pixel parameter kernel (the band does not fit 56 KB of LDS), per pass count: one chunk | several | a ragged last chunk
    row("fwd-single-grid", "bi-TAPS9", "par-PIXEL-p1", 1, 3, 5, 1, 224, 3, 1, 1, wavelet="shannon"),
    row("fwd-single-grid-ragged", "bi-TAPS9", "par-PIXEL-p1-chunked", 1, 3, 5, 2, 223, 3, 1, 1, wavelet="mexican_hat"),
    row("fwd-single-grid-ragged", "bi-TAPS9", "par-PIXEL-p1-chunked-raggedchunk", 1, 3, 5, 2, 257, 3, 1, 1, neg=True, wavelet="morlet"),
    row("fwd-single-grid", "bi-STRIDE1", "par-PIXEL-p2", 1, 3, 5, 1, 224, (2, 5), 1, (2, 4), 2, wavelet="dog"),
    row("fwd-multi-grid", "bi-STRIDE1", "par-PIXEL-p2-chunked", 2, 3, 5, 1, 224, (2, 5), 1, (2, 4), 2, wavelet="meyer"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-PIXEL-p2-chunked-raggedchunk", 1, 3, 5, 1, 257, (2, 5), 1, (2, 4), 2, wavelet="shannon"),
    row("fwd-single", "bi-STRIDE1", "par-PIXEL-p3", 1, 3, 5, 16, 16, (3, 9), 1, (2, 8), 2, neg=True, wavelet="mexican_hat"),
    row("fwd-multi", "bi-STRIDED", "par-PIXEL-p3-chunked", 2, 3, 5, 8, 32, 5, (1, 2), 4, 2, wavelet="morlet"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-PIXEL-p3-chunked-raggedchunk", 1, 3, 5, 9, 41, 5, 1, 4, (2, 3), kind="bstride", wavelet="dog"),
    row("fwd-single-grid", "bi-STRIDE1", "par-PIXEL-p4", 1, 3, 5, 4, 64, (4, 7), 1, (3, 6), 2, wavelet="meyer"),
    row("fwd-multi-grid", "bi-STRIDE1", "par-PIXEL-p4-chunked", 2, 3, 5, 4, 64, (4, 7), 1, (3, 6), 2, x3=True, wavelet="shannon"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-PIXEL-p4-chunked-raggedchunk", 1, 3, 5, 5, 67, (4, 7), 1, (3, 6), 2, wavelet="mexican_hat"),
    row("fwd-single", "bi-STRIDE1", "par-PIXEL-p6", 1, 3, 5, 15, 15, 7, 1, 6, 2, wavelet="morlet"),
    row("fwd-single-grid-ragged", "bi-STRIDE1", "par-PIXEL-p6-chunked-raggedchunk", 1, 3, 5, 17, 17, 7, 1, 6, 2, wavelet="dog"),
    # the forward's remaining cells: the tile-shrinking loop (a 16 x 16 tile's region above 1792 cells), the NIMG cut, grids, ragged edges
    row("fwd-single-shrunk-grid", "bi-STRIDED", "par-PIXEL-p6-chunked", 1, 2, 5, 32, 32, 7, 2, 6, 2, wavelet="dog", kind="bstride", neg=True),
    row("fwd-single-shrunk-cut-grid", "bi-TAPS9", "par-TILED-p1-chunked-items1-raggedband", 3, 3, 5, 48, 48, 3, 3, 1, wavelet="shannon"),
    row("fwd-single-shrunk-cut-grid-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items1", 2, 3, 5, 50, 48, 3, 3, 1, wavelet="mexican_hat"),
    row("fwd-single-shrunk-grid-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items1", 1, 3, 5, 50, 48, 3, 3, 1, wavelet="morlet"),
    row("fwd-multi-shrunk-grid", "bi-TAPS9", "par-TILED-p1-chunked-items1", 2, 3, 5, 48, 32, (1, 3), 3, 2, 2, wavelet="dog"),
    row("fwd-multi-shrunk-grid-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items1", 3, 3, 5, 48, 32, (1, 3), 3, 2, 2, neg=True, wavelet="meyer"),
    row("fwd-single-cut", "bi-TAPS9", "par-TILED-p1-chunked-items1", 2, 3, 5, 48, 20, 3, 3, 1, wavelet="shannon"),
    row("fwd-single-cut-grid", "bi-TAPS9", "par-TILED-p1-chunked-items1", 2, 3, 5, 24, 96, 3, 3, 1, wavelet="mexican_hat"),
    row("fwd-single-cut-grid-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items1", 2, 3, 5, 24, 100, 3, 3, 1, wavelet="morlet"),
    row("fwd-multi-cut", "bi-TAPS9", "par-TILED-p1-chunked-items1-raggedband", 10, 3, 5, 18, 18, 3, 3, 1, wavelet="dog"),
    row("fwd-multi-cut-grid-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items1-raggedband", 8, 3, 5, 6, 50, 3, 3, 1, wavelet="meyer"),
    row("fwd-multi-grid-ragged", "bi-TAPS9", "par-TILED-p1-items1", 2, 3, 5, 6, 20, 3, 1, 1, (1, 2), wavelet="shannon"),
    # switch points not yet on both sides: the region of a 16 x 16 tile = 1792 cells exactly | 1848; the LDS limit of the band at W = 222 (| 223 above)
    row("fwd-single", "bi-STRIDED", "par-TILED-p2-chunked-items1", 1, 3, 5, 32, 56, (2, 6), (2, 3), 0, (1, 2), wavelet="meyer"),
    row("fwd-single-shrunk-grid", "bi-STRIDED", "par-TILED-p2-chunked-items1-raggedband", 1, 3, 5, 33, 56, (2, 6), (2, 3), 0, 2, wavelet="shannon"),
    row("fwd-single-grid-ragged", "bi-TAPS9", "par-TILED-p1-chunked-items1", 1, 3, 5, 2, 222, 3, 1, 1, wavelet="dog"),
    # the forward refuses (host-side, before any launch): a single pixel's region does not fit 64 KB
    row("fwd-refuse", "bi-STRIDE1", "par-PIXEL-p6", 1, 2, 3, 4, 4, 7, 1, 24, 8, kind="refuse", wavelet="meyer"),
]
# fmt: on


def case_id(case):
    f = lambda v: str(v) if isinstance(v, int) else f"{v[0]}x{v[1]}"
    return f"B{case['B']}C{case['C']}O{case['O']}-{case['H']}x{case['W']}-k{f(case['k'])}s{f(case['s'])}p{f(case['p'])}d{f(case['d'])}-{case['wavelet']}" + \
        (f"-{case['kind']}" if case["kind"] else "") + ("-neg" if case["neg"] else "") + ("-x3" if case["x3"] else "")


def case_ids(cases):
    return [case_id(c) for c in cases]


# ------------------------------------------------------------------------------------------ inputs and the reference
def _psi(x, scale, trans, kind):
    """Wavelet values [b, O, C, H, W] of x [b, C, H, W]."""
    from oracle.kan_oracle import wavelet
    O, Cn = scale.shape
    return wavelet((x[:, None] - trans.view(1, O, Cn, 1, 1)) / scale.view(1, O, Cn, 1, 1), kind)


def _draw(case, seed):
    g = torch.Generator().manual_seed(seed)
    B, Cn, O, H, W = (case[n] for n in ("B", "C", "O", "H", "W"))
    kh, kw = _pair(case["k"])
    x = torch.randn(B, Cn, H, W, generator=g, dtype=torch.float64) * (3 if case["x3"] else 1)
    scale = 0.5 + 1.1 * torch.rand(O, Cn, generator=g, dtype=torch.float64)
    if case["neg"]:
        scale.view(-1)[1::4] *= -1
    trans = 0.5 * torch.randn(O, Cn, generator=g, dtype=torch.float64)
    w = torch.randn(O, Cn, kh, kw, generator=g, dtype=torch.float64) / math.sqrt(Cn * kh * kw)
    geom = case_geom(case)
    du = torch.randn(B, O, geom.Ho, geom.Wo, generator=g, dtype=torch.float64)
    return g, x, scale, trans, w, du


def _on_kink(x, scale, trans):
    """Input elements of x [B, C, H, W] whose |u| is below MEYER_KINK for some output (fp64)."""
    O, Cn = scale.shape
    u = (x[:, None] - trans.view(1, O, Cn, 1, 1)) / scale.view(1, O, Cn, 1, 1)
    return (u.abs() < MEYER_KINK).any(1)


@functools.lru_cache(maxsize=4)
def _inputs(idx):
    case = WAV_CASES[idx]
    g, x, scale, trans, w, du = _draw(case, 2000 + case["seed"])
    redrawn = torch.zeros(x.shape, dtype=torch.bool)
    if case["wavelet"] == "meyer":
        step = max(1, CHUNK_ELEMS // (x[0].numel() * case["O"]))
        for _ in range(100):
            bad = torch.cat([_on_kink(x[b:b + step], scale, trans) for b in range(0, case["B"], step)])
            if not bad.any():
                break
            x[bad] = torch.randn(int(bad.sum()), generator=g, dtype=torch.float64) * (3 if case["x3"] else 1)
            redrawn |= bad
        else:
            raise AssertionError(f"{case}: Meyer conditioning does not settle")
    # the rows are fp32 data: what the kernels are given, exactly, is also what both executions of the reference start from
    return tuple(t.float() for t in (x, scale, trans, w, du)), float(redrawn.float().mean())


def make_inputs(case):
    """fp32 CPU tensors of a row: x [B, C, H, W], scale and trans [O, C], w [O, C, kh, kw], du [B, O, Ho, Wo]."""
    return _inputs(WAV_CASES.index(case))[0]


def redraw_share(case):
    """Share of the row's input elements its Meyer conditioning drew again (0 on the other wavelets)."""
    return _inputs(WAV_CASES.index(case))[1]


def stage(x, scale, trans, w, kind, s, p, d):
    """u [b, O, Ho, Wo] = sum_c conv2d(psi[:, o, c], w[o, c]) per output o, zero padding applied to the wavelet values: one conv2d per
    output over its C wavelet planes, spelled as one grouped call (group o = output o)."""
    psi = _psi(x, scale, trans, kind)
    b, O, Cn, H, W = psi.shape
    return F.conv2d(psi.reshape(b, O * Cn, H, W), w, None, _pair(s), _pair(p), _pair(d), groups=O)


def run_reference(case, inputs, dtype):
    """u, dx, dw, dscale, dtrans of the stage in `dtype`: plain torch on the CPU, gradients by autograd, images in chunks."""
    x, scale, trans, w, du = (t.to(dtype) for t in inputs)
    scale, trans, w = (t.clone().requires_grad_(True) for t in (scale, trans, w))
    step = max(1, CHUNK_ELEMS // (x[0].numel() * case["O"]))
    us, dxs = [], []
    for b in range(0, case["B"], step):
        xc = x[b:b + step].clone().requires_grad_(True)
        u = stage(xc, scale, trans, w, case["wavelet"], case["s"], case["p"], case["d"])
        u.backward(du[b:b + step])
        us.append(u.detach()); dxs.append(xc.grad)
    return dict(u=torch.cat(us), dx=torch.cat(dxs), dw=w.grad, dscale=scale.grad, dtrans=trans.grad)


@functools.lru_cache(maxsize=2)
def reference_pair(idx):
    """Row WAV_CASES[idx]: (inputs, fp64 results, fp32 results) -- computed once, shared, never modified."""
    case = WAV_CASES[idx]
    inputs = make_inputs(case)
    return inputs, run_reference(case, inputs, torch.float64), run_reference(case, inputs, torch.float32)


def reference(case, dtype):
    ref = reference_pair(WAV_CASES.index(case))
    return ref[1] if dtype == torch.float64 else ref[2]
