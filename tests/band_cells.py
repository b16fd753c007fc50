"""The cell matrix of the band conv kernels (csrc/kan_direct.hip: k_band_fwd, k_band_bwd_weight): which instantiation and which run-time switches
`kan_band_route` reports for a launch, one oracle row per cell.

The public KanPlan shows fwd_band / bwd_weight_band and little else; kan_band_cfg chooses per geometry the channels per group NG, the wave tile
(MO, WP), the live expansion units, the phase list, split-K, the LDS class and how many images share a pixel tile, and for the weight gradient
(WR, NI), SLOTS, the pixel tiles per image and the splits.  kan_band_route (include/kanconv.h) copies those out of the configuration the launchers
read, and two kinds of cell are keyed on it:

    instantiation cells   ("F", spec class, NG, MO, WP)               the k_band_fwd template body
                          ("W", spec class, NG, WR, NI, SLOTS)        the k_band_bwd_weight template body
    feature cells         ("Ff", NG, MO, WP, feature)                 a run-time switch of the forward under that tile, any spec
                          ("Wf", NG, WR, NI, SLOTS, feature)          ... of the weight gradient

A feature that is absent is not a cell (a launch without a ragged tile is every other row).  GRID is the committed set of geometries; a cell is
"reached" when some GRID geometry lands in it, and BAND_CASES holds, for every reached cell, the smallest geometry that reaches it under work()
(one row serves all the cells it lands in; tests/test_band_matrix.py keeps the table complete and minimal).  work() leaves the planes out, so
the specs tie on a geometry: a feature cell's row takes a spec that already has a row on that geometry, else the specs take turns
(SPEC_LAYERS[(B + C + O + H + W + G) % 6] first); instantiation cells name their spec.  A row that is the smallest of no cell any more is
dropped (tools/make_band_cases.py prints the rows from the grid by these rules).  tests/test_gpu_band_matrix.py runs every row against the
fp64 oracle."""
import ctypes
import itertools

from convkan_amd import _lib as L
import route_cells
from route_cells import FAST_NAMES, KINDS, LAYERS, ORACLE_EXTRA

# kernel geometries: those of route_cells.SHAPES plus a stride past the kernel (empty phases), wide strided kernels (many phases of unequal tap
# counts), stride + dilation, and a rectangular kernel
SHAPES = dict(route_cells.SHAPES,
              k2s3=dict(kernel_size=2, stride=3, padding=0, dilation=1), k7s2=dict(kernel_size=7, stride=2, padding=3, dilation=1),
              k11s4=dict(kernel_size=11, stride=4, padding=2, dilation=1), k5s3d2=dict(kernel_size=5, stride=3, padding=3, dilation=2),
              k3x1=dict(kernel_size=(3, 1), stride=1, padding=(1, 0), dilation=1))
# one layer per spec class with a band kernel (FAST_* of csrc/kan_internal.h with ON_BAND_FWD); the first four also have k_band_bwd_weight
SPEC_LAYERS = ("kan_silu", "kan_gelu", "fast_g8", "cheby_d4", "cheby_d3", "lucas_d3")
SPEC_OF = {"kan_silu": "FAST_BSPLINE_SILU", "kan_gelu": "FAST_BSPLINE_GELU", "fast_g8": "FAST_RBF8", "cheby_d4": "FAST_CHEBY5",
           "cheby_d3": "FAST_CHEBY4", "lucas_d3": "FAST_POLY4", "bessel_d3": "FAST_POLY4"}
BW_SPECS = ("FAST_BSPLINE_SILU", "FAST_BSPLINE_GELU", "FAST_RBF8", "FAST_CHEBY5")
PLANES_OF = {"FAST_BSPLINE_SILU": 9, "FAST_BSPLINE_GELU": 9, "FAST_RBF8": 9, "FAST_CHEBY5": 5, "FAST_CHEBY4": 4, "FAST_POLY4": 5}
# the compiled instantiations: band_has_kernel (kan_direct.hip) and the (WR, NI) list of kan_band_bwd_weight_launch
FWD_TILES = ((1, 2), (2, 2), (3, 2), (1, 4))                      # (MO, WP)
BW_TILES = ((4, 2), (8, 2), (4, 4), (4, 6))                       # (WR, NI)
BW_SLOTS = (3, 6)

# ---------------------------------------------------------------------------------------------------------------- the grid
GRID_C = (1, 2, 3, 4, 5, 6, 7, 8)
GRID_O = (2, 40, 64, 96, 128, 192, 256, 320)
GRID_PLANES = ((3, 3), (4, 4), (5, 5), (7, 9), (8, 8), (13, 13), (16, 16), (32, 32), (64, 64), (40, 200))
GRID_B = (1, 2, 3, 8, 16, 17, 40)
GRID_G2 = dict(B=(2, 17), planes=((5, 5), (13, 13), (32, 32)))    # two groups: on a part of the grid
MIN_PIXELS = 4                                                   # InstanceNorm over fewer output pixels is pure cancellation in the reference itself
MAX_FLOPS = 3.0e9                                                # dense FLOPs of a geometry: a row stays well under a second on the GPU


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_hw(shape, H, W):
    s = SHAPES[shape]
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = (_pair(s[n]) for n in ("kernel_size", "stride", "padding", "dilation"))
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def taps(shape):
    kh, kw = _pair(SHAPES[shape]["kernel_size"])
    return kh * kw


def work(c):
    """The stated order of the table: multiply-adds of the dense convolution per plane of the basis, B Ho Wo (C / G) O kh kw (planes left out, so that
    the specs tie on one geometry), then the geometry itself."""
    Ho, Wo = out_hw(c["shape"], c["H"], c["W"])
    return c["B"] * Ho * Wo * (c["C"] // c["G"]) * c["O"] * taps(c["shape"])


def order(c):
    return (work(c), c["B"], c["C"], c["O"], c["H"], c["W"], c["G"], sorted(SHAPES).index(c["shape"]))


def grid():
    """Every geometry of the grid as a dict(shape, B, C, O, H, W, G) (C, O: totals over the groups), without a layer: MIN_PIXELS output pixels at
    least and under MAX_FLOPS for the nine-plane specs."""
    for shape in SHAPES:
        for (H, W) in GRID_PLANES:
            Ho, Wo = out_hw(shape, H, W)
            if Ho <= 0 or Wo <= 0 or Ho * Wo < MIN_PIXELS:
                continue
            for B, C_, O in itertools.product(GRID_B, GRID_C, GRID_O):
                gs = (1, 2) if (B in GRID_G2["B"] and (H, W) in GRID_G2["planes"]) else (1,)
                for G in gs:
                    c = dict(shape=shape, B=B, C=C_ * G, O=O * G, H=H, W=W, G=G)
                    if 2.0 * work(c) * 9 < MAX_FLOPS:
                        yield c


def grid_layers(c):
    """The spec layers a grid geometry is planned for: all six, without ChebyKAN under the rectangular kernel (its constructor takes an int
    kernel_size, as the reference's does)."""
    return tuple(l for l in SPEC_LAYERS if not (c["shape"] == "k3x1" and l.startswith("cheby")))


# ---------------------------------------------------------------------------------------------------------------- structs and keys
def geom_of(c):
    """KanGeom of a geometry dict, as ops._plan_cached builds it (dense batch strides)."""
    s = SHAPES[c["shape"]]
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = (_pair(s[n]) for n in ("kernel_size", "stride", "padding", "dilation"))
    Ho, Wo = out_hw(c["shape"], c["H"], c["W"])
    G = c["G"]
    g = L.KanGeom()
    g.B, g.C, g.H, g.W, g.O, g.Ho, g.Wo = c["B"], c["C"] // G, c["H"], c["W"], c["O"] // G, Ho, Wo
    g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, g.dh, g.dw, g.groups = kh, kw, sh, sw, ph, pw, dh, dw, G
    g.x_bstride, g.y_bstride = c["C"] * c["H"] * c["W"], c["O"] * Ho * Wo
    return g


_BASES = {}


def basis_of(layer):
    """KanBasis of LAYERS[layer] (host fields only: what the planner reads)."""
    if layer not in _BASES:
        from golden.make_plan_snapshot import basis_key, make_structs
        import convkan_amd as K
        cls, kw = LAYERS[layer]
        _BASES[layer] = make_structs([0] * 18, basis_key(getattr(K, cls)(4, 4, 3, **kw).conv_spec()))[1]
    return _BASES[layer]


def band_route(g, b):
    """kan_band_route of the library, or None for a geometry the planner rejects."""
    r = L.KanBandRoute()
    rc = L.load().kan_band_route(ctypes.byref(g), ctypes.byref(b), ctypes.byref(r))
    return r if rc == 0 else None


def fwd_features(g, r):
    f = ["units1" if r.slots == 1 else "units6" if r.slots == 6 else "units2-5",
         "empty-phase" if r.empty_phase else "phases" if r.n_phase > 1 else "phase1",
         "splits" if r.fwd_splits > 1 else "split1",
         "lds>64K" if r.lds_bytes > 65536 else "lds<=64K",
         "img1" if r.max_images == 1 else "img2" if r.max_images == 2 else "img3+"]
    if (g.B * g.Ho * g.Wo) % r.TP:
        f.append("ragged-pixels")
    if g.C % r.NG:
        f.append("ragged-group")
    if (r.NG * r.P) & 1:
        f.append("pad-row")
    if g.O % r.TO:
        f.append("ragged-O")
    if g.groups > 1:
        f.append("groups2")
    return f


def bw_features(g, r):
    f = ["tpi>1" if r.bw_TPI > 1 else "tpi1", "splits" if r.bw_splits > 1 else "split1", "lds>64K" if r.bw_lds_bytes > 65536 else "lds<=64K"]
    if (g.Ho * g.Wo) % 128:
        f.append("partial-pixel-tile")
    if any((r.phase_taps[i] * r.NPLE) % (32 * r.bw_WR) for i in range(r.n_phase)):
        f.append("partial-row-tile")
    if g.C % r.NG:
        f.append("ragged-group")
    if g.O % (32 * r.bw_NI):
        f.append("ragged-O")
    if g.groups > 1:
        f.append("groups2")
    return f


def cells_of(g, b, r):
    """The cells a launch lands in, from its route: instantiation cells first."""
    spec = "FAST_" + FAST_NAMES[r.fast] if r.fwd_band else None
    out = []
    if r.fwd_band:
        out.append(("F", spec, r.NG, r.MO, r.WP))
        out += [("Ff", r.NG, r.MO, r.WP, f) for f in fwd_features(g, r)]
    if r.bw_band:
        out.append(("W", spec, r.NG, r.bw_WR, r.bw_NI, r.bw_slots))
        out += [("Wf", r.NG, r.bw_WR, r.bw_NI, r.bw_slots, f) for f in bw_features(g, r)]
    return out


def cell_id(cell):
    return "-".join(str(v).replace("FAST_", "") for v in cell)


# ---------------------------------------------------------------------------------------------------------------- rows
def brow(layer, shape, B, C, O, H, W, fwd, bw, G=1, **opts):
    """One BAND_CASES row: LAYERS[layer] with the SHAPES[shape] conv geometry on [B, C, H, W] (C, O: totals over G groups), and the instantiations
    it declares: fwd = 'NG/MO/WP' of k_band_fwd, bw = 'WR/NI/SLOTS' of k_band_bwd_weight or None where the weight gradient leaves the band route.
    opts: scale (input multiplier on top of 1.3), affine (perturbed affine InstanceNorm), seed (another draw: the reason stands next to the row)."""
    spec = SPEC_OF[layer]
    NG, MO, WP = (int(v) for v in fwd.split("/"))
    cells = [("F", spec, NG, MO, WP)] + ([("W", spec, NG) + tuple(int(v) for v in bw.split("/"))] if bw else [])
    return dict(layer=layer, shape=shape, B=B, C=C, O=O, H=H, W=W, G=G, cells=cells, **opts)


def case_layer(case):
    import convkan_amd as K
    cls, kw = LAYERS[case["layer"]]
    kw = dict(kw, groups=case["G"], **SHAPES[case["shape"]])
    if case.get("affine"):
        kw["affine"] = True
    return getattr(K, cls)(case["C"], case["O"], **kw)


def case_structs(case, layer=None):
    return route_cells.case_structs(case, case_layer(case) if layer is None else layer)


def case_cfg(case, layer):
    """The oracle config of helpers.oracle_forward for the row's layer (route_cells.case_cfg on this table's SHAPES)."""
    import torch.nn as nn
    cls, kw = LAYERS[case["layer"]]
    kind, s = KINDS[cls], SHAPES[case["shape"]]
    cfg = dict(kind=kind, C=case["C"], O=case["O"], k=s["kernel_size"], s=s["stride"], p=s["padding"], d=s["dilation"], groups=case["G"],
               extra={n: kw[n] for n in ORACLE_EXTRA.get(kind, ())})
    act = getattr(layer, "base_activation", None)
    if act is not None:
        cfg["act"] = {nn.SiLU: "silu", nn.GELU: "gelu"}[act if isinstance(act, type) else type(act)]
    return cfg


def case_id(case):
    return "-".join(str(case[k]) for k in ("layer", "shape", "B", "C", "O", "H", "W", "G"))


def case_ids(cases):
    return [case_id(c) for c in cases]


def case_route(case):
    g, b, _ = case_structs(case)
    return g, b, band_route(g, b)


def built(case):
    """(layer, x) of a row, seeded: the layer's own init, a perturbed affine norm where the row says so, and the input -- randn x 1.3, x 3 more on
    alternating rows of the B-spline and RBF specs (past the grid range).  The CPU conditioning check and the GPU tests build the same tensors."""
    import torch
    torch.manual_seed(case.get("seed", 0))
    layer = case_layer(case)
    gen = torch.Generator().manual_seed(1 + case.get("seed", 0))
    if case.get("affine"):
        with torch.no_grad():
            for m in layer.layer_norm:
                m.weight.add_(0.2 * torch.randn(m.weight.shape, generator=gen))
                m.bias.add_(0.2 * torch.randn(m.bias.shape, generator=gen))
    x = torch.randn(case["B"], case["C"], case["H"], case["W"], generator=gen) * 1.3 * case.get("scale", 1.0)
    return layer, x


# Instantiations that are compiled (FWD_TILES x NG 1..3 per forward spec; BW_TILES x BW_SLOTS x NG 1..3 per weight-gradient spec) and that no GRID
# geometry reaches: {cell: (the most expansion units, NG x bw_cells, of any GRID launch of its (spec, NG, WR, NI); one-line reason)}.
# tests/test_band_matrix.py fails when one of them becomes reachable or when the figure no longer holds.  All ten are the eight-wave row tile
# (WR, NI) = (8, 2) with six expansion slots, which takes a phase of more than 128 rows (13 taps at NG = 1, 8 at NG = 2, 5 at NG = 3 of a nine-plane
# spec; 22 at NG = 1 of ChebyKAN) AND more than 3 x 512 = 1536 units.
_NINE = "units of the widest (8, 2) launch of GRID, 1536 would still be 3 per thread; a nine-plane halo wide enough for more is over the forward's " \
        "six units per thread or 80 KB on every GRID geometry, which takes the whole layer off the band route"
UNREACHED = {
    ("W", "FAST_BSPLINE_SILU", 1, 8, 2, 6): (1224, _NINE), ("W", "FAST_BSPLINE_SILU", 2, 8, 2, 6): (1236, _NINE),
    ("W", "FAST_BSPLINE_SILU", 3, 8, 2, 6): (1530, _NINE),
    ("W", "FAST_BSPLINE_GELU", 1, 8, 2, 6): (1224, _NINE), ("W", "FAST_BSPLINE_GELU", 2, 8, 2, 6): (1236, _NINE),
    ("W", "FAST_BSPLINE_GELU", 3, 8, 2, 6): (1530, _NINE),
    ("W", "FAST_RBF8", 1, 8, 2, 6): (1224, _NINE), ("W", "FAST_RBF8", 2, 8, 2, 6): (1236, _NINE), ("W", "FAST_RBF8", 3, 8, 2, 6): (1530, _NINE),
    ("W", "FAST_CHEBY5", 1, 8, 2, 6): (1224, "units: one ChebyKAN channel per group fills a 256-row tile only under 22 taps of one phase or more -- "
                                             "the 5x5 stride-1 kernel on GRID -- and its widest plane there, 40x200, needs 6 rows x 204 cells"),
}

# cells knowingly left without a row.  Empty on purpose.
EXEMPT = {}

# The smallest geometry of every cell GRID reaches (tests/test_band_matrix.py: by order()).  Rows of the B-spline and RBF specs alternate inputs scaled
# 3x past their grid range; every third row has a perturbed affine InstanceNorm (FastKAN: its input norm); the two recurrence families of FAST_POLY4
# take turns.
BAND_CASES = [
    brow('kan_silu', '1x1', 1, 2, 2, 3, 3, '2/1/4', '4/2/3'),
    brow('kan_silu', '1x1', 1, 3, 2, 3, 3, '3/1/4', '4/2/3', scale=3.0),
    brow('kan_silu', 's2', 1, 2, 2, 3, 3, '2/1/4', '4/2/3', affine=True),
    brow('kan_silu', 'p0', 1, 2, 2, 4, 4, '2/1/4', '8/2/3', scale=3.0),
    brow('kan_silu', '5x5s2', 1, 1, 2, 3, 3, '1/1/4', '4/2/3'),
    brow('kan_silu', 'p0', 1, 3, 2, 4, 4, '3/1/4', '8/2/3', scale=3.0, affine=True),
    brow('kan_silu', 'k2s3', 2, 4, 4, 5, 5, '2/1/4', '4/2/3', G=2),
    brow('kan_silu', 'p0', 2, 2, 2, 4, 4, '2/1/4', '8/2/3', scale=3.0),
    brow('kan_silu', 'p0', 1, 5, 2, 4, 4, '2/1/4', '8/2/3', affine=True),
    brow('kan_silu', 'k2s3', 2, 6, 4, 5, 5, '3/1/4', '4/2/3', G=2, scale=3.0),
    brow('kan_silu', 'k7s2', 1, 1, 2, 3, 3, '1/1/4', '8/2/3'),
    brow('kan_silu', '5x5s2', 2, 1, 2, 3, 3, '1/1/4', '4/2/3', scale=3.0, affine=True),
    brow('kan_silu', 'p0', 2, 3, 2, 4, 4, '3/1/4', '8/2/3'),
    brow('kan_silu', '1x1p2', 1, 2, 2, 7, 9, '2/1/4', '4/2/3', scale=3.0),
    brow('kan_silu', '1x1', 3, 2, 2, 7, 9, '2/1/2', '4/2/3', affine=True),
    brow('kan_silu', 'k7s2', 2, 1, 2, 3, 3, '1/1/4', '8/2/3', scale=3.0),
    brow('kan_silu', '1x1p2', 1, 3, 2, 7, 9, '3/1/4', '4/2/3'),
    brow('kan_silu', '1x1', 1, 1, 96, 3, 3, '1/2/2', '4/4/3', scale=3.0, affine=True),
    brow('kan_silu', '1x1', 3, 3, 2, 7, 9, '3/1/2', '4/2/3'),
    brow('kan_silu', 'p0', 2, 4, 4, 5, 5, '2/1/4', '8/2/3', G=2, scale=3.0),
    brow('kan_silu', '1x1', 1, 1, 192, 3, 3, '1/3/2', '4/6/3', affine=True),
    brow('kan_silu', '1x1', 1, 2, 96, 3, 3, '2/2/2', '4/4/3', scale=3.0),
    brow('kan_silu', '1x1', 2, 1, 96, 3, 3, '1/2/2', '4/4/3'),
    brow('kan_silu', 'p0', 2, 6, 4, 5, 5, '3/1/4', '8/2/3', G=2, scale=3.0, affine=True),
    brow('kan_silu', 'p0', 17, 2, 2, 4, 4, '2/1/4', '8/2/3'),
    brow('kan_silu', '1x1', 1, 3, 96, 3, 3, '3/2/2', '4/4/3', scale=3.0),
    brow('kan_silu', '1x1', 1, 2, 192, 3, 3, '2/3/2', '4/6/3', affine=True),
    brow('kan_silu', '1x1', 2, 1, 192, 3, 3, '1/3/2', '4/6/3', scale=3.0),
    brow('kan_silu', '1x1', 2, 2, 96, 3, 3, '2/2/2', '4/4/3'),
    brow('kan_silu', '1x1', 1, 3, 192, 3, 3, '3/3/2', '4/6/3', scale=3.0, affine=True),
    brow('kan_silu', '1x1', 2, 3, 96, 3, 3, '3/2/2', '4/4/3'),
    brow('kan_silu', '1x1', 3, 2, 96, 3, 3, '2/2/2', '4/4/3', scale=3.0),
    brow('kan_silu', 'd2', 16, 2, 2, 3, 3, '2/1/4', None, affine=True),
    brow('kan_silu', '1x1p2', 1, 1, 40, 7, 9, '1/1/4', '4/2/3', scale=3.0),
    brow('kan_silu', 'k2s3', 2, 2, 192, 5, 5, '1/2/2', '4/4/3', G=2),
    brow('kan_silu', '1x1', 2, 2, 192, 3, 3, '2/3/2', '4/6/3', scale=3.0, affine=True),
    brow('kan_silu', 'd2', 8, 3, 2, 4, 4, '3/1/4', '8/2/3'),
    brow('kan_silu', '1x1', 3, 1, 40, 7, 9, '1/1/2', '4/2/3', scale=3.0),
    brow('kan_silu', 'p0', 40, 3, 2, 4, 4, '3/1/2', '8/2/3', affine=True),
    brow('kan_silu', '1x1', 2, 3, 192, 3, 3, '3/3/2', '4/6/3', scale=3.0),
    brow('kan_silu', '1x1', 3, 2, 192, 3, 3, '2/3/2', '4/6/3'),
    brow('kan_silu', 'k2s3', 2, 2, 384, 5, 5, '1/3/2', '4/6/3', G=2, scale=3.0, affine=True),
    brow('kan_silu', 'k2s3', 2, 4, 192, 5, 5, '2/2/2', '4/4/3', G=2),
    brow('kan_silu', 'd2', 40, 2, 2, 3, 3, '2/1/2', None, scale=3.0),
    brow('kan_silu', 'k2s3', 2, 4, 384, 5, 5, '2/3/2', '4/6/3', G=2, affine=True),
    brow('kan_silu', '1x1p2', 2, 3, 96, 3, 3, '3/2/2', '4/4/3', scale=3.0),
    brow('kan_silu', '1x1', 1, 2, 2, 40, 200, '2/1/2', '4/2/6'),
    brow('kan_silu', '1x1', 1, 3, 2, 40, 200, '3/1/2', '4/2/6', scale=3.0, affine=True),
    brow('kan_silu', '1x1p2', 2, 3, 192, 3, 3, '3/3/2', '4/6/3'),
    brow('kan_silu', 'd2', 8, 3, 96, 3, 3, '3/2/2', '4/4/3', scale=3.0),
    brow('kan_silu', '5x5', 1, 1, 2, 40, 200, '1/1/4', '8/2/3', affine=True),
    brow('kan_silu', 'k3x1', 1, 1, 40, 40, 200, '1/1/4', '4/2/6', scale=3.0),
    brow('kan_silu', '1x1', 1, 2, 96, 40, 200, '2/2/2', '4/4/6'),
    brow('kan_silu', 'k3x1', 1, 1, 96, 40, 200, '1/2/2', '4/4/6', scale=3.0, affine=True),
    brow('kan_silu', '1x1', 1, 3, 96, 40, 200, '3/2/2', '4/4/6'),
    brow('kan_silu', '1x1p1', 1, 3, 96, 40, 200, '3/2/2', '4/4/6', scale=3.0),
    brow('kan_silu', '1x1', 1, 2, 192, 40, 200, '2/3/2', '4/6/6', affine=True),
    brow('kan_silu', 'k3x1', 1, 1, 192, 40, 200, '1/3/2', '4/6/6', scale=3.0),
    brow('kan_silu', 'd2', 1, 3, 192, 32, 32, '3/3/2', '4/6/6'),
    brow('kan_silu', 'd2', 1, 1, 96, 40, 200, '1/2/2', '4/4/6', scale=3.0, affine=True),
    brow('kan_silu', 'k3x1', 2, 1, 192, 40, 200, '1/3/2', '4/6/6'),
    brow('kan_silu', 'd2', 1, 1, 192, 40, 200, '1/3/2', '4/6/6', scale=3.0),
    brow('kan_silu', 'k7s2', 1, 2, 96, 40, 200, '2/2/2', '4/4/6', affine=True),
    brow('kan_silu', '5x5s2', 1, 2, 192, 40, 200, '2/3/2', '4/6/6', scale=3.0),
    brow('kan_gelu', '1x1', 1, 2, 2, 3, 3, '2/1/4', '4/2/3'),
    brow('kan_gelu', '1x1', 1, 3, 2, 3, 3, '3/1/4', '4/2/3', scale=3.0, affine=True),
    brow('kan_gelu', '1x1', 2, 2, 2, 3, 3, '2/1/4', '4/2/3'),
    brow('kan_gelu', 'p0', 1, 2, 2, 4, 4, '2/1/4', '8/2/3', scale=3.0),
    brow('kan_gelu', '5x5s2', 1, 1, 2, 3, 3, '1/1/4', '4/2/3', affine=True),
    brow('kan_gelu', 's2', 1, 3, 2, 3, 3, '3/1/4', '4/2/3', scale=3.0),
    brow('kan_gelu', 'p0', 1, 3, 2, 4, 4, '3/1/4', '8/2/3'),
    brow('kan_gelu', '1x1', 1, 1, 40, 3, 3, '1/1/4', '4/2/3', scale=3.0, affine=True),
    brow('kan_gelu', 'k7s2', 1, 1, 2, 3, 3, '1/1/4', '8/2/3'),
    brow('kan_gelu', '5x5s2', 1, 3, 2, 3, 3, '3/1/4', '8/2/3', scale=3.0),
    brow('kan_gelu', '5x5s2', 3, 1, 2, 3, 3, '1/1/4', '4/2/3', affine=True),
    brow('kan_gelu', '1x1', 3, 2, 2, 7, 9, '2/1/2', '4/2/3', scale=3.0),
    brow('kan_gelu', '1x1', 1, 1, 96, 3, 3, '1/2/2', '4/4/3'),
    brow('kan_gelu', '1x1', 3, 3, 2, 7, 9, '3/1/2', '4/2/3', scale=3.0, affine=True),
    brow('kan_gelu', 'k2s3', 1, 1, 96, 5, 5, '1/2/2', '4/4/3'),
    brow('kan_gelu', '1x1', 1, 1, 192, 3, 3, '1/3/2', '4/6/3', scale=3.0),
    brow('kan_gelu', '1x1', 1, 2, 96, 3, 3, '2/2/2', '4/4/3', affine=True),
    brow('kan_gelu', '1x1', 1, 3, 96, 3, 3, '3/2/2', '4/4/3', scale=3.0),
    brow('kan_gelu', 'k2s3', 1, 1, 192, 5, 5, '1/3/2', '4/6/3'),
    brow('kan_gelu', '1x1', 1, 2, 192, 3, 3, '2/3/2', '4/6/3', scale=3.0, affine=True),
    brow('kan_gelu', '1x1', 1, 3, 192, 3, 3, '3/3/2', '4/6/3'),
    brow('kan_gelu', '1x1', 3, 1, 40, 7, 9, '1/1/2', '4/2/3', scale=3.0),
    brow('kan_gelu', '1x1', 3, 3, 96, 3, 3, '3/2/2', '4/4/3', affine=True),
    brow('kan_gelu', '5x5', 1, 1, 2, 13, 13, '1/1/4', '8/2/3', scale=3.0),
    brow('kan_gelu', '1x1', 1, 5, 192, 3, 3, '2/3/2', '4/6/3'),
    brow('kan_gelu', '1x1p2', 1, 1, 96, 7, 9, '1/2/2', '4/4/3', scale=3.0, affine=True),
    brow('kan_gelu', '1x1', 3, 3, 192, 3, 3, '3/3/2', '4/6/3'),
    brow('kan_gelu', 'k2s3', 1, 7, 192, 5, 5, '2/3/2', '4/6/3', scale=3.0),
    brow('kan_gelu', '1x1p2', 1, 1, 192, 7, 9, '1/3/2', '4/6/3', affine=True),
    brow('kan_gelu', '1x1', 1, 2, 2, 40, 200, '2/1/2', '4/2/6', scale=3.0),
    brow('kan_gelu', '1x1', 1, 3, 2, 40, 200, '3/1/2', '4/2/6'),
    brow('kan_gelu', 'd2', 16, 2, 96, 3, 3, '2/2/2', None, scale=3.0, affine=True),
    brow('kan_gelu', '5x5s2', 1, 3, 2, 40, 200, '3/1/2', '8/2/3'),
    brow('kan_gelu', 'd2', 8, 2, 192, 4, 4, '2/3/2', '4/6/3', scale=3.0),
    brow('kan_gelu', 'k3x1', 1, 1, 40, 40, 200, '1/1/4', '4/2/6', affine=True),
    brow('kan_gelu', '1x1', 1, 2, 96, 40, 200, '2/2/2', '4/4/6', scale=3.0),
    brow('kan_gelu', 'k3x1', 1, 1, 96, 40, 200, '1/2/2', '4/4/6'),
    brow('kan_gelu', '1x1', 1, 3, 96, 40, 200, '3/2/2', '4/4/6', scale=3.0, affine=True),
    brow('kan_gelu', '1x1', 1, 2, 192, 40, 200, '2/3/2', '4/6/6'),
    brow('kan_gelu', 'k3x1', 1, 1, 192, 40, 200, '1/3/2', '4/6/6', scale=3.0),
    brow('kan_gelu', 'd2', 1, 3, 192, 32, 32, '3/3/2', '4/6/6', affine=True),
    brow('kan_gelu', '1x1', 1, 5, 192, 40, 200, '2/3/2', '4/6/6', scale=3.0),
    brow('fast_g8', '1x1', 1, 2, 2, 3, 3, '2/1/4', '4/2/3'),
    brow('fast_g8', '1x1', 1, 3, 2, 3, 3, '3/1/4', '4/2/3', scale=3.0, affine=True),
    brow('fast_g8', '1x1', 2, 3, 2, 3, 3, '3/1/4', '4/2/3'),
    brow('fast_g8', '1x1', 3, 2, 2, 3, 3, '2/1/4', '4/2/3', scale=3.0),
    brow('fast_g8', 'p0', 1, 2, 2, 4, 4, '2/1/4', '8/2/3', affine=True),
    brow('fast_g8', '5x5s2', 1, 1, 2, 3, 3, '1/1/4', '4/2/3', scale=3.0),
    brow('fast_g8', 'p0', 1, 3, 2, 4, 4, '3/1/4', '8/2/3'),
    brow('fast_g8', 'k7s2', 1, 1, 2, 3, 3, '1/1/4', '8/2/3', scale=3.0, affine=True),
    brow('fast_g8', '1x1', 3, 2, 2, 7, 9, '2/1/2', '4/2/3'),
    brow('fast_g8', '1x1', 1, 1, 96, 3, 3, '1/2/2', '4/4/3', scale=3.0),
    brow('fast_g8', '1x1p1', 1, 2, 2, 13, 13, '2/1/2', '4/2/3', affine=True),
    brow('fast_g8', '1x1', 3, 3, 2, 7, 9, '3/1/2', '4/2/3', scale=3.0),
    brow('fast_g8', '1x1', 1, 1, 192, 3, 3, '1/3/2', '4/6/3'),
    brow('fast_g8', '1x1', 1, 2, 96, 3, 3, '2/2/2', '4/4/3', scale=3.0, affine=True),
    brow('fast_g8', '5x5s2', 2, 2, 4, 5, 5, '1/1/4', '4/2/3', G=2),
    brow('fast_g8', '1x1', 1, 3, 96, 3, 3, '3/2/2', '4/4/3', scale=3.0),
    brow('fast_g8', '1x1', 2, 4, 4, 13, 13, '2/1/2', '4/2/3', G=2, affine=True),
    brow('fast_g8', 'k2s3', 1, 2, 96, 5, 5, '2/2/2', '4/4/3', scale=3.0),
    brow('fast_g8', '1x1', 1, 2, 192, 3, 3, '2/3/2', '4/6/3'),
    brow('fast_g8', 'k7s2', 2, 2, 4, 5, 5, '1/1/4', '8/2/3', G=2, scale=3.0, affine=True),
    brow('fast_g8', '1x1', 1, 3, 192, 3, 3, '3/3/2', '4/6/3'),
    brow('fast_g8', '3x3', 1, 2, 2, 13, 13, '2/1/4', '8/2/3', scale=3.0),
    brow('fast_g8', 'k2s3', 1, 2, 192, 5, 5, '2/3/2', '4/6/3', affine=True),
    brow('fast_g8', '5x5', 16, 1, 2, 3, 3, '1/1/4', '8/2/3', scale=3.0),
    brow('fast_g8', '1x1', 3, 1, 40, 7, 9, '1/1/2', '4/2/3'),
    brow('fast_g8', 'k2s3', 8, 7, 2, 16, 16, '2/1/2', '4/2/3', scale=3.0, affine=True),
    brow('fast_g8', 'k2s3', 1, 8, 96, 5, 5, '2/2/2', '4/4/3'),
    brow('fast_g8', 'k2s3', 2, 6, 192, 5, 5, '3/2/2', '4/4/3', G=2, scale=3.0),
    brow('fast_g8', 'k5s3d2', 2, 2, 4, 32, 32, '1/1/2', '4/2/3', G=2, affine=True),
    brow('fast_g8', '5x5s2', 40, 3, 2, 3, 3, '3/1/2', '8/2/3', scale=3.0),
    brow('fast_g8', '1x1p2', 1, 2, 96, 7, 9, '2/2/2', '4/4/3'),
    brow('fast_g8', '1x1', 1, 2, 2, 40, 200, '2/1/2', '4/2/6', scale=3.0, affine=True),
    brow('fast_g8', 'k2s3', 2, 6, 384, 5, 5, '3/3/2', '4/6/3', G=2),
    brow('fast_g8', '1x1', 1, 3, 2, 40, 200, '3/1/2', '4/2/6', scale=3.0),
    brow('fast_g8', '1x1p2', 1, 2, 192, 7, 9, '2/3/2', '4/6/3', affine=True),
    brow('fast_g8', 'k3x1', 8, 3, 192, 4, 4, '3/3/2', '4/6/3', scale=3.0),
    brow('fast_g8', 'k3x1', 1, 1, 40, 40, 200, '1/1/4', '4/2/6'),
    brow('fast_g8', '1x1', 1, 2, 96, 40, 200, '2/2/2', '4/4/6', scale=3.0, affine=True),
    brow('fast_g8', 'k3x1', 1, 1, 96, 40, 200, '1/2/2', '4/4/6'),
    brow('fast_g8', '1x1', 1, 3, 96, 40, 200, '3/2/2', '4/4/6', scale=3.0),
    brow('fast_g8', '1x1', 1, 2, 192, 40, 200, '2/3/2', '4/6/6', affine=True),
    brow('fast_g8', 'k3x1', 1, 1, 192, 40, 200, '1/3/2', '4/6/6', scale=3.0),
    brow('fast_g8', 'd2', 1, 3, 192, 32, 32, '3/3/2', '4/6/6'),
    brow('fast_g8', 'd2', 2, 6, 192, 32, 32, '3/2/2', '4/4/6', G=2, scale=3.0, affine=True),
    brow('fast_g8', 'd2', 2, 6, 384, 32, 32, '3/3/2', '4/6/6', G=2),
    brow('cheby_d4', '1x1', 1, 2, 2, 3, 3, '2/1/4', '4/2/3'),
    brow('cheby_d4', '1x1', 1, 3, 2, 3, 3, '3/1/4', '4/2/3', affine=True),
    brow('cheby_d4', '1x1', 1, 5, 2, 3, 3, '2/1/4', '4/2/3'),
    brow('cheby_d4', '1x1', 3, 3, 2, 3, 3, '3/1/4', '4/2/3'),
    brow('cheby_d4', '5x5s2', 1, 1, 2, 3, 3, '1/1/4', '4/2/3', affine=True),
    brow('cheby_d4', 'p0', 1, 3, 2, 4, 4, '3/1/4', '8/2/3'),
    brow('cheby_d4', 'k2s3', 1, 7, 2, 5, 5, '2/1/4', '4/2/3'),
    brow('cheby_d4', '5x5', 1, 1, 2, 3, 3, '1/1/4', '8/2/3', affine=True),
    brow('cheby_d4', '1x1', 3, 2, 2, 7, 9, '2/1/2', '4/2/3'),
    brow('cheby_d4', 'k7s2', 1, 2, 2, 3, 3, '2/1/4', '8/2/3'),
    brow('cheby_d4', '1x1', 1, 1, 96, 3, 3, '1/2/2', '4/4/3', affine=True),
    brow('cheby_d4', '1x1', 3, 3, 2, 7, 9, '3/1/2', '4/2/3'),
    brow('cheby_d4', '1x1p1', 1, 3, 2, 13, 13, '3/1/2', '4/2/3'),
    brow('cheby_d4', '1x1', 1, 1, 192, 3, 3, '1/3/2', '4/6/3', affine=True),
    brow('cheby_d4', '1x1', 1, 2, 96, 3, 3, '2/2/2', '4/4/3'),
    brow('cheby_d4', '1x1', 3, 5, 2, 7, 9, '2/1/2', '4/2/3'),
    brow('cheby_d4', '1x1', 1, 3, 96, 3, 3, '3/2/2', '4/4/3', affine=True),
    brow('cheby_d4', 'k2s3', 8, 2, 2, 16, 16, '2/1/2', '4/2/3'),
    brow('cheby_d4', 's2', 1, 1, 96, 3, 3, '1/2/2', '4/4/3'),
    brow('cheby_d4', '1x1', 1, 2, 192, 3, 3, '2/3/2', '4/6/3', affine=True),
    brow('cheby_d4', 'k2s3', 1, 3, 96, 5, 5, '3/2/2', '4/4/3'),
    brow('cheby_d4', '1x1', 1, 3, 192, 3, 3, '3/3/2', '4/6/3'),
    brow('cheby_d4', 's2', 1, 1, 192, 3, 3, '1/3/2', '4/6/3', affine=True),
    brow('cheby_d4', '1x1', 3, 1, 40, 7, 9, '1/1/2', '4/2/3'),
    brow('cheby_d4', '1x1p1', 1, 1, 40, 13, 13, '1/1/2', '4/2/3'),
    brow('cheby_d4', '3x3', 1, 3, 2, 13, 13, '3/1/4', '8/2/3', affine=True),
    brow('cheby_d4', 'k2s3', 1, 3, 192, 5, 5, '3/3/2', '4/6/3'),
    brow('cheby_d4', '5x5s2', 1, 1, 96, 3, 3, '1/2/2', '4/4/3'),
    brow('cheby_d4', '5x5s2', 3, 1, 2, 16, 16, '1/1/2', '4/2/3', affine=True),
    brow('cheby_d4', '5x5s2', 1, 1, 192, 3, 3, '1/3/2', '4/6/3'),
    brow('cheby_d4', '1x1', 1, 2, 2, 40, 200, '2/1/2', '4/2/6'),
    brow('cheby_d4', '1x1p2', 1, 3, 96, 7, 9, '3/2/2', '4/4/3', affine=True),
    brow('cheby_d4', '1x1', 1, 3, 2, 40, 200, '3/1/2', '4/2/6'),
    # seed 1: the InstanceNorm runs over 2x2 output planes, and the draw of seed 0 holds a near-constant one -- y missed by 2.7e-5 against a bound
    # of 1.1e-5 (the fp32 oracle itself 2.8e-6, ten times its usual) while the conv stage of the same draw sat at z 3.5e-7 / dW 4.3e-7 (the fp32
    # oracle 2.3e-7 / 3.0e-7); seeds 1 .. 6 give y 2.2e-6 .. 3.5e-6 against the oracle's own 2.2e-6 .. 4.8e-6
    brow('cheby_d4', 'p0', 17, 1, 96, 4, 4, '1/2/2', '4/4/3', seed=1),
    brow('cheby_d4', '1x1', 1, 5, 2, 40, 200, '2/1/2', '4/2/6', affine=True),
    brow('cheby_d4', '1x1p2', 1, 3, 192, 7, 9, '3/3/2', '4/6/3'),
    brow('cheby_d4', 'p0', 17, 1, 192, 4, 4, '1/3/2', '4/6/3'),
    brow('cheby_d4', 'd2', 1, 2, 2, 40, 200, '2/1/4', None, affine=True),
    brow('cheby_d4', 'd2', 8, 3, 96, 4, 4, '3/2/2', '4/4/3'),
    brow('cheby_d4', 'p0', 1, 3, 2, 40, 200, '3/1/4', '8/2/6'),
    brow('cheby_d4', 'd2', 16, 2, 192, 3, 3, '2/3/2', None, affine=True),
    brow('cheby_d4', 'k7s2', 1, 3, 2, 40, 200, '3/1/4', '8/2/6'),
    brow('cheby_d4', 'd2', 8, 3, 192, 4, 4, '3/3/2', '4/6/3'),
    brow('cheby_d4', '5x5', 1, 2, 2, 40, 200, '2/1/4', '8/2/6', affine=True),
    brow('cheby_d4', '1x1', 1, 2, 96, 40, 200, '2/2/2', '4/4/6'),
    brow('cheby_d4', '5x5', 1, 5, 2, 40, 200, '2/1/4', '8/2/6'),
    brow('cheby_d4', '1x1', 1, 3, 96, 40, 200, '3/2/2', '4/4/6', affine=True),
    brow('cheby_d4', 'p0', 1, 1, 40, 40, 200, '1/1/4', '4/2/6'),
    brow('cheby_d4', '1x1', 1, 2, 192, 40, 200, '2/3/2', '4/6/6'),
    brow('cheby_d4', '1x1', 1, 3, 192, 40, 200, '3/3/2', '4/6/6', affine=True),
    brow('cheby_d4', 'p0', 1, 1, 96, 40, 200, '1/2/2', '4/4/6'),
    brow('cheby_d4', 'p0', 1, 1, 192, 40, 200, '1/3/2', '4/6/6'),
    brow('cheby_d3', '1x1', 1, 2, 2, 3, 3, '2/1/4', None, affine=True),
    brow('cheby_d3', '1x1', 1, 3, 2, 3, 3, '3/1/4', None),
    brow('cheby_d3', 'k2s3', 1, 2, 2, 5, 5, '2/1/4', None),
    brow('cheby_d3', '5x5s2', 1, 1, 2, 3, 3, '1/1/4', None, affine=True),
    brow('cheby_d3', '1x1', 3, 2, 2, 7, 9, '2/1/2', None),
    brow('cheby_d3', '1x1p2', 3, 2, 2, 4, 4, '2/1/2', None),
    brow('cheby_d3', '1x1', 1, 1, 96, 3, 3, '1/2/2', None, affine=True),
    brow('cheby_d3', '1x1', 3, 3, 2, 7, 9, '3/1/2', None),
    brow('cheby_d3', '1x1', 1, 1, 192, 3, 3, '1/3/2', None),
    brow('cheby_d3', '1x1', 1, 2, 96, 3, 3, '2/2/2', None, affine=True),
    brow('cheby_d3', '1x1', 1, 3, 96, 3, 3, '3/2/2', None),
    brow('cheby_d3', '1x1', 1, 2, 192, 3, 3, '2/3/2', None),
    brow('cheby_d3', '1x1', 2, 6, 4, 13, 13, '3/1/2', None, G=2, affine=True),
    brow('cheby_d3', 'k2s3', 8, 3, 2, 16, 16, '3/1/2', None),
    brow('cheby_d3', '1x1', 1, 3, 192, 3, 3, '3/3/2', None),
    brow('cheby_d3', 's2', 1, 2, 96, 3, 3, '2/2/2', None, affine=True),
    brow('cheby_d3', 's2', 3, 2, 2, 16, 16, '2/1/2', None),
    brow('cheby_d3', '1x1', 3, 1, 40, 7, 9, '1/1/2', None),
    brow('cheby_d3', 's2', 1, 2, 192, 3, 3, '2/3/2', None, affine=True),
    brow('cheby_d3', 'k2s3', 8, 1, 40, 16, 16, '1/1/2', None),
    brow('cheby_d3', 'k7s2', 40, 3, 2, 3, 3, '3/1/4', None),
    brow('lucas_d3', '1x1', 1, 2, 2, 3, 3, '2/1/4', None, affine=True),
    brow('bessel_d3', '1x1', 1, 3, 2, 3, 3, '3/1/4', None),
    brow('lucas_d3', 'k2s3', 1, 3, 2, 5, 5, '3/1/4', None),
    brow('bessel_d3', '5x5s2', 1, 1, 2, 3, 3, '1/1/4', None, affine=True),
    brow('lucas_d3', 'k2s3', 1, 1, 40, 5, 5, '1/1/4', None),
    brow('bessel_d3', '1x1', 3, 2, 2, 7, 9, '2/1/2', None),
    brow('lucas_d3', '1x1', 1, 1, 96, 3, 3, '1/2/2', None, affine=True),
    brow('bessel_d3', '1x1', 3, 3, 2, 7, 9, '3/1/2', None),
    brow('lucas_d3', '1x1p2', 3, 3, 2, 4, 4, '3/1/2', None),
    brow('bessel_d3', '1x1', 1, 1, 192, 3, 3, '1/3/2', None, affine=True),
    brow('lucas_d3', '1x1', 1, 2, 96, 3, 3, '2/2/2', None),
    brow('bessel_d3', 'k3x1', 8, 3, 2, 4, 4, '3/1/4', None),
    brow('lucas_d3', '1x1', 1, 3, 96, 3, 3, '3/2/2', None, affine=True),
    brow('bessel_d3', '1x1', 3, 1, 96, 3, 3, '1/2/2', None),
    brow('lucas_d3', '1x1', 1, 2, 192, 3, 3, '2/3/2', None),
    brow('bessel_d3', '1x1', 1, 3, 192, 3, 3, '3/3/2', None, affine=True),
    brow('lucas_d3', '1x1', 3, 1, 192, 3, 3, '1/3/2', None),
    brow('bessel_d3', '1x1', 3, 1, 40, 7, 9, '1/1/2', None),
    brow('lucas_d3', '1x1p2', 3, 1, 40, 4, 4, '1/1/2', None, affine=True),
    brow('bessel_d3', '5x5', 3, 1, 2, 8, 8, '1/1/2', None),
    brow('lucas_d3', 's2', 1, 3, 96, 3, 3, '3/2/2', None),
    brow('bessel_d3', 's2', 3, 3, 2, 16, 16, '3/1/2', None, affine=True),
    brow('lucas_d3', 's2', 1, 3, 192, 3, 3, '3/3/2', None),
    brow('bessel_d3', '5x5s2', 1, 3, 96, 3, 3, '3/2/2', None),
    brow('lucas_d3', '5x5s2', 1, 3, 192, 3, 3, '3/3/2', None, affine=True),
]
