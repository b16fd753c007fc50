"""Route cells of the conv-KAN planner: which compile-time spec and which kernel route each of the three stages of a launch takes.

route_key(geom, basis, plan) restates, from the public KanPlan and the KanGeom / KanBasis structs, what plan_conv
(csrc/kan_plan.hip) decides and the launchers (csrc/kanconv.hip, ops.py) run.  ROUTE_CASES holds small layers, at least one per reachable
cell: tests/test_route_matrix.py checks on CPU that every row plans to its declared key and that every cell the planner reaches
has a row; tests/test_gpu_route_matrix.py runs every row against the fp64 oracle and twice for bitwise equality."""
import ctypes

import torch.nn as nn

from convkan_amd import _lib as L

FAST_NAMES = {1: "BSPLINE_SILU", 2: "BSPLINE_GELU", 3: "RBF8", 4: "CHEBY5", 5: "CHEBY4", 6: "POLY4", 7: "POLY3", 8: "RBF5",
              9: "RELU8", 10: "GRAM4", 11: "POLY1"}                         # FAST_* of csrc/kan_internal.h
KIND_NAMES = {L.BASIS_BSPLINE: "BSPLINE", L.BASIS_RBF: "RBF", L.BASIS_CHEBY: "CHEBY", L.BASIS_POLY: "POLY", L.BASIS_FOURIER: "FOURIER",
              L.BASIS_RELU: "RELU", L.BASIS_GRAM: "GRAM"}
DW_T, DW_MAX_TP = 9, 96                                                     # kan_internal.h: DW_T, DW_MAX_TP


def fast_variant(b):
    """FAST_* number of a basis: restates fast_variant() (kan_plan.hip:58)."""
    if b.kind == L.BASIS_BSPLINE and b.n_basis == 8 and b.order == 3:      # kan_plan.hip:59-60
        return 1 if b.act == L.ACT_SILU else 2 if b.act == L.ACT_GELU else 0
    if b.kind == L.BASIS_RBF and b.act == L.ACT_SILU and b.n_basis in (8, 5):          # kan_plan.hip:61
        return 3 if b.n_basis == 8 else 8
    if b.kind == L.BASIS_CHEBY and b.act == L.ACT_NONE:                    # kan_plan.hip:62
        return {5: 4, 4: 5}.get(b.n_basis, 0)
    if b.kind == L.BASIS_POLY and b.act != L.ACT_NONE:                     # kan_plan.hip:63-64
        return {4: 6, 3: 7, 1: 11}.get(b.n_basis, 0)
    if b.kind == L.BASIS_RELU and b.act == L.ACT_SILU and b.n_basis == 8:  # kan_plan.hip:65
        return 9
    if b.kind == L.BASIS_GRAM and b.act == L.ACT_SILU and b.n_basis == 4:  # kan_plan.hip:66
        return 10
    return 0


def spec_class(b):
    """FAST_<name>, or GENERIC:<kind> -- the generic kernels are instantiated once per basis kind (dispatch_kind, kan_internal.h:94)."""
    f = fast_variant(b)
    return f"FAST_{FAST_NAMES[f]}" if f else f"GENERIC:{KIND_NAMES[b.kind]}"


def dw_direct(g, b):
    """Depthwise direct kernels: restates dw_direct() (kan_plan.hip:283)."""
    T, P = g.kh * g.kw, b.n_basis + (b.act != L.ACT_NONE)
    return g.C == 1 and g.O <= 2 and T <= DW_T and T * P <= DW_MAX_TP


def second_input(b):
    """LegendreKAN (recurrence basis of order 0) always hands the kernels a second, pre-normalised tensor; ops.py then makes no
    position-major copy (ops.py:423, ops.py:484) and every launch stays image-major.  (FastKAN also passes one, but the planner
    never offers it a position-major launch: want_pix_major, kan_plan.hip.)"""
    return b.kind == L.BASIS_POLY and b.order == 0


def route_key(g, b, p):
    """(spec class, fwd route, bwd-data route, bwd-weight route) of one launch."""
    if dw_direct(g, b):                                     # kan_plan.hip:377-379: DW takes all three stages
        return spec_class(b), "DW", "DW", "DW"
    pm = not second_input(b)
    if p.fwd_band:                                          # kan_plan.hip:377 (route order: DW, BAND, HALO, EXPANDED, TAP_MAJOR)
        fwd = "BAND"
    elif p.fwd_halo:
        fwd = "HALO+RB" if p.row_blocks & 1 else "HALO"     # kan_plan.hip:453: row_blocks bit 0 = ROWBLK halo forward
    elif p.fwd_expanded:
        fwd = "EXPANDED"
    else:
        fwd = "TAP-PM" if p.fwd_target > 0 and pm else "TAP"        # kan_plan.hip:428: a target only for the position-major launch
    if p.bwd_data_target > 0 and pm:                        # kan_plan.hip:378, 440
        bd = "TAP-PM"
    else:
        bd = "TAP-RB" if p.row_blocks & 2 else "TAP"        # kan_plan.hip:453: bit 1 = row-ordered pixel blocks (image-major only)
    if p.bwd_weight_band:                                   # kan_plan.hip:379
        bw = "BAND"
    elif p.bwd_weight_halo:
        bw = "HALO"
    elif p.bwd_weight_expanded:
        bw = "EXPANDED"
    else:
        bw = "TAP-PM" if p.bwd_weight_target > 0 and pm else "TAP"  # kan_plan.hip:434
    return spec_class(b), fwd, bd, bw


def key_id(key):
    return "-".join(k.replace(":", "_") for k in key)


def plan_of(g, b):
    p = L.KanPlan()
    rc = L.load().kan_plan(ctypes.byref(g), ctypes.byref(b), ctypes.byref(p))
    return p if rc == 0 else None


def stage_splits(p, stage):
    """Split count (slabs) of a stage, from the public plan."""
    return {"fwd": p.fwd_splits, "bd": p.bwd_data_splits, "bw": p.bwd_weight_splits}[stage]


# ---------------------------------------------------------------------------------------------------------------- the case table
# The layers of the rows: (class, constructor kwargs besides in/out/kernel/geometry), one per compile-time spec or generic kind of
# make_plan_snapshot.basis_specs() plus the recurrence families that share their specs.
LAYERS = {
    "kan_silu": ("KANConv2DLayer", dict(base_activation=nn.SiLU)),
    "kan_gelu": ("KANConv2DLayer", dict(base_activation=nn.GELU)),
    "kan_g3o2": ("KANConv2DLayer", dict(grid_size=3, spline_order=2, base_activation=nn.SiLU)),
    "kan_g8o1": ("KANConv2DLayer", dict(grid_size=8, spline_order=1, base_activation=nn.GELU)),
    "fast_g8": ("FastKANConv2DLayer", dict(grid_size=8, base_activation=nn.SiLU)),
    "fast_g5": ("FastKANConv2DLayer", dict(grid_size=5, base_activation=nn.SiLU)),
    "fast_g4_gelu": ("FastKANConv2DLayer", dict(grid_size=4, base_activation=nn.GELU)),
    "cheby_d4": ("ChebyKANConv2DLayer", dict(degree=4)),
    "cheby_d3": ("ChebyKANConv2DLayer", dict(degree=3)),
    "cheby_d6": ("ChebyKANConv2DLayer", dict(degree=6)),
    "lucas_d3": ("LucasKANConv2DLayer", dict(degree=3)),
    "bessel_d3": ("BesselKANConv2DLayer", dict(degree=3)),
    "jacobi_d3": ("JacobiKANConv2DLayer", dict(degree=3, a=1.0, b=1.0)),
    "bersnstein_d3": ("BersnsteinKANConv2DLayer", dict(degree=3)),
    "legendre_d3": ("LegendreKANConv2DLayer", dict(degree=3)),
    "hermite_d2": ("HermiteKANConv2DLayer", dict(degree=2)),
    "fibonacci_d2": ("FibonacciKANConv2DLayer", dict(degree=2)),
    "taylor_d1": ("TaylorKANConv2DLayer", dict(degree=1)),
    "gegen_d5": ("GegenbauerKANConv2DLayer", dict(degree=5, alpha_param=1.0)),
    "laguerre_d5": ("LaguerreKANConv2DLayer", dict(degree=5, alpha=1.0)),
    "legendre_d2": ("LegendreKANConv2DLayer", dict(degree=2)),
    "fourier_g3": ("FourierKANConv2DLayer", dict(grid_size=3)),
    "fourier_g5": ("FourierKANConv2DLayer", dict(grid_size=5)),
    "relu_g5k3": ("ReLUKANConv2DLayer", dict(g=5, k=3)),
    "relu_g3k2": ("ReLUKANConv2DLayer", dict(g=3, k=2)),
    "gram_d3": ("GRAMKANConv2DLayer", dict(degree=3)),
    "gram_d5": ("GRAMKANConv2DLayer", dict(degree=5)),
}
KINDS = {"KANConv2DLayer": "bspline", "FastKANConv2DLayer": "rbf", "ChebyKANConv2DLayer": "cheby", "LucasKANConv2DLayer": "lucas",
         "BesselKANConv2DLayer": "bessel", "JacobiKANConv2DLayer": "jacobi", "BersnsteinKANConv2DLayer": "bersnstein",
         "LegendreKANConv2DLayer": "legendre", "HermiteKANConv2DLayer": "hermite", "FibonacciKANConv2DLayer": "fibonacci",
         "TaylorKANConv2DLayer": "taylor", "GegenbauerKANConv2DLayer": "gegenbauer", "LaguerreKANConv2DLayer": "laguerre",
         "FourierKANConv2DLayer": "fourier", "ReLUKANConv2DLayer": "relu", "GRAMKANConv2DLayer": "gram"}
ORACLE_EXTRA = {"gegenbauer": ("alpha_param",), "laguerre": ("alpha",), "jacobi": ("a", "b")}     # kwargs the oracle needs as well
SHAPES = {"3x3": dict(kernel_size=3, stride=1, padding=1, dilation=1), "1x1": dict(kernel_size=1, stride=1, padding=0, dilation=1),
          "s2": dict(kernel_size=3, stride=2, padding=1, dilation=1), "d2": dict(kernel_size=3, stride=1, padding=2, dilation=2),
          "5x5": dict(kernel_size=5, stride=1, padding=2, dilation=1), "p0": dict(kernel_size=3, stride=1, padding=0, dilation=1),
          "5x5s2": dict(kernel_size=5, stride=2, padding=2, dilation=1), "1x1p2": dict(kernel_size=1, stride=1, padding=2, dilation=1),
          "1x1p1": dict(kernel_size=1, stride=1, padding=1, dilation=1)}


def row(key, layer, shape, B, C, O, H, W=None, G=1, **opts):
    """One ROUTE_CASES row: LAYERS[layer] with the SHAPES[shape] conv geometry, input [B, C, H, W] (C, O: totals over G groups).
    opts: scale (input multiplier: past the grid range), affine (perturbed affine InstanceNorm), perturb (ReLU-KAN phases / GRAM
    beta_weights away from their init)."""
    return dict(key=tuple(key.split()), layer=layer, shape=shape, B=B, C=C, O=O, H=H, W=H if W is None else W, G=G, **opts)


def case_layer(case):
    import convkan_amd as K
    cls, kw = LAYERS[case["layer"]]
    kw = dict(kw, groups=case["G"], **SHAPES[case["shape"]])
    if case.get("affine"):
        kw["affine"] = True
    return getattr(K, cls)(case["C"], case["O"], **kw)


def case_structs(case, layer=None):
    """(KanGeom, KanBasis, KanPlan) of the row's layer on its input, as ops.py plans it."""
    from convkan_amd import ops
    layer = case_layer(case) if layer is None else layer
    G = case["G"]
    return ops._plan_cached(layer.conv_spec(), case["B"], case["C"] // G, case["H"], case["W"], case["O"] // G, case["C"], case["O"])


def case_cfg(case, layer):
    """The oracle config of helpers.oracle_forward for the row's layer."""
    cls, kw = LAYERS[case["layer"]]
    kind = KINDS[cls]
    s = SHAPES[case["shape"]]
    cfg = dict(kind=kind, C=case["C"], O=case["O"], k=s["kernel_size"], s=s["stride"], p=s["padding"], d=s["dilation"], groups=case["G"],
               extra={n: kw[n] for n in ORACLE_EXTRA.get(kind, ())})
    act = getattr(layer, "base_activation", None)
    if act is not None and not isinstance(act, type):
        act = type(act)
    names = {nn.SiLU: "silu", nn.GELU: "gelu", nn.ReLU: "relu", nn.Tanh: "tanh", nn.Sigmoid: "sigmoid", nn.Identity: "none"}
    if act is not None:
        cfg["act"] = names[act]
    return cfg


# One row per cell the planner reaches (tests/test_route_matrix.py keeps the list complete, and its grid reaches every cell listed),
# the cheapest layer that reaches it, with the recurrence families of one compile-time spec taking turns; plus rows that give every
# (stage, route) a grouped launch and both a single-slab and a split-K launch where the planner makes both, and LegendreKAN rows
# (second input tensor: image-major launches where the plan offers position-major ones).  Rows of the B-spline, FastKAN and ReLU-KAN bases alternate inputs scaled 3x past their grid range; every third row has a
# perturbed affine InstanceNorm; ReLU-KAN phases and GRAM-KAN beta weights are always perturbed (tests/test_gpu_route_matrix.py).
# A row whose PReLU-slope gradient cancels to near zero (the fp32 oracle itself then misses fp64 by ~1e-5) gets another batch, not a
# wider tolerance: FAST_BSPLINE_SILU HALO TAP-RB EXPANDED runs 32 images (16 summed its slope gradient to -0.44 from ~3e4 terms).
ROUTE_CASES = [
    # FAST_BSPLINE_GELU
    row('FAST_BSPLINE_GELU BAND TAP BAND', 'kan_gelu', '3x3', 17, 6, 2, 5, G=2, scale=3.0),
    row('FAST_BSPLINE_GELU BAND TAP EXPANDED', 'kan_gelu', '3x3', 16, 128, 96, 3, affine=True),
    row('FAST_BSPLINE_GELU BAND TAP HALO', 'kan_gelu', '3x3', 256, 2, 192, 16, G=2, scale=3.0),
    row('FAST_BSPLINE_GELU BAND TAP TAP', 'kan_gelu', '5x5s2', 17, 2, 1024, 32, G=2),
    row('FAST_BSPLINE_GELU BAND TAP TAP-PM', 'kan_gelu', '3x3', 17, 6, 2, 3, G=2, scale=3.0, affine=True),
    row('FAST_BSPLINE_GELU BAND TAP-PM BAND', 'kan_gelu', '1x1p2', 17, 2, 32, 2, G=2),
    row('FAST_BSPLINE_GELU BAND TAP-PM TAP', 'kan_gelu', '1x1p2', 17, 1024, 384, 2, G=2, scale=3.0),
    row('FAST_BSPLINE_GELU BAND TAP-PM TAP-PM', 'kan_gelu', '1x1p1', 17, 2, 32, 2, G=2, affine=True),
    row('FAST_BSPLINE_GELU BAND TAP-RB BAND', 'kan_gelu', '3x3', 8, 2, 32, 4, G=2, scale=3.0),
    row('FAST_BSPLINE_GELU BAND TAP-RB EXPANDED', 'kan_gelu', '3x3', 16, 128, 96, 4),
    row('FAST_BSPLINE_GELU BAND TAP-RB HALO', 'kan_gelu', '3x3', 16, 1, 96, 4, scale=3.0, affine=True),
    row('FAST_BSPLINE_GELU BAND TAP-RB TAP', 'kan_gelu', '3x3', 8, 1024, 192, 4, G=2),
    row('FAST_BSPLINE_GELU BAND TAP-RB TAP-PM', 'kan_gelu', '3x3', 16, 1, 16, 4, scale=3.0),
    row('FAST_BSPLINE_GELU DW DW DW', 'kan_gelu', '3x3', 17, 2, 2, 2, G=2),
    row('FAST_BSPLINE_GELU EXPANDED TAP EXPANDED', 'kan_gelu', 's2', 128, 128, 96, 3, scale=3.0),
    row('FAST_BSPLINE_GELU EXPANDED TAP TAP-PM', 'kan_gelu', 's2', 128, 2, 96, 3),
    row('FAST_BSPLINE_GELU EXPANDED TAP-PM EXPANDED', 'kan_gelu', '3x3', 128, 128, 96, 2, scale=3.0, affine=True),
    row('FAST_BSPLINE_GELU EXPANDED TAP-PM TAP-PM', 'kan_gelu', '3x3', 128, 2, 96, 2),
    row('FAST_BSPLINE_GELU HALO TAP HALO', 'kan_gelu', '3x3', 2, 2, 128, 4, scale=3.0),
    row('FAST_BSPLINE_GELU HALO TAP TAP', 'kan_gelu', '3x3', 1, 2, 128, 4, affine=True),
    row('FAST_BSPLINE_GELU HALO TAP TAP-PM', 'kan_gelu', '3x3', 17, 2, 128, 4, scale=3.0),
    row('FAST_BSPLINE_GELU HALO TAP-RB EXPANDED', 'kan_gelu', '3x3', 16, 128, 128, 4),
    row('FAST_BSPLINE_GELU HALO TAP-RB HALO', 'kan_gelu', '3x3', 8, 2, 128, 4, scale=3.0, affine=True),
    row('FAST_BSPLINE_GELU HALO TAP-RB TAP', 'kan_gelu', '3x3', 8, 512, 128, 4),
    row('FAST_BSPLINE_GELU HALO+RB TAP HALO', 'kan_gelu', '3x3', 2, 2, 256, 4, scale=3.0),
    row('FAST_BSPLINE_GELU HALO+RB TAP TAP', 'kan_gelu', '3x3', 1, 2, 256, 4, affine=True),
    row('FAST_BSPLINE_GELU HALO+RB TAP TAP-PM', 'kan_gelu', '3x3', 17, 2, 256, 4, scale=3.0),
    row('FAST_BSPLINE_GELU HALO+RB TAP-RB EXPANDED', 'kan_gelu', '3x3', 16, 128, 256, 4),
    row('FAST_BSPLINE_GELU HALO+RB TAP-RB HALO', 'kan_gelu', '3x3', 8, 2, 256, 4, scale=3.0, affine=True),
    row('FAST_BSPLINE_GELU HALO+RB TAP-RB TAP', 'kan_gelu', '3x3', 8, 512, 256, 4),
    row('FAST_BSPLINE_GELU TAP TAP HALO', 'kan_gelu', '3x3', 2, 5, 96, 4, scale=3.0),
    row('FAST_BSPLINE_GELU TAP TAP TAP', 'kan_gelu', '1x1', 17, 5, 96, 2, affine=True),
    row('FAST_BSPLINE_GELU TAP TAP TAP-PM', 'kan_gelu', 'd2', 17, 6, 2, 3, G=2, scale=3.0),
    row('FAST_BSPLINE_GELU TAP TAP-PM EXPANDED', 'kan_gelu', '1x1p1', 16, 128, 96, 2),
    row('FAST_BSPLINE_GELU TAP TAP-PM TAP', 'kan_gelu', '1x1p2', 17, 5, 96, 2, scale=3.0, affine=True),
    row('FAST_BSPLINE_GELU TAP TAP-PM TAP-PM', 'kan_gelu', '1x1p1', 17, 5, 96, 2),
    row('FAST_BSPLINE_GELU TAP TAP-RB HALO', 'kan_gelu', '3x3', 8, 5, 96, 4, scale=3.0),
    row('FAST_BSPLINE_GELU TAP-PM TAP EXPANDED', 'kan_gelu', 's2', 16, 128, 96, 3, affine=True),
    row('FAST_BSPLINE_GELU TAP-PM TAP TAP-PM', 'kan_gelu', 's2', 17, 2, 32, 3, G=2, scale=3.0),
    row('FAST_BSPLINE_GELU TAP-PM TAP-PM EXPANDED', 'kan_gelu', '3x3', 16, 128, 96, 2),
    row('FAST_BSPLINE_GELU TAP-PM TAP-PM TAP-PM', 'kan_gelu', '3x3', 17, 2, 32, 2, G=2, scale=3.0, affine=True),
    # FAST_BSPLINE_SILU
    row('FAST_BSPLINE_SILU BAND TAP BAND', 'kan_silu', '3x3', 17, 6, 2, 5, G=2),
    row('FAST_BSPLINE_SILU BAND TAP EXPANDED', 'kan_silu', '3x3', 16, 128, 96, 3, scale=3.0),
    row('FAST_BSPLINE_SILU BAND TAP HALO', 'kan_silu', '3x3', 256, 2, 192, 16, G=2, affine=True),
    row('FAST_BSPLINE_SILU BAND TAP TAP', 'kan_silu', '5x5s2', 17, 2, 1024, 32, G=2, scale=3.0),
    row('FAST_BSPLINE_SILU BAND TAP TAP-PM', 'kan_silu', '3x3', 17, 6, 2, 3, G=2),
    row('FAST_BSPLINE_SILU BAND TAP-PM BAND', 'kan_silu', '1x1p2', 17, 2, 32, 2, G=2, scale=3.0, affine=True),
    row('FAST_BSPLINE_SILU BAND TAP-PM TAP', 'kan_silu', '1x1p2', 17, 1024, 384, 2, G=2),
    row('FAST_BSPLINE_SILU BAND TAP-PM TAP-PM', 'kan_silu', '1x1p1', 17, 2, 32, 2, G=2, scale=3.0),
    row('FAST_BSPLINE_SILU BAND TAP-RB BAND', 'kan_silu', '3x3', 8, 2, 32, 4, G=2, affine=True),
    row('FAST_BSPLINE_SILU BAND TAP-RB EXPANDED', 'kan_silu', '3x3', 16, 128, 96, 4, scale=3.0),
    row('FAST_BSPLINE_SILU BAND TAP-RB HALO', 'kan_silu', '3x3', 16, 1, 96, 4),
    row('FAST_BSPLINE_SILU BAND TAP-RB TAP', 'kan_silu', '3x3', 8, 1024, 192, 4, G=2, scale=3.0, affine=True),
    row('FAST_BSPLINE_SILU BAND TAP-RB TAP-PM', 'kan_silu', '3x3', 16, 1, 16, 4),
    row('FAST_BSPLINE_SILU DW DW DW', 'kan_silu', '3x3', 17, 2, 2, 2, G=2, scale=3.0),
    row('FAST_BSPLINE_SILU EXPANDED TAP EXPANDED', 'kan_silu', 's2', 128, 128, 96, 3, affine=True),
    row('FAST_BSPLINE_SILU EXPANDED TAP TAP-PM', 'kan_silu', 's2', 128, 2, 96, 3, scale=3.0),
    row('FAST_BSPLINE_SILU EXPANDED TAP-PM EXPANDED', 'kan_silu', '3x3', 128, 128, 96, 2),
    row('FAST_BSPLINE_SILU EXPANDED TAP-PM TAP-PM', 'kan_silu', '3x3', 128, 2, 96, 2, scale=3.0, affine=True),
    row('FAST_BSPLINE_SILU HALO TAP HALO', 'kan_silu', '3x3', 2, 2, 128, 4),
    row('FAST_BSPLINE_SILU HALO TAP TAP', 'kan_silu', '3x3', 1, 2, 128, 4, scale=3.0),
    row('FAST_BSPLINE_SILU HALO TAP TAP-PM', 'kan_silu', '3x3', 17, 2, 128, 4, affine=True),
    row('FAST_BSPLINE_SILU HALO TAP-RB EXPANDED', 'kan_silu', '3x3', 32, 128, 128, 4, scale=3.0),
    row('FAST_BSPLINE_SILU HALO TAP-RB HALO', 'kan_silu', '3x3', 8, 2, 128, 4),
    row('FAST_BSPLINE_SILU HALO TAP-RB TAP', 'kan_silu', '3x3', 8, 512, 128, 4, scale=3.0, affine=True),
    row('FAST_BSPLINE_SILU HALO+RB TAP HALO', 'kan_silu', '3x3', 2, 2, 256, 4),
    row('FAST_BSPLINE_SILU HALO+RB TAP TAP', 'kan_silu', '3x3', 1, 2, 256, 4, scale=3.0),
    row('FAST_BSPLINE_SILU HALO+RB TAP TAP-PM', 'kan_silu', '3x3', 17, 2, 256, 4, affine=True),
    row('FAST_BSPLINE_SILU HALO+RB TAP-RB EXPANDED', 'kan_silu', '3x3', 16, 128, 256, 4, scale=3.0),
    row('FAST_BSPLINE_SILU HALO+RB TAP-RB HALO', 'kan_silu', '3x3', 8, 2, 256, 4),
    row('FAST_BSPLINE_SILU HALO+RB TAP-RB TAP', 'kan_silu', '3x3', 8, 512, 256, 4, scale=3.0, affine=True),
    row('FAST_BSPLINE_SILU TAP TAP HALO', 'kan_silu', '3x3', 2, 5, 96, 4),
    row('FAST_BSPLINE_SILU TAP TAP TAP', 'kan_silu', '1x1', 17, 5, 96, 2, scale=3.0),
    row('FAST_BSPLINE_SILU TAP TAP TAP-PM', 'kan_silu', 'd2', 17, 6, 2, 3, G=2, affine=True),
    row('FAST_BSPLINE_SILU TAP TAP-PM EXPANDED', 'kan_silu', '1x1p1', 16, 128, 96, 2, scale=3.0),
    row('FAST_BSPLINE_SILU TAP TAP-PM TAP', 'kan_silu', '1x1p2', 17, 5, 96, 2),
    row('FAST_BSPLINE_SILU TAP TAP-PM TAP-PM', 'kan_silu', '1x1p1', 17, 5, 96, 2, scale=3.0, affine=True),
    row('FAST_BSPLINE_SILU TAP TAP-RB HALO', 'kan_silu', '3x3', 8, 5, 96, 4),
    row('FAST_BSPLINE_SILU TAP-PM TAP EXPANDED', 'kan_silu', 's2', 16, 128, 96, 3, scale=3.0),
    row('FAST_BSPLINE_SILU TAP-PM TAP TAP-PM', 'kan_silu', 's2', 17, 2, 32, 3, G=2, affine=True),
    row('FAST_BSPLINE_SILU TAP-PM TAP-PM EXPANDED', 'kan_silu', '3x3', 16, 128, 96, 2, scale=3.0),
    row('FAST_BSPLINE_SILU TAP-PM TAP-PM TAP-PM', 'kan_silu', '3x3', 17, 2, 32, 2, G=2),
    # FAST_CHEBY4
    row('FAST_CHEBY4 BAND TAP TAP', 'cheby_d3', '3x3', 17, 6, 2, 5, G=2, affine=True),
    row('FAST_CHEBY4 BAND TAP TAP-PM', 'cheby_d3', '3x3', 17, 2, 32, 3, G=2),
    row('FAST_CHEBY4 BAND TAP-PM TAP', 'cheby_d3', '1x1p2', 17, 2, 32, 2, G=2),
    row('FAST_CHEBY4 BAND TAP-PM TAP-PM', 'cheby_d3', '1x1p1', 17, 2, 32, 2, G=2, affine=True),
    row('FAST_CHEBY4 DW DW DW', 'cheby_d3', '3x3', 17, 2, 2, 2, G=2),
    row('FAST_CHEBY4 HALO TAP TAP', 'cheby_d3', '3x3', 1, 4, 256, 4, G=2),
    row('FAST_CHEBY4 HALO TAP TAP-PM', 'cheby_d3', '3x3', 17, 2, 128, 4, affine=True),
    row('FAST_CHEBY4 TAP TAP TAP', 'cheby_d3', '1x1', 17, 10, 192, 2, G=2),
    row('FAST_CHEBY4 TAP TAP TAP-PM', 'cheby_d3', 'd2', 32, 6, 2, 3, G=2),
    row('FAST_CHEBY4 TAP TAP-PM TAP', 'cheby_d3', '1x1p2', 17, 5, 96, 2, affine=True),
    row('FAST_CHEBY4 TAP TAP-PM TAP-PM', 'cheby_d3', '1x1p1', 17, 5, 96, 2),
    row('FAST_CHEBY4 TAP-PM TAP TAP-PM', 'cheby_d3', 's2', 17, 2, 32, 3, G=2),
    row('FAST_CHEBY4 TAP-PM TAP-PM TAP-PM', 'cheby_d3', '3x3', 17, 2, 32, 2, G=2, affine=True),
    # FAST_CHEBY5
    row('FAST_CHEBY5 BAND TAP BAND', 'cheby_d4', '1x1', 1, 2, 1, 2),
    row('FAST_CHEBY5 BAND TAP BAND', 'cheby_d4', '3x3', 17, 6, 2, 5, G=2),
    row('FAST_CHEBY5 BAND TAP TAP', 'cheby_d4', '3x3', 17, 32, 80, 32, G=2, affine=True),
    row('FAST_CHEBY5 BAND TAP TAP-PM', 'cheby_d4', '3x3', 17, 2, 32, 3, G=2),
    row('FAST_CHEBY5 BAND TAP-PM BAND', 'cheby_d4', '1x1p2', 17, 2, 32, 2, G=2),
    row('FAST_CHEBY5 BAND TAP-PM TAP', 'cheby_d4', '1x1p2', 256, 1024, 80, 2, G=2, affine=True),
    row('FAST_CHEBY5 BAND TAP-PM TAP-PM', 'cheby_d4', '1x1p1', 17, 2, 32, 2, G=2),
    row('FAST_CHEBY5 DW DW DW', 'cheby_d4', '3x3', 17, 2, 2, 2, G=2),
    row('FAST_CHEBY5 TAP TAP TAP', 'cheby_d4', '1x1', 17, 10, 192, 2, G=2, affine=True),
    row('FAST_CHEBY5 TAP TAP TAP-PM', 'cheby_d4', 'd2', 32, 6, 2, 3, G=2),
    row('FAST_CHEBY5 TAP TAP-PM TAP', 'cheby_d4', '1x1p2', 17, 5, 96, 2),
    row('FAST_CHEBY5 TAP TAP-PM TAP-PM', 'cheby_d4', '1x1p1', 17, 5, 96, 2, affine=True),
    row('FAST_CHEBY5 TAP-PM TAP TAP-PM', 'cheby_d4', 's2', 17, 2, 32, 3, G=2),
    row('FAST_CHEBY5 TAP-PM TAP-PM TAP-PM', 'cheby_d4', '3x3', 17, 2, 32, 2, G=2),
    # FAST_GRAM4
    row('FAST_GRAM4 DW DW DW', 'gram_d3', '3x3', 17, 2, 2, 2, G=2),
    row('FAST_GRAM4 HALO TAP EXPANDED', 'gram_d3', '3x3', 16, 128, 128, 4),
    row('FAST_GRAM4 HALO TAP HALO', 'gram_d3', '3x3', 2, 2, 128, 4),
    row('FAST_GRAM4 HALO TAP TAP', 'gram_d3', '3x3', 1, 4, 256, 4, G=2, affine=True),
    row('FAST_GRAM4 HALO TAP TAP-PM', 'gram_d3', '3x3', 17, 2, 128, 4),
    row('FAST_GRAM4 TAP TAP EXPANDED', 'gram_d3', '3x3', 16, 128, 96, 3),
    row('FAST_GRAM4 TAP TAP HALO', 'gram_d3', '3x3', 2, 2, 192, 4, G=2, affine=True),
    row('FAST_GRAM4 TAP TAP TAP', 'gram_d3', '3x3', 17, 6, 2, 5, G=2),
    row('FAST_GRAM4 TAP TAP TAP-PM', 'gram_d3', '3x3', 17, 2, 32, 3, G=2),
    row('FAST_GRAM4 TAP TAP-PM EXPANDED', 'gram_d3', '1x1p1', 16, 128, 96, 2, affine=True),
    row('FAST_GRAM4 TAP TAP-PM TAP', 'gram_d3', '1x1p2', 17, 2, 32, 2, G=2),
    row('FAST_GRAM4 TAP TAP-PM TAP-PM', 'gram_d3', '1x1p1', 17, 2, 32, 2, G=2),
    row('FAST_GRAM4 TAP-PM TAP EXPANDED', 'gram_d3', 's2', 16, 128, 96, 3, affine=True),
    row('FAST_GRAM4 TAP-PM TAP TAP-PM', 'gram_d3', 's2', 17, 2, 32, 3, G=2),
    row('FAST_GRAM4 TAP-PM TAP-PM EXPANDED', 'gram_d3', '3x3', 16, 128, 96, 2),
    row('FAST_GRAM4 TAP-PM TAP-PM EXPANDED', 'gram_d3', '3x3', 16, 256, 192, 2, G=2, affine=True),
    row('FAST_GRAM4 TAP-PM TAP-PM TAP-PM', 'gram_d3', '3x3', 17, 2, 32, 2, G=2),
    # FAST_POLY1
    row('FAST_POLY1 DW DW DW', 'taylor_d1', '3x3', 17, 2, 2, 2, G=2),
    row('FAST_POLY1 TAP TAP TAP', 'taylor_d1', '3x3', 17, 2, 32, 5, G=2, affine=True),
    row('FAST_POLY1 TAP TAP TAP-PM', 'taylor_d1', '3x3', 17, 2, 32, 3, G=2),
    row('FAST_POLY1 TAP TAP-PM TAP', 'taylor_d1', '1x1p2', 17, 2, 32, 2, G=2),
    row('FAST_POLY1 TAP TAP-PM TAP-PM', 'taylor_d1', '1x1p1', 17, 2, 32, 2, G=2, affine=True),
    row('FAST_POLY1 TAP-PM TAP TAP-PM', 'taylor_d1', 's2', 17, 2, 32, 3, G=2),
    row('FAST_POLY1 TAP-PM TAP-PM TAP-PM', 'taylor_d1', '3x3', 17, 2, 32, 2, G=2),
    # FAST_POLY3
    row('FAST_POLY3 DW DW DW', 'hermite_d2', '3x3', 17, 2, 2, 2, G=2),
    row('FAST_POLY3 TAP TAP TAP', 'fibonacci_d2', '3x3', 17, 6, 2, 5, G=2),
    row('FAST_POLY3 TAP TAP TAP-PM', 'hermite_d2', '3x3', 17, 2, 32, 3, G=2),
    row('FAST_POLY3 TAP TAP-PM TAP', 'fibonacci_d2', '1x1p2', 17, 2, 32, 2, G=2, affine=True),
    row('FAST_POLY3 TAP TAP-PM TAP-PM', 'hermite_d2', '1x1p1', 17, 2, 32, 2, G=2),
    row('FAST_POLY3 TAP-PM TAP TAP-PM', 'fibonacci_d2', 's2', 17, 2, 32, 3, G=2),
    row('FAST_POLY3 TAP-PM TAP-PM TAP-PM', 'hermite_d2', '3x3', 17, 2, 32, 2, G=2, affine=True),
    # FAST_POLY4
    row('FAST_POLY4 BAND TAP TAP', 'lucas_d3', '3x3', 17, 6, 2, 5, G=2),
    row('FAST_POLY4 BAND TAP TAP-PM', 'bessel_d3', '3x3', 17, 2, 32, 3, G=2),
    row('FAST_POLY4 BAND TAP-PM TAP', 'jacobi_d3', '1x1p2', 17, 2, 32, 2, G=2, affine=True),
    row('FAST_POLY4 BAND TAP-PM TAP-PM', 'bersnstein_d3', '1x1p1', 17, 2, 32, 2, G=2),
    row('FAST_POLY4 DW DW DW', 'lucas_d3', '3x3', 17, 2, 2, 2, G=2),
    row('FAST_POLY4 HALO TAP TAP', 'bessel_d3', '3x3', 1, 4, 256, 4, G=2, affine=True),
    row('FAST_POLY4 HALO TAP TAP-PM', 'jacobi_d3', '3x3', 17, 2, 128, 4),
    row('FAST_POLY4 HALO+RB TAP TAP', 'bersnstein_d3', '3x3', 1, 2, 256, 4),
    row('FAST_POLY4 HALO+RB TAP TAP', 'lucas_d3', '3x3', 1, 4, 512, 4, G=2, affine=True),
    row('FAST_POLY4 HALO+RB TAP TAP-PM', 'bessel_d3', '3x3', 17, 2, 256, 4),
    row('FAST_POLY4 TAP TAP TAP', 'jacobi_d3', '1x1', 17, 10, 192, 2, G=2),
    row('FAST_POLY4 TAP TAP TAP-PM', 'bersnstein_d3', 'd2', 32, 6, 2, 3, G=2, affine=True),
    row('FAST_POLY4 TAP TAP-PM TAP', 'lucas_d3', '1x1p2', 17, 5, 96, 2),
    row('FAST_POLY4 TAP TAP-PM TAP-PM', 'bessel_d3', '1x1p1', 17, 5, 96, 2),
    row('FAST_POLY4 TAP-PM TAP TAP-PM', 'jacobi_d3', 's2', 17, 2, 32, 3, G=2, affine=True),
    row('FAST_POLY4 TAP-PM TAP-PM TAP-PM', 'bersnstein_d3', '3x3', 17, 2, 32, 2, G=2),
    # FAST_RBF5
    row('FAST_RBF5 DW DW DW', 'fast_g5', '3x3', 17, 2, 2, 2, G=2, scale=3.0),
    row('FAST_RBF5 TAP TAP TAP', 'fast_g5', '3x3', 17, 2, 32, 2, G=2, affine=True),
    # FAST_RBF8
    row('FAST_RBF8 BAND TAP BAND', 'fast_g8', '3x3', 17, 2, 32, 2, G=2, scale=3.0),
    row('FAST_RBF8 BAND TAP TAP', 'fast_g8', '5x5s2', 17, 2, 1024, 32, G=2),
    row('FAST_RBF8 DW DW DW', 'fast_g8', '3x3', 17, 2, 2, 2, G=2, scale=3.0),
    row('FAST_RBF8 TAP TAP TAP', 'fast_g8', 'd2', 17, 6, 2, 2, G=2),
    # FAST_RELU8
    row('FAST_RELU8 DW DW DW', 'relu_g5k3', '3x3', 17, 2, 2, 2, G=2, scale=3.0),
    row('FAST_RELU8 EXPANDED TAP EXPANDED', 'relu_g5k3', 's2', 128, 128, 96, 3, affine=True),
    row('FAST_RELU8 EXPANDED TAP TAP-PM', 'relu_g5k3', 's2', 128, 2, 96, 3, scale=3.0),
    row('FAST_RELU8 EXPANDED TAP-PM EXPANDED', 'relu_g5k3', '3x3', 128, 128, 96, 2),
    row('FAST_RELU8 EXPANDED TAP-PM TAP-PM', 'relu_g5k3', '3x3', 128, 2, 96, 2, scale=3.0, affine=True),
    row('FAST_RELU8 EXPANDED TAP-PM TAP-PM', 'relu_g5k3', '3x3', 128, 4, 192, 2, G=2),
    row('FAST_RELU8 HALO TAP EXPANDED', 'relu_g5k3', '3x3', 16, 128, 128, 4, scale=3.0),
    row('FAST_RELU8 HALO TAP HALO', 'relu_g5k3', '3x3', 2, 2, 128, 4, affine=True),
    row('FAST_RELU8 HALO TAP TAP', 'relu_g5k3', '3x3', 1, 2, 128, 4, scale=3.0),
    row('FAST_RELU8 HALO TAP TAP-PM', 'relu_g5k3', '3x3', 17, 2, 128, 4),
    row('FAST_RELU8 TAP TAP EXPANDED', 'relu_g5k3', '3x3', 16, 128, 96, 3, scale=3.0, affine=True),
    row('FAST_RELU8 TAP TAP HALO', 'relu_g5k3', '3x3', 2, 2, 192, 4, G=2),
    row('FAST_RELU8 TAP TAP TAP', 'relu_g5k3', '3x3', 17, 6, 2, 5, G=2, scale=3.0),
    row('FAST_RELU8 TAP TAP TAP-PM', 'relu_g5k3', '3x3', 17, 6, 2, 3, G=2, affine=True),
    row('FAST_RELU8 TAP TAP-PM EXPANDED', 'relu_g5k3', '1x1p1', 16, 128, 96, 2, scale=3.0),
    row('FAST_RELU8 TAP TAP-PM TAP', 'relu_g5k3', '1x1p2', 17, 2, 32, 2, G=2),
    row('FAST_RELU8 TAP TAP-PM TAP-PM', 'relu_g5k3', '1x1p1', 17, 2, 32, 2, G=2, scale=3.0, affine=True),
    row('FAST_RELU8 TAP-PM TAP EXPANDED', 'relu_g5k3', 's2', 16, 128, 96, 3),
    row('FAST_RELU8 TAP-PM TAP TAP-PM', 'relu_g5k3', 's2', 17, 2, 32, 3, G=2, scale=3.0),
    row('FAST_RELU8 TAP-PM TAP-PM EXPANDED', 'relu_g5k3', '3x3', 16, 128, 96, 2, affine=True),
    row('FAST_RELU8 TAP-PM TAP-PM TAP-PM', 'relu_g5k3', '3x3', 17, 2, 32, 2, G=2, scale=3.0),
    # GENERIC:BSPLINE
    row('GENERIC:BSPLINE DW DW DW', 'kan_g3o2', '3x3', 17, 2, 2, 2, G=2),
    row('GENERIC:BSPLINE TAP TAP TAP', 'kan_g8o1', '3x3', 17, 6, 2, 5, G=2, scale=3.0, affine=True),
    row('GENERIC:BSPLINE TAP TAP TAP-PM', 'kan_g3o2', '3x3', 17, 2, 32, 3, G=2),
    row('GENERIC:BSPLINE TAP TAP-PM TAP', 'kan_g8o1', '1x1p2', 17, 2, 32, 2, G=2, scale=3.0),
    row('GENERIC:BSPLINE TAP TAP-PM TAP-PM', 'kan_g3o2', '1x1p1', 17, 2, 32, 2, G=2, affine=True),
    row('GENERIC:BSPLINE TAP-PM TAP TAP-PM', 'kan_g8o1', 's2', 17, 2, 32, 3, G=2, scale=3.0),
    row('GENERIC:BSPLINE TAP-PM TAP-PM TAP-PM', 'kan_g3o2', '3x3', 17, 2, 32, 2, G=2),
    # GENERIC:CHEBY
    row('GENERIC:CHEBY DW DW DW', 'cheby_d6', '3x3', 17, 2, 2, 2, G=2),
    row('GENERIC:CHEBY TAP TAP TAP', 'cheby_d6', '3x3', 17, 6, 2, 5, G=2),
    row('GENERIC:CHEBY TAP TAP TAP-PM', 'cheby_d6', '3x3', 17, 2, 32, 3, G=2),
    row('GENERIC:CHEBY TAP TAP-PM TAP', 'cheby_d6', '1x1p2', 17, 2, 32, 2, G=2, affine=True),
    row('GENERIC:CHEBY TAP TAP-PM TAP-PM', 'cheby_d6', '1x1p1', 17, 2, 32, 2, G=2),
    row('GENERIC:CHEBY TAP-PM TAP TAP-PM', 'cheby_d6', 's2', 17, 2, 32, 3, G=2),
    row('GENERIC:CHEBY TAP-PM TAP-PM TAP-PM', 'cheby_d6', '3x3', 17, 2, 32, 2, G=2, affine=True),
    # GENERIC:FOURIER
    row('GENERIC:FOURIER DW DW DW', 'fourier_g3', '3x3', 17, 2, 2, 2, G=2),
    row('GENERIC:FOURIER TAP TAP TAP', 'fourier_g5', '3x3', 17, 6, 2, 5, G=2),
    row('GENERIC:FOURIER TAP TAP TAP-PM', 'fourier_g3', '3x3', 17, 2, 32, 3, G=2, affine=True),
    row('GENERIC:FOURIER TAP TAP-PM TAP', 'fourier_g5', '1x1p2', 17, 2, 32, 2, G=2),
    row('GENERIC:FOURIER TAP TAP-PM TAP-PM', 'fourier_g3', '1x1p1', 17, 2, 32, 2, G=2),
    row('GENERIC:FOURIER TAP-PM TAP TAP-PM', 'fourier_g5', 's2', 17, 2, 32, 3, G=2, affine=True),
    row('GENERIC:FOURIER TAP-PM TAP-PM TAP-PM', 'fourier_g3', '3x3', 17, 2, 32, 2, G=2),
    # GENERIC:GRAM
    row('GENERIC:GRAM DW DW DW', 'gram_d5', '3x3', 17, 2, 2, 2, G=2),
    row('GENERIC:GRAM TAP TAP TAP', 'gram_d5', '3x3', 17, 6, 2, 5, G=2, affine=True),
    row('GENERIC:GRAM TAP TAP TAP-PM', 'gram_d5', '3x3', 17, 2, 32, 3, G=2),
    row('GENERIC:GRAM TAP TAP-PM TAP', 'gram_d5', '1x1p2', 17, 2, 32, 2, G=2),
    row('GENERIC:GRAM TAP TAP-PM TAP-PM', 'gram_d5', '1x1p1', 17, 2, 32, 2, G=2, affine=True),
    row('GENERIC:GRAM TAP-PM TAP TAP-PM', 'gram_d5', 's2', 17, 2, 32, 3, G=2),
    row('GENERIC:GRAM TAP-PM TAP-PM TAP-PM', 'gram_d5', '3x3', 17, 2, 32, 2, G=2),
    # GENERIC:POLY
    row('GENERIC:POLY DW DW DW', 'gegen_d5', '3x3', 17, 2, 2, 2, G=2),
    row('GENERIC:POLY TAP TAP TAP', 'laguerre_d5', '3x3', 17, 6, 2, 5, G=2),
    row('GENERIC:POLY TAP TAP TAP-PM', 'gegen_d5', '3x3', 17, 2, 32, 3, G=2),
    row('GENERIC:POLY TAP TAP-PM TAP', 'laguerre_d5', '1x1p2', 17, 2, 32, 2, G=2, affine=True),
    row('GENERIC:POLY TAP TAP-PM TAP-PM', 'gegen_d5', '1x1p1', 17, 2, 32, 2, G=2),
    row('GENERIC:POLY TAP-PM TAP TAP-PM', 'laguerre_d5', 's2', 17, 2, 32, 3, G=2),
    row('GENERIC:POLY TAP-PM TAP-PM TAP-PM', 'gegen_d5', '3x3', 17, 2, 32, 2, G=2, affine=True),
    # GENERIC:RBF
    row('GENERIC:RBF DW DW DW', 'fast_g4_gelu', '3x3', 17, 2, 2, 2, G=2, scale=3.0),
    row('GENERIC:RBF TAP TAP TAP', 'fast_g4_gelu', '3x3', 17, 2, 32, 2, G=2),
    # GENERIC:RELU
    row('GENERIC:RELU DW DW DW', 'relu_g3k2', '3x3', 17, 2, 2, 2, G=2, scale=3.0),
    row('GENERIC:RELU TAP TAP TAP', 'relu_g3k2', '3x3', 17, 6, 2, 5, G=2),
    row('GENERIC:RELU TAP TAP TAP-PM', 'relu_g3k2', '3x3', 17, 2, 32, 3, G=2, scale=3.0),
    row('GENERIC:RELU TAP TAP-PM TAP', 'relu_g3k2', '1x1p2', 17, 2, 32, 2, G=2, affine=True),
    row('GENERIC:RELU TAP TAP-PM TAP-PM', 'relu_g3k2', '1x1p1', 17, 2, 32, 2, G=2, scale=3.0),
    row('GENERIC:RELU TAP-PM TAP TAP-PM', 'relu_g3k2', 's2', 17, 2, 32, 3, G=2),
    row('GENERIC:RELU TAP-PM TAP-PM TAP-PM', 'relu_g3k2', '3x3', 17, 2, 32, 2, G=2, scale=3.0, affine=True),
    # depthwise weight gradients over several slabs (dw_weight_chunks > 1: B * Ho * Wo > 256)
    row('FAST_BSPLINE_GELU DW DW DW', 'kan_gelu', '3x3', 17, 2, 2, 8, G=2, scale=3.0),
    row('FAST_BSPLINE_SILU DW DW DW', 'kan_silu', '3x3', 17, 2, 4, 8, G=2, affine=True),
    row('FAST_CHEBY4 DW DW DW', 'cheby_d3', '3x3', 17, 2, 2, 8, G=2),
    row('FAST_CHEBY5 DW DW DW', 'cheby_d4', '3x3', 17, 2, 4, 8, G=2, affine=True),
    row('FAST_GRAM4 DW DW DW', 'gram_d3', '3x3', 17, 2, 2, 8, G=2),
    row('FAST_POLY1 DW DW DW', 'taylor_d1', '3x3', 17, 2, 4, 8, G=2, affine=True),
    row('FAST_POLY3 DW DW DW', 'fibonacci_d2', '3x3', 17, 2, 2, 8, G=2),
    row('FAST_POLY4 DW DW DW', 'bessel_d3', '3x3', 17, 2, 4, 8, G=2, affine=True),
    row('FAST_RBF5 DW DW DW', 'fast_g5', '3x3', 17, 2, 2, 8, G=2, scale=3.0),
    row('FAST_RBF8 DW DW DW', 'fast_g8', '3x3', 17, 2, 4, 8, G=2, affine=True),
    row('FAST_RELU8 DW DW DW', 'relu_g5k3', '3x3', 17, 2, 2, 8, G=2, scale=3.0),
    row('GENERIC:BSPLINE DW DW DW', 'kan_g8o1', '3x3', 17, 2, 4, 8, G=2, affine=True),
    row('GENERIC:CHEBY DW DW DW', 'cheby_d6', '3x3', 17, 2, 2, 8, G=2),
    row('GENERIC:FOURIER DW DW DW', 'fourier_g3', '3x3', 17, 2, 4, 8, G=2, affine=True),
    row('GENERIC:GRAM DW DW DW', 'gram_d5', '3x3', 17, 2, 2, 8, G=2),
    row('GENERIC:POLY DW DW DW', 'laguerre_d5', '3x3', 17, 2, 4, 8, G=2, affine=True),
    row('GENERIC:RBF DW DW DW', 'fast_g4_gelu', '3x3', 17, 2, 2, 8, G=2, scale=3.0),
    row('GENERIC:RELU DW DW DW', 'relu_g3k2', '3x3', 17, 2, 4, 8, G=2, affine=True),
    # LegendreKAN: second input tensor; the plan sets position-major targets (and the shape would take halo / band kernels), the launch stays image-major
    row('FAST_POLY4 TAP TAP TAP', 'legendre_d3', '3x3', 17, 3, 40, 2, affine=True),
    row('FAST_POLY4 TAP TAP TAP', 'legendre_d3', '3x3', 2, 2, 128, 8, G=2),
    row('FAST_POLY3 TAP TAP TAP', 'legendre_d2', '3x3', 17, 3, 40, 2),
]


def case_ids(cases):
    """Readable, unique test ids: spec-fwd-bd-bw, with a suffix for the extra rows of a cell."""
    seen, out = {}, []
    for c in cases:
        i = key_id(c["key"])
        n = seen[i] = seen.get(i, 0) + 1
        out.append(i if n == 1 else f"{i}-{n}")
    return out
