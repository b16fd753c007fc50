"""Edge-input cells of the basis expansions: every way the kernels turn an input value into its planes (value) and into the derivatives
of those planes (input gradient), fed inputs that sit ON the special points of each basis instead of `randn * scale`.

The arithmetic exists in five separately written forms:

  1  stage_unit<KIND, FAST != 0>        csrc/kan_common.h   compile-time specs, hardware exp2 / rcp, kan_tanh_fast
  2  stage_unit<KIND, 0>                csrc/kan_common.h   -> bspline_uniform<false> / kan_planes_each<KIND, false> (csrc/kan_device.h)
  3  stage_unit_grad<KIND, FAST>        csrc/kan_common.h   k_conv_bwd_data, compile-time specs
  4  kan_planes_each<KIND, true>        csrc/kan_device.h   k_conv_bwd_data, generic specs
  5  kan_planes<KIND, DERIV>            csrc/kan_device.h   the depthwise k_dw_* kernels (array form), all three stages

A cell is (spec class of route_cells.spec_class, MFMA | DW).  Which form each stage (forward / input gradient / weight gradient) of a
cell runs, read from the launchers (csrc/kanconv.hip: dispatch_fast<ON_*> takes a compile-time spec only onto the kernel families of its
fast_spec row, csrc/kan_internal.h; kan_conv_bwd_data falls back to the generic epilogue when the tensors do not fit the spec):

  spec class                              MFMA fwd / bwd-data / bwd-weight      DW (all stages)
  FAST_BSPLINE_SILU, FAST_BSPLINE_GELU    1 / 3 / 1                             5
  FAST_RBF8, FAST_RBF5                    1 / 3 / 1   (whole layer, see below)  5   (whole layer)
  FAST_CHEBY5, FAST_CHEBY4                1 / 3 / 1                             5
  FAST_POLY4, FAST_POLY3, FAST_POLY1      1 / 3 / 1                             5
  FAST_RELU8, FAST_GRAM4                  1 / 4 / 1   (halo forward and halo    5
                                          weight gradient: the only kernels
                                          of these specs; bwd-data has none)
  GENERIC:BSPLINE (g8o1, g3o2, g5o1,      2 / 4 / 2                             5
                   g7o1, g5o0)
  GENERIC:RBF                             2 / 4 / 2   (whole layer)             5   (whole layer)
  GENERIC:CHEBY, GENERIC:FOURIER,         2 / 4 / 2                             5
  GENERIC:RELU, GENERIC:GRAM
  GENERIC:POLY  gegen_d5 (on tanh x)      2 / 4 / 2                             5
                legendre_d4 (on x_n, the  2 / 4 / 2                             5
                layer's second input)

FastKAN evaluates its RBFs on a second, instance-normalised tensor that the layer computes itself, and the oracle has no pre-norm output
for it (the layer HAS no norm after the conv stage): its cells run the whole layer through helpers.check_vs_oracle(fallback=False).  Every
other cell is compared at the conv stage (hip_stage / oracle_stage below), before the norm.

Inputs (edge_values): every element of x is an edge value of the layer's own basis parameters -- the `grid` set (knots / centres / phases /
multiples of pi/2 with their fp32 neighbours, span ends, zeros, denormals, +-1, +-0.5) or the `tail` set (+-6 .. +-104: saturated tanh, the
Chebyshev clamp, exp over- and underflow in SiLU / GELU / the RBFs) -- tiled through the tensor by a seeded permutation per channel
(edge_input).  Non-finite inputs (nonfinite_cell, nonfinite_input): randn with one NaN, one +inf and one -inf, each in its own image of four.

Backward rows dropped from the non-finite tests (fp32 and fp64 oracle disagree on the mask of dx): NO_BACKWARD, empty.  Forward rows whose
layer is swapped for its SiLU twin (fp32 and fp64 torch disagree on GELU(+inf)): SILU_TWINS."""
import copy

import numpy as np
import torch
import torch.nn as nn

import route_cells as R
from helpers import oracle_forward

# B-spline layers at the orders whose derivative is discontinuous at the knots (order 1: slope +-1/h per cell) or whose value is (order 0),
# and a recurrence family of the generic spec that runs on plain x (LegendreKAN: x_n, the layer's second input).
EXTRA_LAYERS = {
    "kan_g5o1": ("KANConv2DLayer", dict(grid_size=5, spline_order=1)),
    "kan_g7o1": ("KANConv2DLayer", dict(grid_size=7, spline_order=1)),
    "kan_g5o0": ("KANConv2DLayer", dict(grid_size=5, spline_order=0)),
    "legendre_d4": ("LegendreKANConv2DLayer", dict(degree=4)),
}
# Non-finite tests: torch's fp32 GELU(+inf) is NaN on the CPU (vectorised erf) and its fp64 GELU(+inf) is +inf, so where the base branch
# alone decides what +inf becomes (bounded bases on tanh x; the order-0 B-spline, whose planes are plain indicators) the two oracles disagree
# on the forward mask.  Those layers run the non-finite tests with a SiLU base branch, which leaves their spec class as it is; GELU meets
# +inf in the FAST_BSPLINE_GELU and GENERIC:BSPLINE g8o1 cells (NaN in both oracles: the Cox-de Boor recursion multiplies inf by 0).
SILU_TWINS = ("lucas_d3", "hermite_d2", "taylor_d1", "gegen_d5", "kan_g5o0")
for _name in SILU_TWINS:
    _cls, _kw = R.LAYERS.get(_name) or EXTRA_LAYERS[_name]
    EXTRA_LAYERS[_name + "_silu"] = (_cls, dict(_kw, base_activation=nn.SiLU))
for _name, _spec in EXTRA_LAYERS.items():          # case_layer / case_cfg look layers up in route_cells.LAYERS; no ROUTE_CASES row names these
    R.LAYERS.setdefault(_name, _spec)

# (spec class, layer, forms "fwd/bwd-data/bwd-weight" of the MFMA cell, whole layer)
SPECS = [
    ("FAST_BSPLINE_SILU", "kan_silu", "1/3/1", False), ("FAST_BSPLINE_GELU", "kan_gelu", "1/3/1", False),
    ("FAST_RBF8", "fast_g8", "1/3/1", True), ("FAST_RBF5", "fast_g5", "1/3/1", True),
    ("FAST_CHEBY5", "cheby_d4", "1/3/1", False), ("FAST_CHEBY4", "cheby_d3", "1/3/1", False),
    ("FAST_POLY4", "lucas_d3", "1/3/1", False), ("FAST_POLY3", "hermite_d2", "1/3/1", False), ("FAST_POLY1", "taylor_d1", "1/3/1", False),
    ("FAST_RELU8", "relu_g5k3", "1/4/1", False), ("FAST_GRAM4", "gram_d3", "1/4/1", False),
    ("GENERIC:BSPLINE", "kan_g8o1", "2/4/2", False), ("GENERIC:BSPLINE", "kan_g3o2", "2/4/2", False), ("GENERIC:BSPLINE", "kan_g5o1", "2/4/2", False),
    ("GENERIC:BSPLINE", "kan_g7o1", "2/4/2", False), ("GENERIC:BSPLINE", "kan_g5o0", "2/4/2", False),
    ("GENERIC:RBF", "fast_g4_gelu", "2/4/2", True), ("GENERIC:CHEBY", "cheby_d6", "2/4/2", False),
    ("GENERIC:POLY", "gegen_d5", "2/4/2", False), ("GENERIC:POLY", "legendre_d4", "2/4/2", False),
    ("GENERIC:FOURIER", "fourier_g3", "2/4/2", False), ("GENERIC:RELU", "relu_g3k2", "2/4/2", False), ("GENERIC:GRAM", "gram_d5", "2/4/2", False),
]
SPEC_CLASSES = ["FAST_" + n for n in R.FAST_NAMES.values()] + ["GENERIC:" + n for n in R.KIND_NAMES.values()]
HALO_ONLY = ("FAST_RELU8", "FAST_GRAM4")           # compile-time staging in the halo and expanded kernels alone (kan_internal.h: fast_spec)
NO_BACKWARD = set()                                # layers whose non-finite backward row is dropped (test_edge_matrix.py keeps this honest)


def _cells():
    """Two inputs per image plane of 8x8 (128 values per channel: room for the largest grid set), 3x3 kernels.  MFMA: two input channels in
    one group, so dw_direct fails; 128 outputs put the 3x3 layer on the halo forward (the cheapest HALO rows of ROUTE_CASES are (B=2, C=2,
    O=128, H=4)), which FAST_RELU8 / FAST_GRAM4 need to reach form 1 and which costs the others nothing.  DW: one input channel and one
    output per group."""
    out = []
    for spec, layer, forms, whole in SPECS:
        out.append(dict(R.row(spec, layer, "3x3", 2, 2, 128, 8), spec=spec, kind="MFMA", forms=forms, whole=whole))
        out.append(dict(R.row(spec, layer, "3x3", 2, 2, 2, 8, G=2), spec=spec, kind="DW", forms="5/5/5", whole=whole))
    return out


CELLS = _cells()


def cell_id(cell):
    return f"{cell['spec'].replace(':', '_')}-{cell['layer']}-{cell['kind']}"


def nonfinite_cell(cell):
    """The cell for the non-finite tests: four images (one per non-finite value and a clean one: FastKAN's instance norm spreads a non-finite
    value over its whole plane), and a 1x1 kernel where the cell's forms do not hang on the halo kernels (3x3 only); the SiLU twin of a layer
    whose GELU base branch the two oracles disagree on (SILU_TWINS)."""
    return dict(cell, B=4, shape="3x3" if cell["kind"] == "MFMA" and cell["spec"] in HALO_ONLY else "1x1",
                layer=cell["layer"] + "_silu" if cell["layer"] in SILU_TWINS else cell["layer"])


def family(cell, layer=None):
    """(spec class, "DW" | "MFMA", forward route, bwd-data route) the planner gives the cell's layer on its input."""
    g, b, p = R.case_structs(cell, layer)
    key = R.route_key(g, b, p)
    return key[0], "DW" if key[1] == "DW" else "MFMA", key[1], key[2]


def forms_of(cell, layer=None):
    """"fwd/bwd-data/bwd-weight" forms of the cell's launches, restated from the launchers: DW runs kan_planes throughout; a generic spec
    runs stage_unit<KIND, 0> and kan_planes_each<KIND, true>; a compile-time spec runs stage_unit<KIND, FAST> on the routes the planner picks
    for it (it offers a spec only its own kernels, fast_spec().routes) and stage_unit_grad where it has tap-major kernels and the tensors fit
    (kan_conv_bwd_data: one input tensor); the halo-only specs stage generically on every other route."""
    g, b, p = R.case_structs(cell, layer)
    key = R.route_key(g, b, p)
    if key[1] == "DW":
        return "5/5/5"
    if key[0].startswith("GENERIC"):
        return "2/4/2"
    if key[0] in HALO_ONLY:
        return f"{1 if key[1].startswith(('HALO', 'EXPANDED')) else 2}/4/{1 if key[3] in ('HALO', 'EXPANDED') else 2}"
    return f"1/{4 if R.second_input(b) else 3}/1"


def make_layer(cell, seed=0):
    """The cell's layer, seeded, with its trainable basis parameters away from their init (test_gpu_route_matrix._perturb)."""
    torch.manual_seed(seed)
    layer = R.case_layer(cell)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        if hasattr(layer, "phase_low"):
            layer.phase_low.add_(0.06 * torch.randn(layer.phase_low.shape, generator=gen))
            layer.phase_high.add_(0.06 * torch.randn(layer.phase_high.shape, generator=gen))
        if hasattr(layer, "beta_weights"):
            layer.beta_weights.copy_(0.2 * torch.randn(layer.beta_weights.shape, generator=gen))
    return layer


# --------------------------------------------------------------------------------------------------------------- edge values
TAIL = [6.0, 8.0, 9.0, 9.02, 10.0, 20.0, 44.0, 88.0, 89.0, 104.0]
TAIL_KEPT = [6.0, 8.0, 9.0, 9.02, 10.0, 20.0]      # what every family must keep
f32 = np.float32
_INF = f32(np.inf)


def _ulp(v):
    v = f32(v)
    return [np.nextafter(v, -_INF), np.nextafter(v, _INF)]


def special_points(layer):
    """{class: fp32 array} of the points the layer's own basis parameters define."""
    from convkan_amd import _lib as L
    kw = layer._basis_kw()
    if kw["kind"] == L.BASIS_BSPLINE:
        return {"on a knot": layer.grid.numpy().astype(f32)}
    if kw["kind"] == L.BASIS_RBF:
        return {"on a centre": layer.rbf.grid.detach().numpy().astype(f32)}
    if kw["kind"] == L.BASIS_RELU:
        return {"on a phase": torch.cat([layer.phase_low.detach().reshape(-1), layer.phase_high.detach().reshape(-1)]).numpy().astype(f32)}
    if kw["kind"] == L.BASIS_FOURIER:
        return {"multiple of pi/2": np.array([f32(k * np.pi / 2) for k in range(-8, 9)], dtype=f32)}
    return {}


def edge_values(layer, which):
    """(values, classes): the fp32 edge values of `which` ('grid' | 'tail', before the oracle's finiteness filter) and the class of each.  A value
    that belongs to several classes keeps the first one added."""
    from convkan_amd import _lib as L
    seen = {}

    def add(v, cls):
        seen.setdefault(f32(v).tobytes(), (f32(v), cls))
    if which == "tail":
        for v in TAIL:
            add(v, "tail value"); add(-v, "tail value")
    else:
        pts = special_points(layer)
        for cls, vals in pts.items():
            for v in vals:
                add(v, cls)
        if layer._basis_kw()["kind"] == L.BASIS_BSPLINE:
            kn = pts["on a knot"]
            h = f32(kn[1] - kn[0])
            add(np.nextafter(kn[-1], -_INF), "span end")           # (g0 and gN themselves are knots: first class wins)
            add(f32(kn[0] - h), "outside"); add(f32(kn[-1] + h), "outside")
            for a, b in zip(kn[:-1], kn[1:]):
                add(f32(0.5) * (a + b), "midpoint")
        for vals in pts.values():
            for v in vals:
                for n in _ulp(v):
                    add(n, "one ulp off")
        add(0.0, "zero"); add(-0.0, "zero")
        den = np.nextafter(f32(0), _INF)
        add(den, "denormal"); add(-den, "denormal")
        for v in (1.0, -1.0, 0.5, -0.5):
            add(v, "unit")
    vals = np.array([v for v, _ in seen.values()], dtype=f32)
    return vals, [c for _, c in seen.values()]


def edge_input(values, B, C, H, W, seed):
    """[B, C, H, W] of `values` alone: per channel the set tiled to B*H*W and permuted (seeded), so each value meets each channel."""
    n = B * H * W
    assert 0 < len(values) <= n, f"{len(values)} edge values do not fit {n} positions per channel"
    rng = np.random.default_rng(seed)
    x = np.empty((B, C, H, W), dtype=f32)
    for c in range(C):
        x[:, c] = np.resize(values, n)[rng.permutation(n)].reshape(B, H, W)
    return torch.from_numpy(x)


def class_of(values, classes):
    """{bit pattern: class}: names the edge class of an element of x."""
    return {f32(v).tobytes(): c for v, c in zip(values, classes)}


def nonfinite_input(cell, seed, only_nan=False):
    """randn with one NaN, one +inf and one -inf (`only_nan`: the NaN alone), each in its own image and -- where the layer has two channels -- not all
    in the same one; at its pixel every other channel is an ordinary value."""
    x = torch.randn(cell["B"], cell["C"], cell["H"], cell["W"], generator=torch.Generator().manual_seed(seed))
    C, H, W = cell["C"], cell["H"], cell["W"]
    x[0, 0, H // 2, W // 2] = float("nan")
    if not only_nan:
        x[1, C - 1, 0, W - 1] = float("inf")
        x[2, 0, H - 1, 1] = float("-inf")
    return x


# --------------------------------------------------------------------------------------------------------------- the two conv stages
def oracle_stage(cfg, layer, x, dz, dtype):
    """The CPU oracle's pre-norm tensor z (helpers.oracle_forward's pre_norm_out, groups concatenated) with `layer`'s parameters in `dtype`,
    and -- with an upstream gradient dz -- torch.autograd.grad of <z, dz>: (z, dx, {parameter gradients})."""
    l2 = copy.deepcopy(layer).cpu().to(dtype)
    if isinstance(getattr(l2, "grid", None), torch.Tensor):
        l2.grid = l2.grid.to(dtype)
    xo = x.to(dtype).clone().requires_grad_(True)
    pre = []
    y = oracle_forward(cfg, l2, xo, pre)
    z = torch.cat(pre, dim=1) if pre else y        # FastKAN: no norm after the conv stage, the layer's output is z
    if dz is None:
        return z.detach(), None, {}
    named = [(n, p) for n, p in l2.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad((z * dz.to(dtype)).sum(), [xo] + [p for _, p in named], allow_unused=True)
    return z.detach(), grads[0], {n: g for (n, _), g in zip(named, grads[1:]) if g is not None}


def hip_stage(layer, x):
    """The pre-norm tensor of the HIP layer, through the layer's own conv-stage call: _conv_stage (ops.kan_conv) as forward() makes it for the
    'norm, PReLU' layers; forward() itself with the norm-and-activation tail taken off for the 'norm, then activation' layers (ReLU-KAN:
    kan_conv_phased on its stacked phases; GRAM: on its coefficients; Legendre: on x_n)."""
    from convkan_amd.layers.conv_layers import FastKANConvNDLayer, _FusedTailLayer
    if isinstance(layer, FastKANConvNDLayer):       # the whole layer: its output is the conv stage of (x, instance-normalised x)
        return layer(x)
    if isinstance(layer, _FusedTailLayer):
        xa, xb = layer._base_input(x) if layer._has_base else (x, None)
        wb = [m.weight for m in layer.base_conv] if layer._has_base else []
        return layer._conv_stage(layer.conv_spec(), xa, xb, wb, [m.weight for m in getattr(layer, layer._basis)])
    layer._norm_act = lambda z: z
    try:
        return layer(x)
    finally:
        del layer._norm_act


def tail_values(cell, layer, cfg):
    """The cell's tail set: TAIL's values at which the fp32 CPU oracle of the family (z, dx and the parameter gradients of a plane filled with the
    value, with one zero per channel so that LegendreKAN's min-max normalisation has a range) is finite."""
    vals, classes = edge_values(layer, "tail")
    keep = []
    for v in vals:
        x = torch.full((1, cell["C"], 3, 3), float(v))
        x[:, :, 0, 0] = 0.0
        z = oracle_stage(cfg, layer, x, None, torch.float32)[0]
        z, dx, dw = oracle_stage(cfg, layer, x, torch.ones_like(z), torch.float32)
        keep.append(bool(torch.isfinite(z).all() and torch.isfinite(dx).all() and all(torch.isfinite(g).all() for g in dw.values())))
    keep = np.array(keep)
    return vals[keep], [c for c, k in zip(classes, keep) if k]
