"""CPU: the edge-input matrix (tests/edge_cells.py) is what it says it is.

(a) every cell -- and its four-image variant of the non-finite tests -- plans to the route family it declares (DW, or an MFMA forward with
    k_conv_bwd_data) and to the forms its table row names; every spec class has both kinds of cell;
(b) the grid sets hold every knot / centre / phase of the layer bit for bit, with both fp32 neighbours, and fit the tensor; each order-1
    B-spline set holds a value at which floor((x - g0) * inv_h) in fp32 is NOT the half-open cell of the fp32 knots (the inputs on which a
    kernel that trusts that index differentiates the wrong piece);
(c) the tail sets are finite in the fp32 and the fp64 oracle and keep at least +-6 .. +-20;
(d) the fp32 and fp64 oracle agree on every non-finite mask the GPU tests compare against."""
import functools

import numpy as np
import pytest
import torch

import edge_cells as E
import route_cells as R
from oracle import kan_oracle as O

IDS = [E.cell_id(c) for c in E.CELLS]
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _layer(name):
    cell = next(c for c in E.CELLS if c["layer"] == name and c["kind"] == "MFMA")
    return cell, E.make_layer(cell)


LAYER_NAMES = sorted({c["layer"] for c in E.CELLS})


@pytest.mark.parametrize("cell", E.CELLS, ids=IDS)
def test_cell_plans_to_its_family_and_forms(cell):
    for c in (cell, E.nonfinite_cell(cell)):
        spec, kind, fwd, bd = E.family(c)
        assert (spec, kind) == (c["spec"], c["kind"]), f"{c}: plans to {(spec, kind, fwd, bd)}"
        assert bd in (("DW",) if kind == "DW" else ("TAP", "TAP-PM", "TAP-RB")), f"{c}: bwd-data route {bd} is not k_conv_bwd_data"
        assert E.forms_of(c) == c["forms"], f"{c}: runs forms {E.forms_of(c)}"
        assert c["B"] <= 4 and c["H"] == c["W"] <= 8


def test_every_spec_class_has_both_kinds_of_cell():
    have = {}
    for c in E.CELLS:
        have.setdefault(c["spec"], set()).add(c["kind"])
    assert set(have) == set(E.SPEC_CLASSES), set(E.SPEC_CLASSES) ^ set(have)
    assert all(k == {"MFMA", "DW"} for k in have.values()), have
    orders = {R.LAYERS[c["layer"]][1].get("spline_order") for c in E.CELLS if c["spec"] == "GENERIC:BSPLINE"}
    assert {0, 1, 2} <= orders
    assert {R.case_structs(c)[1].order & 1 for c in E.CELLS if c["spec"] == "GENERIC:POLY"} == {0, 1}, "one family on tanh x, one on x"


@pytest.mark.parametrize("name", LAYER_NAMES)
def test_grid_set_holds_every_special_point(name):
    cell, layer = _layer(name)
    vals, classes = E.edge_values(layer, "grid")
    bits = {v.tobytes() for v in vals}
    assert len(bits) == len(vals) == len(classes) <= cell["B"] * cell["H"] * cell["W"]
    kind = R.KINDS[R.LAYERS[name][0]]
    if kind == "bspline":                          # the oracle's own knots / centres, not the layer's copy
        points = O.bspline_knots(layer.grid_size, layer.spline_order, layer.grid_range).numpy()
        assert {f32(points[-1]).tobytes(), np.nextafter(f32(points[-1]), f32(-np.inf)).tobytes()} <= bits
        h = f32(points[1] - points[0])
        assert {f32(points[0] - h).tobytes(), f32(points[-1] + h).tobytes()} <= bits
    elif kind == "rbf":
        points = O.rbf_grid(layer.grid_size, layer.grid_range)[0].numpy()
    elif kind == "relu":
        points = torch.cat([layer.phase_low.detach().reshape(-1), layer.phase_high.detach().reshape(-1)]).numpy()
        assert len({p.tobytes() for p in points}) == len(points), "perturbed phases are all distinct"
    elif kind == "fourier":
        points = np.array([k * np.pi / 2 for k in range(-8, 9)]).astype(f32)
    else:
        points = np.array([], dtype=f32)
    for p in points.astype(f32):
        for v in (p, np.nextafter(p, f32(-np.inf)), np.nextafter(p, f32(np.inf))):
            assert v.tobytes() in bits, f"{name}: {v!r} (point {p!r}) is missing"
    for v in (0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 0.5, -0.5):
        assert f32(v).tobytes() in bits
    x = E.edge_input(vals, cell["B"], cell["C"], cell["H"], cell["W"], seed=3)
    for c in range(cell["C"]):                     # each value meets each channel
        assert {v.tobytes() for v in x[:, c].numpy().reshape(-1)} == bits


@pytest.mark.parametrize("name", [n for n in LAYER_NAMES if R.LAYERS[n][1].get("spline_order") == 1])
def test_order1_grid_set_holds_a_value_whose_fp32_cell_index_is_off(name):
    _, layer = _layer(name)
    kn = O.bspline_knots(layer.grid_size, layer.spline_order, layer.grid_range).numpy()
    ni = len(kn) - 1
    inv_h = f32(f32(ni) / f32(kn[-1] - kn[0]))                  # dev_basis (csrc/kan_common.h)
    off = []
    for v in E.edge_values(layer, "grid")[0]:
        ref = [i for i in range(ni) if v >= kn[i] and v < kn[i + 1]]
        if ref:
            i = min(max(int(np.floor(f32(f32(v - kn[0]) * inv_h))), 0), ni - 1)
            if i != ref[0]:
                off.append((float(v), ref[0], i))
    print(f"{name}: {len(off)} values with a misplaced fp32 cell index (value, half-open cell, floor index): {off[:6]}")
    assert off, f"{name}: no value of the grid set distinguishes the fp32 floor index from the half-open cell"


@pytest.mark.parametrize("cell", [c for c in E.CELLS if c["kind"] == "MFMA"], ids=[i for i, c in zip(IDS, E.CELLS) if c["kind"] == "MFMA"])
def test_tail_set_is_finite_in_both_oracles(cell):
    layer = E.make_layer(cell)
    cfg = R.case_cfg(cell, layer)
    vals, _ = E.tail_values(cell, layer, cfg)
    assert {f32(s * v).tobytes() for v in E.TAIL_KEPT for s in (1, -1)} <= {v.tobytes() for v in vals}, f"{cell}: tail set {vals}"
    x = E.edge_input(vals, cell["B"], cell["C"], cell["H"], cell["W"], seed=5)
    for dtype in (torch.float32, torch.float64):
        z = E.oracle_stage(cfg, layer, x, None, dtype)[0]
        z, dx, dw = E.oracle_stage(cfg, layer, x, torch.ones_like(z), dtype)
        assert torch.isfinite(z).all() and torch.isfinite(dx).all() and all(torch.isfinite(g).all() for g in dw.values()), (cell, dtype)


def _masks(t):
    return torch.isnan(t), t == float("inf"), t == float("-inf")


@pytest.mark.parametrize("cell", E.CELLS, ids=IDS)
def test_oracles_agree_on_the_nonfinite_masks(cell):
    c = E.nonfinite_cell(cell)
    layer = E.make_layer(c)
    cfg = R.case_cfg(c, layer)
    x = E.nonfinite_input(c, seed=7)
    assert int((~torch.isfinite(x)).sum()) == 3 and all(int((~torch.isfinite(x[b])).sum()) == 1 for b in range(3))
    assert int((~torch.isfinite(x)).any(dim=1).sum()) == 3, "one special channel per special pixel"
    z32, z64 = (E.oracle_stage(cfg, layer, x, None, d)[0] for d in (torch.float32, torch.float64))
    for a, b in zip(_masks(z32), _masks(z64)):
        assert torch.equal(a, b), f"{c}: fp32 and fp64 oracle disagree on a forward mask"
    assert not torch.isfinite(z32).all(), "the non-finite inputs reach z"
    xn = E.nonfinite_input(c, seed=7, only_nan=True)
    dz = torch.randn(z32.shape, generator=torch.Generator().manual_seed(8))
    dx32, dx64 = (E.oracle_stage(cfg, layer, xn, dz, d)[1] for d in (torch.float32, torch.float64))
    agree = torch.equal(torch.isfinite(dx32), torch.isfinite(dx64))
    assert agree == (c["layer"] not in E.NO_BACKWARD), f"{c}: backward masks agree: {agree}; NO_BACKWARD says otherwise"
