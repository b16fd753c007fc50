"""Every edge cell (tests/edge_cells.py: spec class x MFMA | DW, i.e. every written form of the basis arithmetic, value and derivative)
against the fp64 oracle on inputs made of edge values alone -- knots, centres, phases and their fp32 neighbours, span ends, zeros,
denormals (the `grid` set) and saturating magnitudes (the `tail` set), judged separately -- and on inputs holding a NaN, a +inf and a -inf.

Compared at the conv stage, before the norm: z, and for an upstream gradient dz ~ N(0, 1) the input gradient and every parameter gradient
(FastKAN: the whole layer, whose output is its conv stage, through helpers.check_vs_oracle).  Tolerance: the project's one rule, per tensor,
max-normalised: error <= max(stated, 4 x the fp32 oracle's own error against fp64 on that tensor, measured live), oneDNN execution only.
Each case prints (error, tolerance, oracle's own error) per tensor and the edge class of the input under the worst element of dx.

Non-finite inputs: the NaN / +inf / -inf masks of z must equal the fp32 oracle's (tests/test_edge_matrix.py: the fp64 oracle has the same
masks), every other element meets the tolerance; for an input with the NaN alone, the non-finite mask of dx must equal the oracle's."""
import copy

import pytest
import torch

import edge_cells as E
import route_cells as R
from helpers import TOL_DW, TOL_DX, TOL_Y, check_vs_oracle, relerr

pytestmark = pytest.mark.gpu
IDS = [E.cell_id(c) for c in E.CELLS]


def _check_plan(cell, layer):
    spec, kind, _, _ = E.family(cell, layer)
    assert (spec, kind) == (cell["spec"], cell["kind"]) and E.forms_of(cell, layer) == cell["forms"], f"{cell}: plans to {E.family(cell, layer)}"


def _judge(errs, name, hip, o32, o64, stated):
    own = relerr(o32, o64)
    errs[name] = (relerr(hip, o64), max(stated, 4.0 * own), own)


def _hip(layer, x, dz):
    dev = copy.deepcopy(layer).cuda()
    xg = x.cuda().requires_grad_(True)
    z = E.hip_stage(dev, xg)
    z.backward(dz.cuda())
    torch.cuda.synchronize()
    return z.detach().cpu(), xg.grad.cpu(), {n: p.grad.cpu() for n, p in dev.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("which", ["grid", "tail"])
@pytest.mark.parametrize("cell", E.CELLS, ids=IDS)
def test_edge_cell_vs_oracle(cell, which, gpu_lib):
    layer = E.make_layer(cell)
    _check_plan(cell, layer)
    cfg = R.case_cfg(cell, layer)
    vals, classes = E.edge_values(layer, "grid") if which == "grid" else E.tail_values(cell, layer, cfg)
    x = E.edge_input(vals, cell["B"], cell["C"], cell["H"], cell["W"], seed=11)
    tag = f"{E.cell_id(cell)}-{which}"
    if cell["whole"]:
        errs = check_vs_oracle(layer, cfg, x, groups=cell["G"], tag=tag, assert_ok=False, fallback=False)
        worst = "(whole layer)"
    else:
        z64 = E.oracle_stage(cfg, layer, x, None, torch.float64)[0]
        dz = torch.randn(z64.shape, generator=torch.Generator().manual_seed(12))
        z32, dx32, dw32 = E.oracle_stage(cfg, layer, x, dz, torch.float32)
        z64, dx64, dw64 = E.oracle_stage(cfg, layer, x, dz, torch.float64)
        z, dx, dw = _hip(layer, x, dz)
        errs = {}
        _judge(errs, "z", z, z32, z64, TOL_Y)
        _judge(errs, "dx", dx, dx32, dx64, TOL_DX)
        assert dw64 and set(dw64) <= set(dw), f"{tag}: parameter gradients the oracle has and the HIP stage lacks: {set(dw64) - set(dw)}"
        for n in dw64:
            _judge(errs, n, dw[n], dw32[n], dw64[n], TOL_DW if dw64[n].dim() >= 3 else 2e-5)
        i = int((dx.double() - dx64).abs().argmax())
        v = x.reshape(-1)[i].numpy()
        worst = f"{E.class_of(vals, classes)[v.tobytes()]} (x = {float(v)!r})"
    print(f"[edge] {tag}: worst dx element under: {worst}")
    for n, (e, t, o) in errs.items():
        print(f"[edge] {tag}: {n}: error {e:.3e} tolerance {t:.3e} oracle's own {o:.3e}")
    bad = {n: v for n, v in errs.items() if not v[0] <= v[1]}
    assert not bad, f"{tag}: (error, tolerance, fp32 oracle's own error) {bad}; worst dx element under: {worst}"


def _masks(t):
    return {"NaN": torch.isnan(t), "+inf": t == float("inf"), "-inf": t == float("-inf")}


@pytest.mark.parametrize("cell", E.CELLS, ids=IDS)
def test_nonfinite_inputs_vs_oracle(cell, gpu_lib):
    c = E.nonfinite_cell(cell)
    layer = E.make_layer(c)
    _check_plan(c, layer)
    cfg = R.case_cfg(c, layer)
    tag = E.cell_id(c)
    x = E.nonfinite_input(c, seed=7)
    z32, z64 = (E.oracle_stage(cfg, layer, x, None, d)[0] for d in (torch.float32, torch.float64))
    dev = copy.deepcopy(layer).cuda()
    with torch.no_grad():
        z = E.hip_stage(dev, x.cuda()).cpu()
    for name, m in _masks(z32).items():
        got = _masks(z)[name]
        print(f"[edge] {tag}: {name}: oracle {int(m.sum())} elements, HIP {int(got.sum())}")
        assert torch.equal(got, m), f"{tag}: {name} mask of z differs from the fp32 oracle's at {(got != m).nonzero()[:8].tolist()} ({int((got != m).sum())} elements)"
    fin = torch.isfinite(z32)                       # the three masks are equal, so these are the finite elements of all three tensors
    assert not fin.all()
    if fin.any():                                   # (LegendreKAN normalises by the batch's min and max: one non-finite input, and no element is finite)
        scale = float(z64[fin].abs().max())
        err, own = (float((t[fin].double() - z64[fin]).abs().max()) / scale for t in (z, z32))
        print(f"[edge] {tag}: finite z: error {err:.3e} tolerance {max(TOL_Y, 4 * own):.3e} oracle's own {own:.3e}")
        assert err <= max(TOL_Y, 4.0 * own), f"{tag}: finite elements of z: error {err:.3e}, oracle's own {own:.3e}"
    if c["layer"] in E.NO_BACKWARD:
        return
    xn = E.nonfinite_input(c, seed=7, only_nan=True)
    dz = torch.randn(z32.shape, generator=torch.Generator().manual_seed(8))
    dx32 = E.oracle_stage(cfg, layer, xn, dz, torch.float32)[1]
    dx = _hip(layer, xn, dz)[1]
    got, want = ~torch.isfinite(dx), ~torch.isfinite(dx32)
    print(f"[edge] {tag}: non-finite dx: oracle {int(want.sum())} elements, HIP {int(got.sum())}")
    assert torch.equal(got, want), f"{tag}: non-finite mask of dx differs from the oracle's at {(got != want).nonzero()[:8].tolist()}"
