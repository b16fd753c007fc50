"""CPU: the band cell matrix (tests/band_cells.py) stays in step with `kan_band_route`, the export of the configuration the band launchers
(csrc/kan_direct.hip) read -- the five properties of tests/test_route_matrix.py / test_order_matrix.py on these keys:

(a) every BAND_CASES row plans to the instantiations it declares, forward and weight gradient (so a constant in place of the route's MO, WP, bw_WR
    or bw_slots, or a planner change that moves a row to another template body, fails here);
(b) every cell reached on band_cells.grid() x the six spec classes has a row;
(c) every cell a row lands in is reached, and every row is the smallest of some cell, so that the table without any one row lacks something;
(d) the smallest row of every cell is the grid's smallest geometry of that cell under band_cells.order();
(e) exemptions (none) are live.
And: the compiled instantiations the grid never reaches are exactly band_cells.UNREACHED, each with a figure that is recomputed here; the export
agrees with the public KanPlan wherever the two overlap; LegendreKAN never takes the band route and FastKAN keeps the band weight gradient where
the single-tensor specs leave it; every single-row deletion breaks (b) or (d); and from the fp64 oracle, at most 1 % of a row's
outputs lie within 1e-4 of the PReLU kink (the ones helpers.check_vs_oracle gives no upstream gradient; 1 % is the norm matrix's cap)."""
import ctypes
import functools
import random

import pytest
import torch

import band_cells as BC
from band_cells import BAND_CASES, EXEMPT, UNREACHED, case_ids
from convkan_amd import _lib as L
from route_cells import plan_of

KINK_CAP = 0.01


@functools.lru_cache(maxsize=1)
def planned():
    """({cell: (order, layer, geometry) of the smallest grid geometry that reaches it}, {(spec, NG, WR, NI): largest NG * bw_cells of a grid launch},
    band launches seen)."""
    reach, units, n = {}, {}, 0
    for c in BC.grid():
        g, o = BC.geom_of(c), BC.order(c)
        for layer in BC.grid_layers(c):
            b = BC.basis_of(layer)
            r = BC.band_route(g, b)
            assert r is not None, f"the planner rejects grid geometry {c} for {layer}"
            if not r.fwd_band:
                assert not r.bw_band
                continue
            n += 1
            for cell in BC.cells_of(g, b, r):
                if cell not in reach or o < reach[cell][0]:
                    reach[cell] = (o, layer, c)
            if r.bw_band:
                k = (BC.SPEC_OF[layer], r.NG, r.bw_WR, r.bw_NI)
                units[k] = max(units.get(k, 0), r.NG * r.bw_cells)
    return reach, units, n


@functools.lru_cache(maxsize=1)
def row_cells():
    """[(order, cells the row lands in)] per BAND_CASES row."""
    out = []
    for case in BAND_CASES:
        g, b, r = BC.case_route(case)
        out.append((BC.order(case), tuple(BC.cells_of(g, b, r)) if r is not None else ()))
    return out


def defects(rows):
    """What a table of (order, cells) rows lacks against the grid: reached cells without a row, and cells whose smallest row is not the grid's."""
    reach = planned()[0]
    least = {}
    for o, cells in rows:
        for cell in cells:
            least[cell] = min(o, least.get(cell, o))
    missing = [cell for cell in reach if cell not in least and cell not in EXEMPT]
    big = [(cell, least[cell], reach[cell]) for cell in least if cell in reach and least[cell] > reach[cell][0]]
    return missing, big


def compiled():
    fwd = {("F", spec, NG, MO, WP) for spec in BC.PLANES_OF for NG in (1, 2, 3) for MO, WP in BC.FWD_TILES}
    bw = {("W", spec, NG, WR, NI, SL) for spec in BC.BW_SPECS for NG in (1, 2, 3) for WR, NI in BC.BW_TILES for SL in BC.BW_SLOTS}
    return fwd | bw


@pytest.mark.parametrize("case", BAND_CASES, ids=case_ids(BAND_CASES))
def test_band_case_plans_to_its_instantiations(case):
    g, b, r = BC.case_route(case)
    assert r is not None and r.fwd_band == 1, f"{case}: the forward does not take the band route"
    inst = [cell for cell in BC.cells_of(g, b, r) if cell[0] in ("F", "W")]
    assert inst == case["cells"], f"row {case} now plans to {inst}"
    Ho, Wo = BC.out_hw(case["shape"], case["H"], case["W"])
    assert Ho * Wo >= BC.MIN_PIXELS and 2.0 * BC.work(case) * r.P < BC.MAX_FLOPS


def test_grid_reaches_the_band_kernels():
    reach, _, n = planned()
    assert n > 200000 and len(reach) > 500, (n, len(reach))


def test_every_reachable_cell_has_a_row():
    missing, _ = defects(row_cells())
    reach = planned()[0]
    assert not missing, f"{len(missing)} reached band cells have no BAND_CASES row:\n" + \
        "\n".join(f"  {BC.cell_id(c)}  (smallest: {reach[c][1]} {reach[c][2]})" for c in sorted(missing, key=str))


def test_every_row_lands_in_reached_cells_and_is_the_smallest_of_one():
    reach = planned()[0]
    stray = sorted({BC.cell_id(cell) for _, cells in row_cells() for cell in cells if cell not in reach})
    assert not stray, f"cells of BAND_CASES rows that no grid geometry reaches: {stray}"
    idle = [BC.case_id(case) for case, (o, cells) in zip(BAND_CASES, row_cells()) if not any(reach[cell][0] == o for cell in cells)]
    assert not idle, f"rows that are the smallest geometry of no cell: {idle}"


def test_smallest_row_of_every_cell_is_its_smallest_geometry():
    _, big = defects(row_cells())
    assert not big, "cells whose smallest row is larger than the smallest grid geometry (cell, row order, (order, layer, geometry)): " + str(big[:10])


def test_exemptions_are_live():
    assert len(EXEMPT) <= 2
    have = {cell for _, cells in row_cells() for cell in cells}
    assert not set(EXEMPT) & have, "an exempted cell also has a row: drop the exemption"
    assert set(EXEMPT) <= set(planned()[0]), "an exempted cell is no longer reached: drop the exemption"


def test_unreached_instantiations_are_listed_with_live_reasons():
    """band_has_kernel's table and the four (WR, NI) pairs give 72 + 96 instantiations; the ones no grid geometry reaches are UNREACHED, by name.
    Each names the most expansion units (NG x halo cells) any grid launch of its (spec, NG, WR, NI) needs: SLOTS = 6 is taken above 3 per thread."""
    reach, units, _ = planned()
    dead = compiled() - set(reach)
    assert dead == set(UNREACHED), f"compiled and unreached but not listed: {sorted(dead - set(UNREACHED), key=str)}; listed but reached or not " \
                                   f"compiled: {sorted(set(UNREACHED) - dead, key=str)}"
    assert not {cell for cell in reach if cell[0] in ("F", "W")} - compiled(), "the route names an instantiation that is not compiled"
    for cell, (most, reason) in UNREACHED.items():
        _, spec, NG, WR, NI, SL = cell
        assert SL == 6 and reason
        got = units.get((spec, NG, WR, NI), 0)
        assert got == most, f"{BC.cell_id(cell)}: the largest grid launch needs {got} units, the reason says {most}"
        assert got <= 3 * WR * 64, f"{BC.cell_id(cell)}: {got} units are more than 3 per thread, yet SLOTS = 6 is not reached"


def _agrees(g, b, r, p, what):
    assert (r.fwd_band, r.bw_band) == (p.fwd_band, p.bwd_weight_band), what
    if r.fwd_band:
        assert (p.KC, p.IPC, p.Kpad, p.fwd_splits) == (r.NPLE, r.NG, r.n_steps * r.NPLE, r.fwd_splits), what
        assert r.TO == 64 * r.MO and r.TP == 64 * r.WP and r.NT == 128 * r.WP and r.NPLE == r.NG * r.P + (r.NG * r.P & 1), what
        assert r.tiles_o * r.TO == p.Opad and r.tiles_p == -(-g.B * g.Ho * g.Wo // r.TP) and r.NGR == -(-g.C // r.NG), what
        assert sum(r.phase_taps) * r.NGR == r.n_steps and all(r.phase_taps[i] > 0 for i in range(r.n_phase)), what
        assert 1 <= r.slots <= 6 and r.slots == -(-r.NG * r.cells // r.NT) and r.lds_bytes <= 80 * 1024, what
        assert 1 <= r.max_images <= g.B and r.empty_phase == (r.n_phase < g.sh * g.sw), what
    else:
        assert not any(getattr(r, n) for n, _ in L.KanBandRoute._fields_ if n != "phase_taps") and not any(r.phase_taps), what
    if r.bw_band:
        assert p.bwd_weight_splits == r.bw_splits and (r.bw_WR, r.bw_NI) in BC.BW_TILES and r.bw_slots in BC.BW_SLOTS, what
        assert r.bw_TPI == -(-g.Ho * g.Wo // 128) and r.bw_ptiles == g.B * r.bw_TPI and r.bw_lds_bytes <= 80 * 1024, what
        assert (r.bw_slots == 6) == (r.NG * r.bw_cells > 3 * r.bw_WR * 64), what
    else:
        assert not any(getattr(r, n) for n, _ in L.KanBandRoute._fields_ if n.startswith("bw_")), what


def test_export_agrees_with_the_public_plan():
    """KC == NPLE, IPC == NG, Kpad == n_steps NPLE, the split counts and the two route flags -- on every row and on every 23rd grid launch, off the
    band route too -- and the arithmetic that ties the exported fields to each other."""
    for case in BAND_CASES:
        g, b, p = BC.case_structs(case)
        _agrees(g, b, BC.band_route(g, b), p, case)
    n = off = 0
    for i, c in enumerate(BC.grid()):
        if i % 23:
            continue
        g = BC.geom_of(c)
        for layer in BC.SPEC_LAYERS + ("legendre_d3", "relu_g5k3"):
            b = BC.basis_of(layer)
            r, p = BC.band_route(g, b), plan_of(g, b)
            _agrees(g, b, r, p, (layer, c))
            n += 1
            off += not r.fwd_band
    assert n > 15000 and off > 2000, (n, off)


def test_a_rejected_geometry_returns_the_planners_error():
    g, b, r = BC.geom_of(BAND_CASES[0]), BC.basis_of("kan_silu"), L.KanBandRoute()
    g.Ho += 1
    lib = L.load()
    assert lib.kan_band_route(ctypes.byref(g), ctypes.byref(b), ctypes.byref(r)) != 0 and b"Ho/Wo" in lib.kan_last_error()
    assert lib.kan_plan(ctypes.byref(g), ctypes.byref(b), ctypes.byref(L.KanPlan())) != 0
    assert not any(getattr(r, n) for n, _ in L.KanBandRoute._fields_ if n != "phase_taps")
    assert lib.kan_band_route(ctypes.byref(g), ctypes.byref(b), None) != 0


def test_legendre_never_and_fastkan_longer_on_the_band_route():
    """LegendreKAN (a second, pre-normalised tensor) never takes the band route.  FastKAN is never position-major, so on small padded planes with
    >= 16 images it keeps the band weight gradient where the B-spline specs leave it for the tap-skipping launch."""
    leg = BC.basis_of("legendre_d3")
    kept = 0
    for c in BC.grid():
        g = BC.geom_of(c)
        r = BC.band_route(g, leg)
        assert r is not None and not r.fwd_band and not r.bw_band, c
        if c["shape"] == "3x3" and c["H"] <= 4 and c["B"] >= 16:
            rs, rf = BC.band_route(g, BC.basis_of("kan_silu")), BC.band_route(g, BC.basis_of("fast_g8"))
            if rf.bw_band and rs.fwd_band:
                assert not rs.bw_band, c
                kept += 1
    assert kept > 50, kept


def test_deleting_a_row_fails():
    """Every single-row deletion, in a seeded order: each leaves a reached cell without a row or with a larger smallest row."""
    rows = row_cells()
    for i in random.Random(20261021).sample(range(len(rows)), len(rows)):
        missing, big = defects(rows[:i] + rows[i + 1:])
        assert missing or big, f"BAND_CASES without row {i} ({BC.case_id(BAND_CASES[i])}) lacks nothing"


@pytest.mark.parametrize("case", BAND_CASES, ids=case_ids(BAND_CASES))
def test_band_case_is_well_conditioned(case):
    """From the fp64 oracle: the share of the row's outputs within 1e-4 of the PReLU kink, which check_vs_oracle gives no upstream gradient."""
    from helpers import oracle_run
    layer, x = BC.built(case)
    if not hasattr(layer, "prelus"):                      # ChebyKAN, FastKAN: no PReLU, nothing is masked
        return
    import copy
    _, _, _, pre = oracle_run(BC.case_cfg(case, layer), layer, x, None, torch.float64)
    assert len(pre) == case["G"]
    norms = copy.deepcopy(layer.layer_norm).double()
    with torch.no_grad():
        n = torch.cat([norms[g](z.detach()) for g, z in enumerate(pre)], 1)
    share = float((n.abs() <= 1e-4).double().mean())
    assert share <= KINK_CAP, f"{case}: {share:.4f} of the outputs sit on the PReLU kink; give the row another seed"
