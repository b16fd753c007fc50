"""Every band cell (tests/band_cells.py: the smallest geometry of every k_band_fwd / k_band_bwd_weight instantiation and run-time switch that
`kan_band_route` reports on the committed grid, kept complete by tests/test_band_matrix.py) on the GPU.

Per row:
(a) the layer still plans to the instantiations the row declares, and the KernelSamples of one forward + backward under ops.PROFILE hold one
    k_band_fwd/o<TO> launch and a k_band_bwd_weight/.. launch exactly where the route says so;
(b) helpers.check_vs_oracle on the whole layer (y, dx, every parameter gradient; fallback=False): max(stated TOL_*, 4 x the fp32 oracle's own error
    on that tensor), no multiplier of its own;
(c) the conv stage alone, so that an InstanceNorm over a tiny plane cannot widen the yardstick: z of ops.kan_conv against the fp64 oracle's pre-norm
    sum, and the weight gradients [O, C n, kh, kw] of that stage against fp64 autograd, under the same rule (FastKAN has no norm behind its conv
    stage: its layer is the stage, and (b) is this check);
(d) two runs give bit-identical y, dx and weight gradients;
(e) rows with two or more images under a pixel tile: three images keep their z bit for bit when every other image of the batch is replaced, and
    when they run alone wherever the one-image launch sums in the same order (the same slab count);
(f) rows with a ragged pixel tile or ragged outputs: raw kan_conv_fwd and kan_conv_bwd_weight launches into slabs that sit inside a larger buffer of
    a finite sentinel -- every guard word intact, every slab word written, the summed slabs equal to what ops returns;
(g) NaN locality for every odd NG x P that has a row and one ragged-channel-group row per tile: one NaN pixel poisons exactly the outputs whose
    receptive field holds it (the SiLU B-spline spec and ChebyKAN; DESIGN.md 4f says why not GELU)."""
import copy
import ctypes as C

import pytest
import torch

import band_cells as BC
from band_cells import BAND_CASES, case_id
from helpers import TOL_DW, TOL_Y, check_vs_oracle, oracle_forward, relerr

pytestmark = pytest.mark.gpu

SENTINEL, PAD = 12345.0, 1 << 12
ROUTES = {case_id(c): BC.case_route(c) for c in BAND_CASES}          # host arithmetic: (geom, basis, route) per row


def _features(case):
    g, b, r = ROUTES[case_id(case)]
    return {cell[-1] for cell in BC.cells_of(g, b, r) if cell[0] == "Ff"}, {cell[-1] for cell in BC.cells_of(g, b, r) if cell[0] == "Wf"}


def _ids(cases):
    return [case_id(c) for c in cases]


def _stage_args(layer, x):
    """(spec, x, xn, base weights, basis weights) of the layer's conv stage as its forward hands them to ops.kan_conv.  FastKAN reads its basis from
    a second tensor (its normalised input): any finite tensor serves the conv stage, tanh(x) here."""
    import convkan_amd as K
    if isinstance(layer, K.FastKANConv2DLayer):
        return layer.conv_spec(), x, torch.tanh(x), [m.weight for m in layer.base_conv], [m.weight for m in layer.spline_conv]
    wb = [m.weight for m in layer.base_conv] if layer._has_base else []
    xa, xb = layer._base_input(x) if layer._has_base else (x, None)
    return layer.conv_spec(), xa, xb, wb, [m.weight for m in getattr(layer, layer._basis)]


def _stage(layer, x):
    from convkan_amd import ops
    return ops.kan_conv(*_stage_args(layer, x))


def _run(layer, x, go):
    layer.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    y = layer(xg)
    y.backward(go)
    torch.cuda.synchronize()
    return y.detach().clone(), xg.grad.clone(), {n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None and p.dim() >= 3}


@pytest.mark.parametrize("case", BAND_CASES, ids=_ids(BAND_CASES))
def test_band_cell_vs_oracle(case, gpu_lib, monkeypatch):
    from convkan_amd import ops
    layer, x = BC.built(case)
    g, b, p = BC.case_structs(case, layer)
    r = BC.band_route(g, b)
    assert [cell for cell in BC.cells_of(g, b, r) if cell[0] in ("F", "W")] == case["cells"], f"{case}: the layer plans to {BC.cells_of(g, b, r)}"
    errs = check_vs_oracle(layer, BC.case_cfg(case, layer), x, groups=case["G"], tag=case_id(case), fallback=False)
    print(f"[band] {case_id(case)} | {' '.join(BC.cell_id(c) for c in case['cells'])} | "
          + " ".join(f"{k}={v[0]:.2e}/{v[2]:.2e}" for k, v in sorted(errs.items())))

    xd = x.cuda()
    go = torch.randn(layer(xd).shape, generator=torch.Generator().manual_seed(7)).cuda()
    monkeypatch.setattr(ops, "PROFILE", [])
    y1, dx1, dw1 = _run(layer, xd, go)
    names = [s.name for s in ops.PROFILE]
    monkeypatch.setattr(ops, "PROFILE", None)
    assert [n for n in names if n.startswith(("k_conv_fwd", "k_band_fwd"))] == [f"k_band_fwd/o{r.TO}"], names
    bw = [n for n in names if "bwd_weight" in n]
    assert len(bw) == 1 and bw[0].startswith("k_band_bwd_weight/") == bool(r.bw_band), names
    y2, dx2, dw2 = _run(layer, xd, go)
    assert torch.equal(y1, y2), f"{case}: forward differs between two identical runs"
    assert torch.equal(dx1, dx2), f"{case}: input gradient differs between two identical runs"
    assert dw1.keys() == dw2.keys() and dw1
    for n in dw1:
        assert torch.equal(dw1[n], dw2[n]), f"{case}: gradient of {n} differs between two identical runs"


def _stage_oracle(cfg, layer, x, gz, dtype):
    """(z, {conv-weight gradients}) of the oracle's conv stage alone in `dtype`: the pre-norm sums of oracle_forward and autograd from them."""
    l2 = copy.deepcopy(layer).to(dtype)
    if hasattr(l2, "grid") and isinstance(l2.grid, torch.Tensor):
        l2.grid = l2.grid.to(dtype)
    pre = []
    oracle_forward(cfg, l2, x.to(dtype), pre)
    z = torch.cat(pre, 1)
    z.backward(gz.to(dtype))
    return z.detach(), {n: p.grad for n, p in l2.named_parameters() if p.grad is not None and p.dim() >= 3}


STAGE_CASES = [c for c in BAND_CASES if c["layer"] != "fast_g8"]


@pytest.mark.parametrize("case", STAGE_CASES, ids=_ids(STAGE_CASES))
def test_band_cell_conv_stage_vs_oracle(case, gpu_lib):
    layer, x = BC.built(case)
    cfg = BC.case_cfg(case, layer)
    Ho, Wo = BC.out_hw(case["shape"], case["H"], case["W"])
    gz = torch.randn(case["B"], case["O"], Ho, Wo, generator=torch.Generator().manual_seed(11))
    z64, dw64 = _stage_oracle(cfg, layer, x, gz, torch.float64)
    z32, dw32 = _stage_oracle(cfg, layer, x, gz, torch.float32)
    dev = layer.cuda()
    dev.zero_grad(set_to_none=True)
    z = _stage(dev, x.cuda())
    z.backward(gz.cuda())
    torch.cuda.synchronize()
    got = {n: p.grad for n, p in dev.named_parameters() if p.grad is not None}
    assert set(got) == set(dw64) and got, (sorted(got), sorted(dw64))
    errs = {"z": (relerr(z, z64), max(TOL_Y, 4.0 * relerr(z32, z64)), relerr(z32, z64))}
    for n in got:
        errs[n] = (relerr(got[n], dw64[n]), max(TOL_DW, 4.0 * relerr(dw32[n], dw64[n])), relerr(dw32[n], dw64[n]))
    print(f"[band-stage] {case_id(case)} | " + " ".join(f"{k}={v[0]:.2e}/{v[2]:.2e}" for k, v in sorted(errs.items())))
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, f"{case_id(case)}: (error, tolerance, fp32 oracle's own error) {bad}  (all: {errs})"


SHARED_CASES = [c for c in BAND_CASES if ROUTES[case_id(c)][2].max_images >= 2]


@pytest.mark.parametrize("case", SHARED_CASES, ids=_ids(SHARED_CASES))
def test_band_cell_is_independent_of_the_other_images(case, gpu_lib):
    layer, x = BC.built(case)
    g, b, r = ROUTES[case_id(case)]
    dev, xd, B = layer.cuda(), x.cuda(), case["B"]
    picks = sorted({0, B // 2, B - 1})
    with torch.no_grad():
        z = _stage(dev, xd)
        other = torch.randn(x.shape, generator=torch.Generator().manual_seed(13)).cuda() * 1.3
        for i in picks:
            other[i] = xd[i]
        z2 = _stage(dev, other)
        for i in picks:
            assert torch.equal(z2[i], z[i]), f"{case_id(case)}: z of image {i} depends on the other images of its pixel tile"
        g1 = BC.geom_of(dict(case, B=1))
        r1 = BC.band_route(g1, b)
        if r1.fwd_band and r1.fwd_splits == r.fwd_splits:          # the same slabs: the same order of every pixel's sum
            for i in picks:
                assert torch.equal(_stage(dev, xd[i:i + 1].contiguous())[0], z[i]), f"{case_id(case)}: image {i} run alone differs"


RAGGED_CASES = [c for c in BAND_CASES if _features(c)[0] & {"ragged-pixels", "ragged-O"} or _features(c)[1] & {"ragged-O", "partial-pixel-tile"}]


@pytest.mark.parametrize("case", RAGGED_CASES, ids=_ids(RAGGED_CASES))
def test_band_cell_raw_launches_stay_inside_their_slabs(case, gpu_lib):
    from convkan_amd import _lib as L
    from convkan_amd import ops
    lib = L.load()
    layer, x = BC.built(case)
    dev, xd = layer.cuda(), x.cuda()
    spec, xa, xn, wb, ws = _stage_args(dev, xd)
    geom, basis, plan = ops._plan_cached(*ops._plan_key(spec, xd.shape, case["O"] // case["G"]))
    basis = ops._with_table(basis, spec, xd.device)
    r = BC.band_route(geom, basis)
    assert plan.fwd_band and r.fwd_band
    st = ops._stream(xd)
    G, Ot = case["G"], case["O"]
    xs = xn if xn is not None else xa

    # ---- forward: fwd_splits slabs of [B][O][Ho][Wo]
    wp = torch.empty(plan.packed_weight_bytes // 4, device=xd.device)
    wb_all, ws_all = (ops._stack(wb) if wb else None), ops._stack(ws)
    L.check(lib.kan_pack_weights(ops._ptr(wb_all), ops._ptr(ws_all), ops._ptr(wp), None, C.byref(geom), C.byref(basis), st), "kan_pack_weights")
    S, n = plan.fwd_splits, plan.fwd_slab_elems
    assert n == geom.B * Ot * geom.Ho * geom.Wo
    big = torch.full((S * n + 2 * PAD,), SENTINEL, device=xd.device)
    L.check(lib.kan_conv_fwd(ops._ptr(xa), ops._ptr(xs), ops._ptr(wp), ops._ptr(big, PAD), C.byref(geom), C.byref(basis), None, st), "kan_conv_fwd")
    torch.cuda.synchronize()
    assert bool((big[:PAD] == SENTINEL).all()) and bool((big[PAD + S * n:] == SENTINEL).all()), "the forward wrote outside its slabs"
    assert bool((big[PAD:PAD + S * n] != SENTINEL).all()), "the forward left slab words unwritten"
    zsum = ops._sum_slabs(big[PAD:PAD + S * n].view(S, geom.B, Ot, geom.Ho, geom.Wo), geom.B, Ot, geom.Ho * geom.Wo)
    dev.zero_grad(set_to_none=True)
    z = ops.kan_conv(spec, xa, xn, wb, ws)
    assert torch.equal(zsum, z.detach()), "the summed slabs of the raw forward differ from ops.kan_conv"

    # ---- weight gradient: bwd_weight_splits slabs of bwd_weight_slab_elems floats, unpacked by the library
    if not r.bw_band:
        return
    gz = torch.randn(z.shape, generator=torch.Generator().manual_seed(17)).cuda()
    z.backward(gz)
    S, n = plan.bwd_weight_splits, plan.bwd_weight_slab_elems
    assert S == r.bw_splits and n == G * plan.Kpad * plan.Opad
    big = torch.full((S * n + 2 * PAD,), SENTINEL, device=xd.device)
    L.check(lib.kan_conv_bwd_weight(ops._ptr(gz), ops._ptr(xa), ops._ptr(xs), ops._ptr(big, PAD), C.byref(geom), C.byref(basis), None, None, st),
            "kan_conv_bwd_weight")
    torch.cuda.synchronize()
    assert bool((big[:PAD] == SENTINEL).all()) and bool((big[PAD + S * n:] == SENTINEL).all()), "the weight gradient wrote outside its slabs"
    assert bool((big[PAD:PAD + S * n] != SENTINEL).all()), "the weight gradient left slab words unwritten"
    kh, kw = spec.kernel
    dwb = torch.full((G, geom.O, geom.C, kh, kw), SENTINEL, device=xd.device) if wb else None
    dws = torch.full((G, geom.O, geom.C * spec.n_basis, kh, kw), SENTINEL, device=xd.device)
    L.check(lib.kan_unpack_wgrad(ops._ptr(big, PAD), ops._ptr(dwb), ops._ptr(dws), C.byref(geom), C.byref(basis), st), "kan_unpack_wgrad")
    torch.cuda.synchronize()
    for gi in range(G):
        assert torch.equal(dws[gi], ws[gi].grad), f"group {gi}: the unpacked raw basis-weight gradient differs from ops"
        if wb:
            assert torch.equal(dwb[gi], wb[gi].grad), f"group {gi}: the unpacked raw base-weight gradient differs from ops"


def _nan_keys(c, r):
    return ([("pad-row", r.NG, r.P)] if (r.NG * r.P) & 1 else []) + ([("ragged-group", r.MO, r.WP)] if (c["C"] // c["G"]) % r.NG else [])


def _nan_cases():
    """First row of every odd NG x P (the zero pad row) and, per tile, of a ragged channel group, among the SiLU B-spline and ChebyKAN rows; a GELU
    B-spline row runs as the SiLU layer of its geometry (the two specs plan alike; the ragged groups under the 192-output tile are GELU rows)."""
    seen, out = set(), []
    for c in BAND_CASES:
        if c["layer"] not in ("kan_silu", "kan_gelu", "cheby_d4"):
            continue
        c = dict(c, layer="kan_silu") if c["layer"] == "kan_gelu" else c
        r = BC.case_route(c)[2]
        new = [k for k in _nan_keys(c, r) if k not in seen]
        if new:
            seen.update(new)
            out.append(c)
    return out


NAN_CASES = _nan_cases()


def test_nan_rows_cover_every_odd_plane_count_and_every_tile_with_a_ragged_group():
    keys = {k for c in NAN_CASES for k in _nan_keys(c, BC.case_route(c)[2])}
    assert {("pad-row", 1, 9), ("pad-row", 3, 9), ("pad-row", 1, 5), ("pad-row", 3, 5)} <= keys, keys
    ragged = {(r.MO, r.WP) for g, b, r in ROUTES.values() if g.C % r.NG}
    assert {k[1:] for k in keys if k[0] == "ragged-group"} == ragged and len(ragged) == 3, (keys, ragged)      # 128-output tiles take even C only


@pytest.mark.parametrize("case", NAN_CASES, ids=_ids(NAN_CASES))
def test_band_cell_nan_stays_local(case, gpu_lib):
    layer, x = BC.built(case)
    g, b, r = BC.case_route(case)
    B, Ct, G = case["B"], case["C"], case["G"]
    bi, ci, i0, j0 = B - 1, Ct - 1, case["H"] // 2, case["W"] // 2          # the last channel: the one of a ragged group
    x[bi, ci, i0, j0] = float("nan")
    with torch.no_grad():
        z = _stage(layer.cuda(), x.cuda()).cpu()
    want = torch.zeros(z.shape, dtype=torch.bool)
    Og, grp = case["O"] // G, ci // (Ct // G)
    for ho in range(g.Ho):
        for wo in range(g.Wo):
            hit = any(ho * g.sh - g.ph + rr * g.dh == i0 for rr in range(g.kh)) and any(wo * g.sw - g.pw + t * g.dw == j0 for t in range(g.kw))
            if hit:
                want[bi, grp * Og:(grp + 1) * Og, ho, wo] = True
    assert bool(want.any()), "the NaN pixel lies in no receptive field: move it"
    assert torch.equal(torch.isnan(z), want), f"{case_id(case)}: {int(torch.isnan(z).sum())} NaN outputs, {int(want.sum())} hold the pixel"
