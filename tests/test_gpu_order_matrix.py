"""Every tile-order cell (tests/order_cells.py: one row per reachable (spec class, kan_tile_orders bits, grouped?, fwd, bwd-data, bwd-weight) key, kept
complete by tests/test_order_matrix.py) on the GPU.

Per row:
(a) the layer still plans to the row's key, the predicates ops.py dispatches on agree with the bits, and the KernelSamples of one forward + backward
    under ops.PROFILE show the order was taken: a k_conv_bwd_weight_pos8 launch for the 8x8 weight gradient, executed / dense FLOPs of 484/576 for the 8x8
    bwd-data tiles, 11/12 for the 8x8 half-plane forward, the live fraction for the quadrant and weight-side orders;
(b) forward, input gradient and every parameter gradient meet check_vs_oracle's tolerance against the oneDNN fp32 execution alone (fallback=False);
(c) two runs on the same inputs give bit-identical y, dx and conv-weight gradients;
(d) rows with a forward or bwd-data order: a fixed seeded permutation of the batch that moves images across the tiles of the order (32-image groups; 4
    for the 8x8 forward), applied to x and to the incoming gradient, gives the permuted y and dx bit for bit -- these tiles mix images, and the order
    of every pixel's sum depends on its plane position and slab only, never on the image's slot."""
import pytest
import torch

from helpers import check_vs_oracle
from order_cells import GROUP_OF, ORDER_CASES, STAGE_OF, case_ids, order_key, perm_batch
from route_cells import case_cfg, case_layer, case_structs
from test_gpu_route_matrix import _perturb, _run

pytestmark = pytest.mark.gpu


def _built(case):
    torch.manual_seed(0)
    layer = case_layer(case)
    gen = torch.Generator().manual_seed(1)
    _perturb(layer, case, gen)
    return layer, gen


def _check_samples(case, g, p, samples):
    """(a): the launches of one forward + backward, as ops.py named and counted them."""
    from convkan_amd import ops
    names = case["key"][1]
    lf = lambda which: ops._live_fraction(which, g.H, g.W, g.Ho, g.Wo, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, g.dh, g.dw)
    fwd = [s for s in samples if s.name.startswith(("k_conv_fwd", "k_band_fwd"))]
    bd = [s for s in samples if s.name == "k_conv_bwd_data"]
    bw = [s for s in samples if "bwd_weight" in s.name]
    assert len(fwd) == 1 and len(bd) == 1 and len(bw) == 1, [s.name for s in samples]
    assert bw[0].name.startswith("k_conv_bwd_weight_pos8/") == ("POS8_BWD_WEIGHT" in names), bw[0].name
    if "POS8_BWD_WEIGHT" in names:
        assert bw[0].executed == bw[0].flops * (484.0 / 576.0)
    assert (bd[0].executed == bd[0].flops * (484.0 / 576.0)) == ("POS8_BWD_DATA" in names), (bd[0].executed, bd[0].flops)
    if "QUAD_BWD_DATA" in names:
        # the launcher takes the quadrant tiles when it is given dz_pm, and ops builds that copy only where the plan wants it for the weight gradient
        # (an EXPANDED or TAP-PM one): under a HALO weight gradient the bit is an offer ops does not take up, and bwd-data stays on the row blocks
        assert lf("bwd_data") < 5.0 / 6.0
        assert bd[0].executed == bd[0].flops * (lf("bwd_data") if p.dz_pm_wanted else 5.0 / 6.0), (bd[0].executed / bd[0].flops, p.dz_pm_wanted)
        assert bool(p.dz_pm_wanted) == (case["key"][5] != "HALO")
    assert (fwd[0].name.startswith("k_conv_fwd_halo/") and fwd[0].executed == fwd[0].flops * (11.0 / 12.0)) == ("ROWBLK8_FWD" in names), fwd[0]
    if "QUAD_FWD" in names:
        assert fwd[0].name.startswith("k_conv_fwd_halo/") and fwd[0].executed == fwd[0].flops * lf("fwd") < fwd[0].flops * (5.0 / 6.0)
    if "FWD_WEIGHT_SIDE" in names:
        assert fwd[0].name.startswith("k_conv_fwd_pmdma/") and fwd[0].executed == fwd[0].flops * lf("fwd") < fwd[0].flops


@pytest.mark.parametrize("case", ORDER_CASES, ids=case_ids(ORDER_CASES))
def test_order_cell_vs_oracle(case, gpu_lib, monkeypatch):
    from convkan_amd import _lib as L
    from convkan_amd import ops
    layer, gen = _built(case)
    g, b, p = case_structs(case, layer)
    names = case["key"][1]
    assert order_key(g, b, p) == case["key"], f"{case}: the layer plans to {order_key(g, b, p)}"
    assert ops._quadrant_order(g, p, "fwd") == ("QUAD_FWD" in names)
    assert ops._quadrant_bwd_data(g, p, True) == ("QUAD_BWD_DATA" in names) and not ops._quadrant_bwd_data(g, p, False)
    assert ops._row_blocks8_forward(g, p) == ("ROWBLK8_FWD" in names)
    assert ops._pos8_bwd_data(g, p) == ("POS8_BWD_DATA" in names)
    assert ops._pos8_bwd_weight(g, p) == ("POS8_BWD_WEIGHT" in names)
    assert bool(p.tile_orders & L.ORDER_FWD_WEIGHT_SIDE) == ("FWD_WEIGHT_SIDE" in names)
    x = torch.randn(case["B"], case["C"], case["H"], case["W"], generator=gen) * case.get("scale", 1.0)
    check_vs_oracle(layer, case_cfg(case, layer), x, groups=case["G"], tag=case, fallback=False)

    xd = x.cuda()
    go = torch.randn(layer(xd).shape, generator=gen).cuda()
    monkeypatch.setattr(ops, "PROFILE", [])
    y1, dx1, dw1 = _run(layer, xd, go)
    samples = list(ops.PROFILE)
    monkeypatch.setattr(ops, "PROFILE", None)
    _check_samples(case, g, p, samples)
    y2, dx2, dw2 = _run(layer, xd, go)
    assert torch.equal(y1, y2), f"{case}: forward differs between two identical runs"
    assert torch.equal(dx1, dx2), f"{case}: input gradient differs between two identical runs"
    assert dw1.keys() == dw2.keys() and dw1, f"{case}: no conv-weight gradients to compare"
    for n in dw1:
        assert torch.equal(dw1[n], dw2[n]), f"{case}: gradient of {n} differs between two identical runs"


PERM_CASES = [c for c in ORDER_CASES if any(STAGE_OF[n] != "bw" for n in c["key"][1])]


@pytest.mark.parametrize("case", PERM_CASES, ids=case_ids(PERM_CASES))
def test_order_cell_is_independent_of_the_image_order(case, gpu_lib):
    layer, gen = _built(case)
    B = perm_batch(case)
    g, b, p = case_structs(dict(case, B=B), layer)
    assert order_key(g, b, p) == case["key"]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(20261021))
    for n in case["key"][1]:
        grp = GROUP_OF.get(n)
        if grp is not None and B > grp:
            assert bool((perm // grp != torch.arange(B) // grp).any()), f"the permutation moves no image across the {grp}-image groups of {n}"
    assert not torch.equal(perm, torch.arange(B))
    layer = layer.cuda()
    x = (torch.randn(B, case["C"], case["H"], case["W"], generator=gen) * case.get("scale", 1.0)).cuda()
    go = torch.randn(layer(x).shape, generator=gen).cuda()
    perm = perm.cuda()
    y, dx, _ = _run(layer, x, go)
    yp, dxp, _ = _run(layer, x[perm].contiguous(), go[perm].contiguous())
    assert torch.equal(yp, y[perm]), f"{case} at B = {B}: the forward of an image depends on its place in the batch"
    assert torch.equal(dxp, dx[perm]), f"{case} at B = {B}: the input gradient of an image depends on its place in the batch"
