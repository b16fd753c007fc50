"""2x2 planes under 3x3 / stride 1 / pad 1: the expanded forward with the four output positions on the weight side of a tile
(KAN_ORDER_FWD_WEIGHT_SIDE: 32 outputs x 4 positions x 128 images, 16-byte stores) against the one-position order it replaces there.

Both orders cut the same live steps into the same splits and add the same 18 rows per step in the same order, so every slab must be
bit-identical: kan_conv_fwd_expanded_order runs both on one e_pm and one wp, the slabs are compared with torch.equal one by one, and
guard words either side of z show that nothing else is written.  The layer then runs once through ops against the fp64 oracle.

Shapes (B, C, O, groups; C and O are totals) are the smallest the route admits (B % 128 == 0, outputs per group padded to a multiple of 128):
one channel pair; a ragged output tile whose second split starts inside an input position (3 pairs per position, 12 steps cut 6 + 6);
O = 100, which ends inside a wave's 16 outputs (whole 16-byte groups are masked); two image tiles with 16 splits; and two groups in
grid.y -- 128 outputs PER GROUP, since 64 per group pad to 64 and leave the expanded route."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import convkan_amd as K
from helpers import check_vs_oracle

pytestmark = pytest.mark.gpu

SHAPES = [(128, 2, 128, 1), (128, 6, 96, 1), (128, 64, 100, 1), (256, 64, 256, 1), (128, 4, 256, 2)]
IDS = ["one_pair", "ragged_o_tile_split_inside_p", "o100_group_mask", "two_image_tiles_split_k", "groups2"]
SENTINEL, PAD = 12345.0, 1 << 12


def _setup(B, Ct, Ot, G):
    from convkan_amd import _lib as L
    from convkan_amd import ops
    lib = L.load()
    layer = K.KANConv2DLayer(Ct, Ot, 3, padding=1, groups=G, base_activation=nn.SiLU).cuda()
    spec = layer.conv_spec()
    x = (torch.randn(B, Ct, 2, 2) * 1.5).cuda()
    geom, basis, plan = ops._plan_cached(*ops._plan_key(spec, x.shape, Ot // G))
    basis = ops._with_table(basis, spec, x.device)
    st = ops._stream(x)
    wb = torch.stack([m.weight.detach() for m in layer.base_conv]).contiguous()
    ws = torch.stack([m.weight.detach() for m in layer.spline_conv]).contiguous()
    wp = torch.empty(plan.packed_weight_bytes // 4, device=x.device)
    L.check(lib.kan_pack_weights(ops._ptr(wb), ops._ptr(ws), ops._ptr(wp), None, C.byref(geom), C.byref(basis), st), "kan_pack_weights")
    e_pm = ops._expand_pm(x, geom, basis, plan, st)
    return layer, x, geom, basis, plan, wp, e_pm, st


@pytest.mark.parametrize("B,Ct,Ot,G", SHAPES, ids=IDS)
def test_weight_side_slabs_equal_the_one_position_slabs_bitwise(B, Ct, Ot, G, gpu_lib):
    from convkan_amd import _lib as L
    from convkan_amd import ops
    lib = L.load()
    torch.manual_seed(B + Ct + Ot)
    layer, x, geom, basis, plan, wp, e_pm, st = _setup(B, Ct, Ot, G)
    assert plan.fwd_expanded and plan.tile_orders & L.ORDER_FWD_WEIGHT_SIDE
    S, n = plan.fwd_splits, plan.fwd_slab_elems
    assert n == B * Ot * 4
    out = {}
    for order in (0, L.ORDER_FWD_WEIGHT_SIDE):
        big = torch.full((S * n + 2 * PAD,), SENTINEL, device=x.device)
        L.check(lib.kan_conv_fwd_expanded_order(ops._ptr(e_pm), ops._ptr(wp), ops._ptr(big, PAD), C.byref(geom), C.byref(basis), st, order),
                "kan_conv_fwd_expanded_order")
        torch.cuda.synchronize()
        assert bool((big[:PAD] == SENTINEL).all()) and bool((big[PAD + S * n:] == SENTINEL).all()), order
        out[order] = big[PAD:PAD + S * n].view(S, n)
        assert bool((out[order] != SENTINEL).all()), order                 # every element of every slab is written
    print(f"[fwd weight side B={B} C={Ct} O={Ot} G={G}] splits {S}, target {plan.fwd_target}")
    for s in range(S):
        assert torch.equal(out[0][s], out[L.ORDER_FWD_WEIGHT_SIDE][s]), s
    assert bool(out[0].sum(0).abs().max() > 0)
    z = torch.empty(S * n, device=x.device)                                # and the planner's own choice is the weight-side kernel's result
    L.check(lib.kan_conv_fwd_expanded(ops._ptr(e_pm), ops._ptr(wp), ops._ptr(z), C.byref(geom), C.byref(basis), st), "kan_conv_fwd_expanded")
    torch.cuda.synchronize()
    assert torch.equal(z.view(S, n), out[0])


def test_forced_order_is_refused_where_the_geometry_does_not_offer_it(gpu_lib):
    """A 2x2 plane under stride 2 takes the expanded route but not the weight-side order: forcing it fails before any launch."""
    from convkan_amd import _lib as L
    from convkan_amd import ops
    lib = L.load()
    layer = K.KANConv2DLayer(2, 96, 3, stride=2, padding=1, base_activation=nn.SiLU).cuda()
    x = torch.randn(128, 2, 3, 3, device="cuda")
    geom, basis, plan = ops._plan_cached(*ops._plan_key(layer.conv_spec(), x.shape, 96))
    assert plan.fwd_expanded and not plan.tile_orders & L.ORDER_FWD_WEIGHT_SIDE
    p = ops._ptr(x)
    assert lib.kan_conv_fwd_expanded_order(p, p, p, C.byref(geom), C.byref(basis), ops._stream(x), L.ORDER_FWD_WEIGHT_SIDE) < 0
    assert "weight-side" in lib.kan_last_error().decode()
    assert lib.kan_conv_fwd_expanded_order(p, p, p, C.byref(geom), C.byref(basis), ops._stream(x), 3) < 0


@pytest.mark.parametrize("B,Ct,Ot,G", SHAPES, ids=IDS)
def test_layer_on_the_weight_side_order_vs_oracle(B, Ct, Ot, G, gpu_lib):
    from convkan_amd import _lib as L
    from convkan_amd import ops
    torch.manual_seed(Ot + B)
    layer = K.KANConv2DLayer(Ct, Ot, 3, padding=1, groups=G, base_activation=nn.SiLU)
    _, _, plan = ops._plan_cached(layer.conv_spec(), B, Ct // G, 2, 2, Ot // G, Ct, Ot)
    assert plan.fwd_expanded and plan.tile_orders & L.ORDER_FWD_WEIGHT_SIDE
    check_vs_oracle(layer, dict(kind="bspline", C=Ct, O=Ot, k=3, s=1, p=1, d=1, groups=G, act="silu"), torch.randn(B, Ct, 2, 2) * 1.5, groups=G)
