"""The weight gradient on 8x8 planes with exact tap skipping (k_conv_bwd_weight_pos8; kan_tile_orders bit KAN_ORDER_POS8_BWD_WEIGHT): a wave owns 32
(channel, plane) pairs under all nine taps, a band is two images and a k-pair one plane position of both, so the taps without a source inside the plane are
not issued (484 of 576 blocks).

Shapes (C -> O, B): 4 -> 32, B = 2 (one full and one partial row group, one band); 8 -> 160, B = 4 (groups straddling channels, an output tail past one
128-tile; run a second time inside tensors of 11 / 163 channels: padded batch strides); 11 -> 128, B = 6 (odd channel count; three bands under two splits,
2 + 1).  Checked: the layer against the fp64 oracle (helpers.check_vs_oracle: max(TOL_DW, 4 x the fp32 oracle's own error)); the raw launch
(kan_conv_bwd_weight_rowgroups + kan_unpack_wgrad_rowgroups) against the plan's route (kan_conv_bwd_weight + kan_unpack_wgrad, which this change leaves alone) at
max-normalised <= 1e-6 on the unpacked gradients; guard words either side of the slabs; padded strides against the same values in dense tensors, bit for
bit; the same against the plan's route for GELU (the kernel's second instantiation); a two-group launch (11 channels and 40 outputs per group, B = 4 and
B = 6) against its groups launched alone through padded strides, bit for bit, with group 0's gradients exact zeros when only group 1 has a dz; single products (one input position, one dz position) landing in exactly their tap, bit-equal to the plan's route; odd B, where the entry is not
offered, and ops with the entry withheld running the plan's route."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import convkan_amd as K
from helpers import check_vs_oracle, relerr

pytestmark = pytest.mark.gpu

SHAPES = [(4, 32, 2, 4, 32), (8, 160, 4, 8, 160), (11, 128, 6, 11, 128), (8, 160, 4, 11, 163)]
IDS = ["c4_o32_b2_partial_group", "c8_o160_b4_output_tail", "c11_o128_b6_two_splits", "c8_o160_b4_padded_strides"]
SENTINEL, PAD = 12345.0, 1 << 12


def _geom(layer, B, Cn, On, Ct, Ot):
    from convkan_amd import ops
    geom, basis, _ = ops._plan_cached(layer.conv_spec(), B, Cn, 8, 8, On, Ct, Ot)
    return geom, basis


def _run(layer, geom, basis, x, dz, off=False, x_off=0, dz_off=0):
    """One weight-gradient launch into guarded slabs + its unpack: the 8x8 entry, or (off) the plan's route.  (plan, slabs, tile orders, dw_base, dw_spline);
    the gradients are [O, ..] of a single-group geometry and [G, O, ..] of a grouped one.  `x_off`, `dz_off`: the launch reads x and dz from that many
    floats into the tensors (the channels of one group of a wider tensor: padded batch strides)."""
    from convkan_amd import _lib as L
    from convkan_amd import ops
    lib = L.load()
    st = ops._stream(x)
    basis = ops._with_table(basis, layer.conv_spec(), x.device)
    plan = L.KanPlan()
    L.check(lib.kan_plan(C.byref(geom), C.byref(basis), C.byref(plan)), "kan_plan")
    orders = lib.kan_tile_orders(C.byref(geom), C.byref(basis))
    groups = max(1, geom.groups)
    S, n = (plan.bwd_weight_splits, plan.bwd_weight_slab_elems) if off else (lib.kan_bwd_weight_rowgroup_slabs(C.byref(geom), C.byref(basis)), groups * plan.K * plan.Opad)
    assert S >= 1
    big = torch.full((S * n + 2 * PAD,), SENTINEL, device=x.device)
    if off:
        L.check(lib.kan_conv_bwd_weight(ops._ptr(dz, dz_off), ops._ptr(x, x_off), ops._ptr(x, x_off), ops._ptr(big, PAD), C.byref(geom), C.byref(basis), None, None, st),
                "kan_conv_bwd_weight")
    else:
        L.check(lib.kan_conv_bwd_weight_rowgroups(ops._ptr(dz, dz_off), ops._ptr(x, x_off), ops._ptr(big, PAD), C.byref(geom), C.byref(basis), st),
                "kan_conv_bwd_weight_rowgroups")
    torch.cuda.synchronize()
    assert bool((big[:PAD] == SENTINEL).all()) and bool((big[PAD + S * n:] == SENTINEL).all()), off
    assert bool((big[PAD:PAD + S * n] != SENTINEL).all()), off                     # every word of every slab is written
    dwb = torch.full((groups, geom.O, geom.C, 3, 3), SENTINEL, device=x.device)
    dws = torch.full((groups, geom.O, geom.C * 8, 3, 3), SENTINEL, device=x.device)
    unpack = lib.kan_unpack_wgrad if off else lib.kan_unpack_wgrad_rowgroups
    L.check(unpack(ops._ptr(big, PAD), ops._ptr(dwb), ops._ptr(dws), C.byref(geom), C.byref(basis), st), "kan_unpack_wgrad")
    torch.cuda.synchronize()
    return (plan, S, orders, dwb[0], dws[0]) if groups == 1 else (plan, S, orders, dwb, dws)


@pytest.mark.parametrize("Cn,On,B,Ct,Ot", SHAPES, ids=IDS)
def test_pos8_dw_against_the_route_it_replaces_and_guard_words(Cn, On, B, Ct, Ot, gpu_lib):
    _against_the_plans_route(nn.SiLU, Cn, On, B, Ct, Ot)


@pytest.mark.parametrize("Cn,On,B,Ct,Ot", SHAPES, ids=IDS)
def test_pos8_dw_gelu_against_the_route_it_replaces_and_guard_words(Cn, On, B, Ct, Ot, gpu_lib):
    """The kernel's other instantiation (FAST_BSPLINE_GELU): the base plane is GELU(x)."""
    _against_the_plans_route(nn.GELU, Cn, On, B, Ct, Ot)


def _against_the_plans_route(act, Cn, On, B, Ct, Ot):
    from convkan_amd import _lib as L
    torch.manual_seed(Cn + On + B)
    layer = K.KANConv2DLayer(Cn, On, 3, padding=1, base_activation=act).cuda()
    geom, basis = _geom(layer, B, Cn, On, Ct, Ot)
    x = (torch.randn(B, Ct, 8, 8) * 1.5).cuda()
    dz = torch.randn(B, Ot, 8, 8).cuda()
    plan, S, orders, nb, ns = _run(layer, geom, basis, x, dz)
    assert orders & L.ORDER_POS8_BWD_WEIGHT and S == (2 if B == 6 else 1)
    _, S_old, _, ob, os_ = _run(layer, geom, basis, x, dz, off=True)
    eb, es = relerr(nb, ob), relerr(ns, os_)
    print(f"[pos8 bwd-weight C={Cn} O={On} B={B} in {Ct}/{Ot}] slabs {S} (the plan's route {S_old}, halo {plan.bwd_weight_halo} band "
          f"{plan.bwd_weight_band}); vs the plan's route: base {eb:.3e} spline {es:.3e}")
    assert bool(ob.abs().max() > 0) and bool(os_.abs().max() > 0)
    assert eb <= 1e-6 and es <= 1e-6
    if Ct != Cn:                                     # padded strides move addresses only: the same bits as the same values in dense tensors
        gd, bd = _geom(layer, B, Cn, On, Cn, On)
        _, _, _, db, ds = _run(layer, gd, bd, x[:, :Cn].contiguous(), dz[:, :On].contiguous())
        assert torch.equal(nb, db) and torch.equal(ns, ds)


@pytest.mark.parametrize("B", [4, 6], ids=["b4_one_slab", "b6_two_slabs"])
def test_pos8_dw_of_a_grouped_launch_equals_its_groups_launched_alone(B, gpu_lib):
    """Two groups of 11 channels and 40 outputs (an odd channel count; an output tail inside one 64-pad) in one launch -- the kernel's own group arithmetic:
    grp = blk.y / tiles_o, x += grp * C * 64, dz += grp * O * 64, dwp += grp * K * Opad, slabs of G * K * Opad -- against one single-group launch of the same
    entry per group on the same tensors (22 / 80 channels wide, the pointers moved to the group's channels).  The same slab count gives the same sum order:
    bit equality; otherwise the 1e-6 max-normalised bound between two weight-gradient routes.  Guard words either side of S * G * K * Opad and every slab
    word written (_run); against the plan's grouped route; and with dz zero outside group 1's outputs, group 0's gradients are exact zeros."""
    from convkan_amd import _lib as L
    G, Cg, Og = 2, 11, 40
    torch.manual_seed(B)
    grouped = K.KANConv2DLayer(G * Cg, G * Og, 3, padding=1, groups=G, base_activation=nn.SiLU).cuda()
    alone = K.KANConv2DLayer(Cg, Og, 3, padding=1, base_activation=nn.SiLU)
    gg, bg = _geom(grouped, B, Cg, Og, G * Cg, G * Og)
    g1, b1 = _geom(alone, B, Cg, Og, G * Cg, G * Og)
    assert gg.groups == G and max(1, g1.groups) == 1 and (g1.C, g1.O, g1.x_bstride, g1.y_bstride) == (gg.C, gg.O, gg.x_bstride, gg.y_bstride)
    x = (torch.randn(B, G * Cg, 8, 8) * 1.5).cuda()
    dz = torch.randn(B, G * Og, 8, 8).cuda()
    plan, S, orders, nb, ns = _run(grouped, gg, bg, x, dz)
    assert orders & L.ORDER_POS8_BWD_WEIGHT and S == (2 if B == 6 else 1) and tuple(nb.shape) == (G, Og, Cg, 3, 3) and tuple(ns.shape) == (G, Og, Cg * 8, 3, 3)
    assert bool((nb != SENTINEL).all()) and bool((ns != SENTINEL).all())                  # the unpack wrote both groups
    for g in range(G):
        _, S1, o1, ab, as_ = _run(alone, g1, b1, x, dz, x_off=g * Cg * 64, dz_off=g * Og * 64)
        assert o1 & L.ORDER_POS8_BWD_WEIGHT and bool(ab.abs().max() > 0) and bool(as_.abs().max() > 0)
        eb, es = relerr(nb[g], ab), relerr(ns[g], as_)
        print(f"[pos8 bwd-weight G=2 B={B}] group {g}: slabs {S} grouped, {S1} alone; base {eb:.3e} spline {es:.3e}")
        if S1 == S:
            assert torch.equal(nb[g], ab) and torch.equal(ns[g], as_), g
        else:
            assert eb <= 1e-6 and es <= 1e-6, g
    _, _, _, ob, os_ = _run(grouped, gg, bg, x, dz, off=True)
    assert relerr(nb, ob) <= 1e-6 and relerr(ns, os_) <= 1e-6
    dz1 = dz.clone()
    dz1[:, :Og] = 0.0
    _, _, _, zb, zs = _run(grouped, gg, bg, x, dz1)
    assert bool((zb[0] == 0).all()) and bool((zs[0] == 0).all())
    assert torch.equal(zb[1], nb[1]) and torch.equal(zs[1], ns[1])


@pytest.mark.parametrize("Cn,On,B", [s[:3] for s in SHAPES[:3]], ids=IDS[:3])
def test_pos8_layer_vs_oracle(Cn, On, B, gpu_lib):
    from convkan_amd import _lib as L
    from convkan_amd import ops
    torch.manual_seed(On + B)
    layer = K.KANConv2DLayer(Cn, On, 3, padding=1, base_activation=nn.SiLU)
    plan = ops._plan_cached(layer.conv_spec(), B, Cn, 8, 8, On, Cn, On)[2]
    assert plan.tile_orders & L.ORDER_POS8_BWD_WEIGHT
    errs = check_vs_oracle(layer, dict(kind="bspline", C=Cn, O=On, k=3, s=1, p=1, d=1, groups=1, act="silu"), torch.randn(B, Cn, 8, 8) * 1.5)
    print(f"[pos8 layer C={Cn} O={On} B={B}] (error, tolerance, fp32 oracle's own): " + ", ".join(f"{k} {v}" for k, v in errs.items() if "conv" in k))


# (image, row, column) of the one live input value and of the one live dz value; the tap (r, t) that pairs them (input = output - 1 + tap), or None
ISOLATED = [((1, 1, 1), (1, 0, 0), (2, 2)),          # corner output: four live taps, this is the last
            ((0, 0, 2), (0, 0, 3), (1, 0)),          # top-edge output, the tap to its left
            ((1, 3, 6), (1, 4, 5), (0, 2)),          # interior output, up and right
            ((0, 7, 7), (0, 7, 7), (1, 1)),          # bottom-right corner, centre tap
            ((1, 7, 0), (1, 6, 0), (2, 1)),          # left-edge output reading the bottom row
            ((0, 3, 6), (1, 4, 5), None)]            # input and dz in different images of the band: nothing


def test_single_products_land_in_exactly_their_tap(gpu_lib):
    """x = -1e4 expands to exact zeros on every plane (outside the grid; SiLU's reciprocal underflows to 0), x = 0.3 to the base plane and four spline
    planes: with one such input value and one non-zero dz value every gradient entry is a single product or an exact zero -- a skipped live tap, a wrong
    shift or a mixed-up k-half moves the pattern, which a tolerance test can hide under the other products."""
    from convkan_amd import _lib as L
    Cn, On, B, c, o = 4, 32, 2, 3, 17                # channel 3 = pairs 27 .. 35: straddles the two row groups
    layer = K.KANConv2DLayer(Cn, On, 3, padding=1, base_activation=nn.SiLU).cuda()
    geom, basis = _geom(layer, B, Cn, On, Cn, On)
    for (xb, xh, xw), (zb, zh, zw), tap in ISOLATED:
        x = torch.full((B, Cn, 8, 8), -1e4)
        x[xb, c, xh, xw] = 0.3
        dz = torch.zeros(B, On, 8, 8)
        dz[zb, o, zh, zw] = 1.5
        _, _, orders, nb, ns = _run(layer, geom, basis, x.cuda(), dz.cuda())
        assert orders & L.ORDER_POS8_BWD_WEIGHT
        _, _, _, ob, os_ = _run(layer, geom, basis, x.cuda(), dz.cuda(), off=True)
        want_b, want_s = torch.zeros(On, Cn, 3, 3, dtype=torch.bool), torch.zeros(On, Cn * 8, 3, 3, dtype=torch.bool)
        if tap is not None:
            assert (xh, xw) == (zh - 1 + tap[0], zw - 1 + tap[1])
            want_b[o, c, tap[0], tap[1]] = True
            want_s[o, c * 8:(c + 1) * 8, tap[0], tap[1]] = True
        case = ((xb, xh, xw), (zb, zh, zw))
        assert torch.equal(nb.cpu() != 0, want_b), case
        assert not bool(((ns.cpu() != 0) & ~want_s).any()), case
        assert int((ns != 0).sum()) == (4 if tap is not None else 0), case            # a cubic spline: four live bases at x = 0.3
        assert torch.equal(nb, ob) and torch.equal(ns, os_), case                       # single products: the old route's bits


def test_odd_batch_and_a_withheld_entry_run_the_plans_route(gpu_lib, monkeypatch):
    import ctypes
    from convkan_amd import _lib as L
    from convkan_amd import ops
    lib = L.load()
    torch.manual_seed(5)
    layer = K.KANConv2DLayer(11, 128, 3, padding=1, base_activation=nn.SiLU).cuda()
    x, dz = (torch.randn(6, 11, 8, 8) * 1.5).cuda(), torch.randn(6, 128, 8, 8).cuda()

    # B = 5: no whole image pairs -- the entry is not offered and refuses, the op runs the plan's route
    geom, basis = _geom(layer, 5, 11, 128, 11, 128)
    assert not lib.kan_tile_orders(ctypes.byref(geom), ctypes.byref(basis)) & L.ORDER_POS8_BWD_WEIGHT
    assert lib.kan_bwd_weight_rowgroup_slabs(ctypes.byref(geom), ctypes.byref(basis)) == 0
    scratch = torch.zeros(16, device="cuda")
    assert lib.kan_conv_bwd_weight_rowgroups(ops._ptr(dz), ops._ptr(x), ops._ptr(scratch), ctypes.byref(geom), ctypes.byref(basis), ops._stream(x)) != 0
    assert b"kan_tile_orders" in lib.kan_last_error() and bool((scratch == 0).all())

    # the op itself: with the entry withheld it gives the plan's route bit for bit, with it the new slabs
    calls = []
    real = ops._pos8_bwd_weight
    spec = layer.conv_spec()
    for B in (5, 6):
        xb, zb = x[:B].contiguous(), dz[:B].contiguous()
        geom, basis = _geom(layer, B, 11, 128, 11, 128)
        _, _, _, ob, os_ = _run(layer, geom, basis, xb, zb, off=True)
        monkeypatch.setattr(ops, "_pos8_bwd_weight", lambda g, p: calls.append(real(g, p)) or calls[-1])
        _, _, db, ds = ops._conv_backward(spec, xb, None, (None, None), zb, False, False, True)
        assert calls[-1] == (B == 6)
        if B == 5:
            assert torch.equal(db[0], ob) and torch.equal(ds[0], os_)
        else:
            _, _, _, nb, ns = _run(layer, geom, basis, xb, zb)
            assert torch.equal(db[0], nb) and torch.equal(ds[0], ns)
            monkeypatch.setattr(ops, "_pos8_bwd_weight", lambda g, p: False)
            _, _, db, ds = ops._conv_backward(spec, xb, None, (None, None), zb, False, False, True)
            assert torch.equal(db[0], ob) and torch.equal(ds[0], os_)
