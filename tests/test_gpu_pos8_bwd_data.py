"""8x8 planes under 3x3 / stride 1 / pad 1 with the batch a multiple of 32: bwd-data orders a tile as 32 images x 4 adjacent columns of one plane row and
copies dz from its position-major copy (k_conv_bwd_data<.., RB = 3>; kan_tile_orders bit KAN_ORDER_POS8_BWD_DATA), so a 32-pixel MFMA block is one plane
position: the tap rows that leave the plane are skipped as whole steps, the tap columns as blocks -- 484 of 576 blocks issued.

Shapes (C -> O, B): 8 -> 16 (one channel tile whose second half holds one channel: an idle quarter), 14 -> 16 (both halves of one tile full), 20 -> 48 (two
channel tiles, the second ragged; three output blocks), 16 -> 32 at B = 64 inside tensors of 20 / 35 channels (padded batch strides), and 128 -> 128, whose plan
cuts the depth into six slabs (the 16-output shapes have one slab, 20 -> 48 three, 16 -> 32 two). Checked: the layer against the fp64 oracle (helpers.check_vs_oracle, TOL_DX); the launch with dz_pm against the same
launch without it (the plane-major tiles): torch.equal where the plan has one slab -- only exact zeros are dropped, the order of the sum stays -- and the
TOL_DX rule on the summed slabs where it has several (the slabs are cut over the live steps); guard words either side of the slabs and in the channels
the launch does not own; the one-slab bit equality for GELU as well (the kernel's second instantiation); a two-group launch (14 channels and 16 outputs per
group) against its groups launched alone, each on its own weights, dz_pm and channels of the same tensors, bit for bit; and a geometry out of scope, which must give the plane-major bits with dz_pm passed."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import convkan_amd as K
from helpers import TOL_DX, check_vs_oracle, relerr

pytestmark = pytest.mark.gpu

# (C, O, B, channels of the x tensor, channels of the dz tensor)
SHAPES = [(8, 16, 32, 8, 16), (14, 16, 32, 14, 16), (20, 48, 32, 20, 48), (16, 32, 64, 20, 35), (128, 128, 32, 128, 128)]
IDS = ["c8_o16_idle_quarter", "c14_o16_full_halves", "c20_o48_two_channel_tiles", "c16_o32_b64_padded_strides", "c128_o128_split_k"]
SENTINEL, PAD = 12345.0, 1 << 12


def _plan(layer, B, Cn, On, Ct, Ot, H=8):
    from convkan_amd import ops
    return ops._plan_cached(layer.conv_spec(), B, Cn, H, H, On, Ct, Ot)


def _run(layer, geom, basis, plan, x, dz, with_pm, grp=None):
    """One kan_conv_bwd_data launch into guarded slabs: returns the owned channels of the [S, B, Ct, H, W] slabs (channels the launch does not own keep
    the sentinel).  A grouped geometry owns the channels of all its groups.  `grp`: a single-group geometry launched as group `grp` of the grouped `layer`
    -- that group's weights packed alone, x, dz and dx at the group's channels of the wider tensors, dz_pm the position-major copy of its outputs."""
    from convkan_amd import _lib as L
    from convkan_amd import ops
    lib = L.load()
    st = ops._stream(x)
    basis = ops._with_table(basis, layer.conv_spec(), x.device)
    G = max(1, geom.groups)
    assert G == 1 or grp is None
    mods = slice(None) if grp is None else slice(grp, grp + 1)
    wb = torch.stack([m.weight.detach() for m in layer.base_conv[mods]]).contiguous()
    ws = torch.stack([m.weight.detach() for m in layer.spline_conv[mods]]).contiguous()
    assert tuple(wb.shape) == (G, geom.O, geom.C, 3, 3)
    wp = torch.empty(plan.packed_weight_bytes // 4, device=x.device)
    wd = torch.empty(plan.bwd_data_weight_bytes // 4, device=x.device)
    L.check(lib.kan_pack_weights(ops._ptr(wb), ops._ptr(ws), ops._ptr(wp), ops._ptr(wd), C.byref(geom), C.byref(basis), st), "kan_pack_weights")
    c0, own, o0 = (grp or 0) * geom.C, G * geom.C, (grp or 0) * geom.O      # first owned channel, owned channels, first output
    assert c0 + own <= x.shape[1] and o0 + G * geom.O <= dz.shape[1]
    dz_pm = ops._position_major(dz, o0, G * geom.O) if with_pm else None
    S, n = plan.bwd_data_splits, plan.bwd_data_slab_elems
    assert n == x.numel()
    big = torch.full((S * n + 2 * PAD,), SENTINEL, device=x.device)
    L.check(lib.kan_conv_bwd_data(ops._ptr(dz, o0 * 64), ops._ptr(x, c0 * 64), ops._ptr(x, c0 * 64), ops._ptr(wd), ops._ptr(big, PAD + c0 * 64), None,
                                  C.byref(geom), C.byref(basis), ops._ptr(dz_pm), st), "kan_conv_bwd_data")
    torch.cuda.synchronize()
    assert bool((big[:PAD] == SENTINEL).all()) and bool((big[PAD + S * n:] == SENTINEL).all()), with_pm
    slabs = big[PAD:PAD + S * n].view(S, *x.shape)
    assert bool((slabs[:, :, :c0] == SENTINEL).all()) and bool((slabs[:, :, c0 + own:] == SENTINEL).all()), with_pm      # the tensor's other channels (another group's; padding), between the images of every slab
    assert bool((slabs[:, :, c0:c0 + own] != SENTINEL).all()), with_pm      # every owned element of every slab is written
    return slabs[:, :, c0:c0 + own]


@pytest.mark.parametrize("Cn,On,B,Ct,Ot", SHAPES, ids=IDS)
def test_pos8_dx_equals_the_plane_major_tiles_and_writes_nothing_else(Cn, On, B, Ct, Ot, gpu_lib):
    from convkan_amd import _lib as L
    from convkan_amd import ops
    torch.manual_seed(Cn + On + B)
    layer = K.KANConv2DLayer(Cn, On, 3, padding=1, base_activation=nn.SiLU).cuda()
    geom, basis, plan = _plan(layer, B, Cn, On, Ct, Ot)
    assert plan.tile_orders & L.ORDER_POS8_BWD_DATA and ops._pos8_bwd_data(geom, plan) and not plan.dz_pm_wanted
    S = plan.bwd_data_splits
    assert (S == 1) == (On == 16)                    # the two 16-output shapes have one slab (bit-equality below); the others 3, 2 and 6
    x = (torch.randn(B, Ct, 8, 8) * 1.5).cuda()
    dz = torch.randn(B, Ot, 8, 8).cuda()
    new, old = _run(layer, geom, basis, plan, x, dz, True), _run(layer, geom, basis, plan, x, dz, False)
    err = relerr(new.sum(0), old.sum(0))
    print(f"[pos8 bwd-data C={Cn} O={On} B={B}] slabs {S}, dx vs the plane-major tiles: max-normalised difference {err:.3e}")
    assert bool(old.sum(0).abs().max() > 0)
    if S == 1:
        assert torch.equal(new, old)
    else:
        assert err <= TOL_DX


@pytest.mark.parametrize("Cn,On,B,Ct,Ot", SHAPES[:2], ids=IDS[:2])
def test_pos8_dx_gelu_equals_the_plane_major_tiles_bit_for_bit(Cn, On, B, Ct, Ot, gpu_lib):
    """The kernel's other instantiation (FAST_BSPLINE_GELU: the epilogue's base derivative is GELU's), on the two one-slab shapes."""
    from convkan_amd import _lib as L
    from convkan_amd import ops
    torch.manual_seed(Cn + On + B + 1)
    layer = K.KANConv2DLayer(Cn, On, 3, padding=1, base_activation=nn.GELU).cuda()
    geom, basis, plan = _plan(layer, B, Cn, On, Ct, Ot)
    assert plan.tile_orders & L.ORDER_POS8_BWD_DATA and ops._pos8_bwd_data(geom, plan) and plan.bwd_data_splits == 1
    x = (torch.randn(B, Ct, 8, 8) * 1.5).cuda()
    dz = torch.randn(B, Ot, 8, 8).cuda()
    new, old = _run(layer, geom, basis, plan, x, dz, True), _run(layer, geom, basis, plan, x, dz, False)
    assert bool(old.abs().max() > 0) and torch.equal(new, old)


def test_pos8_dx_of_a_grouped_launch_equals_its_groups_launched_alone(gpu_lib):
    """Two groups of 14 channels and 16 outputs at B = 32 in one launch -- the kernel's own group arithmetic: the group of a block, x and dx at
    grp * C * 64, the weights of the group, dz_pm at grp * O * HoWo * B -- against one single-group launch per group: that group's weights packed alone, its
    dz_pm = _position_major(dz, g * Og, Og), x, dz and dx at the group's channels of the same 28- / 32-channel tensors.  The same slab count gives the same
    sum order: bit equality; otherwise TOL_DX on the summed slabs.  Guard words, and after a single-group launch the other group's channels still hold the
    sentinel (_run).  The grouped launch with dz_pm against the same launch without it, as for one group."""
    from convkan_amd import _lib as L
    from convkan_amd import ops
    G, Cg, Og, B = 2, 14, 16, 32
    torch.manual_seed(G + Cg + Og + B)
    grouped = K.KANConv2DLayer(G * Cg, G * Og, 3, padding=1, groups=G, base_activation=nn.SiLU).cuda()
    alone = K.KANConv2DLayer(Cg, Og, 3, padding=1, base_activation=nn.SiLU)
    gg, bg, pg = _plan(grouped, B, Cg, Og, G * Cg, G * Og)
    g1, b1, p1 = _plan(alone, B, Cg, Og, G * Cg, G * Og)
    assert gg.groups == G and max(1, g1.groups) == 1
    for plan, geom in ((pg, gg), (p1, g1)):
        assert plan.tile_orders & L.ORDER_POS8_BWD_DATA and ops._pos8_bwd_data(geom, plan) and not plan.dz_pm_wanted
    x = (torch.randn(B, G * Cg, 8, 8) * 1.5).cuda()
    dz = torch.randn(B, G * Og, 8, 8).cuda()
    new, old = _run(grouped, gg, bg, pg, x, dz, True), _run(grouped, gg, bg, pg, x, dz, False)
    assert tuple(new.shape) == (pg.bwd_data_splits, B, G * Cg, 8, 8) and bool(old.sum(0).abs().max() > 0)
    if pg.bwd_data_splits == 1:
        assert torch.equal(new, old)
    else:
        assert relerr(new.sum(0), old.sum(0)) <= TOL_DX
    for g in range(G):
        part = _run(grouped, g1, b1, p1, x, dz, True, grp=g)
        mine = new[:, :, g * Cg:(g + 1) * Cg]
        err = relerr(mine.sum(0), part.sum(0))
        print(f"[pos8 bwd-data G=2] group {g}: slabs {pg.bwd_data_splits} grouped, {p1.bwd_data_splits} alone; max-normalised difference {err:.3e}")
        assert bool(part.sum(0).abs().max() > 0)
        if pg.bwd_data_splits == p1.bwd_data_splits:
            assert torch.equal(mine, part), g
        else:
            assert err <= TOL_DX, g


@pytest.mark.parametrize("Cn,On,B", [(s[0], s[1], s[2]) for s in SHAPES], ids=IDS)
def test_pos8_layer_vs_oracle(Cn, On, B, gpu_lib):
    """(the padded-stride shape runs here in dense tensors: a layer owns its whole input)"""
    from convkan_amd import _lib as L
    torch.manual_seed(On + B)
    layer = K.KANConv2DLayer(Cn, On, 3, padding=1, base_activation=nn.SiLU)
    _, _, plan = _plan(layer, B, Cn, On, Cn, On)
    assert plan.tile_orders & L.ORDER_POS8_BWD_DATA
    errs = check_vs_oracle(layer, dict(kind="bspline", C=Cn, O=On, k=3, s=1, p=1, d=1, groups=1, act="silu"), torch.randn(B, Cn, 8, 8) * 1.5)
    print(f"[pos8 layer C={Cn} O={On} B={B}] dx (error, tolerance, fp32 oracle's own) {errs['dx']}")


def test_geometry_out_of_scope_keeps_the_plane_major_bits_with_dz_pm_passed(gpu_lib):
    """B = 48 has no whole 32-image groups: the launch ignores dz_pm."""
    from convkan_amd import _lib as L
    torch.manual_seed(48)
    layer = K.KANConv2DLayer(16, 32, 3, padding=1, base_activation=nn.SiLU).cuda()
    geom, basis, plan = _plan(layer, 48, 16, 32, 16, 32)
    assert not plan.tile_orders & L.ORDER_POS8_BWD_DATA
    x = (torch.randn(48, 16, 8, 8) * 1.5).cuda()
    dz = torch.randn(48, 32, 8, 8).cuda()
    assert torch.equal(_run(layer, geom, basis, plan, x, dz, True), _run(layer, geom, basis, plan, x, dz, False))


def test_kan_vgg11_bs32_step_with_and_without_the_route(gpu_lib, monkeypatch):
    """One KAN-VGG11 training step at batch 32 (both 8x8 layers take the route) against the same step with the route's dz_pm withheld, which is the
    parent's launch sequence: the forward is untouched, so logits and loss are bit-equal; the gradients meet the tolerances of the model tests
    (TOL_DW on weights, 2e-5 on the PReLU slopes judged together), and those downstream of the 8x8 layers are bit-equal."""
    import torch.nn.functional as F
    from convkan_amd import ops
    from convkan_amd.models import vggkan
    from helpers import TOL_DW
    torch.manual_seed(0)
    model = vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear").cuda().train()
    x = torch.randn(32, 3, 32, 32, device="cuda")
    t = torch.arange(32, device="cuda") % 10

    def step():
        torch.manual_seed(7)                                                 # the model's dropout masks: the same in both steps
        model.zero_grad(set_to_none=True)
        logits = model(x)
        loss = F.cross_entropy(logits, t)
        loss.backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}

    calls = []
    real = ops._pos8_bwd_data
    monkeypatch.setattr(ops, "_pos8_bwd_data", lambda geom, plan: calls.append(real(geom, plan)) or calls[-1])
    la, lossa, ga = step()
    assert sum(calls) >= 2                                                   # the two 8x8 layers asked for the route
    monkeypatch.setattr(ops, "_pos8_bwd_data", lambda geom, plan: False)
    lb, lossb, gb = step()
    assert torch.equal(la, lb) and torch.equal(lossa, lossb)
    slopes_a, slopes_b, moved = [], [], []
    for n in ga:
        if ga[n].numel() == 1:
            slopes_a.append(ga[n].reshape(-1)); slopes_b.append(gb[n].reshape(-1))
            continue
        if not torch.equal(ga[n], gb[n]):
            moved.append(n)
        assert relerr(ga[n], gb[n]) <= TOL_DW, n
    assert relerr(torch.cat(slopes_a), torch.cat(slopes_b)) <= 2e-5
    print(f"[pos8 KAN-VGG11 bs 32] weight gradients that moved: {moved}")
    assert all(int(n.split(".")[1]) < 5 for n in moved), moved              # only upstream of the 8x8 layers (features.5 and .7)
