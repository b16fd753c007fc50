"""kan_unpack_wgrad sums the weight-gradient slabs per element in ONE documented order -- eight running sums take slabs s, s + 8, ... of
each whole group of eight, the remaining slabs go into the first sum one after the other, then ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)) -- and
scatters the sums to the reference layouts.  Checked bit for bit on real slabs of kan_conv_bwd_weight, per row order pack_row serves:

    tap-major           grid 3 / order 2 B-spline (generic kernels), 3 -> 40 @ 8x8   (the default spec's 3 -> 40 @ 8x8 takes the band kernels)
    halo channel-major  default spec, 16 -> 128 @ 8x8
    band                default spec, 3 -> 40 @ 8x8

at slab counts 1, 2, 3, 9 (one group of eight + a remainder) and, for the band order, 19 (two groups + three).  The batch sets the
count; the test checks it, and the route, from the plan.  The reference unpacks every slab ALONE (the same geometry at batch 1 plans one
slab: a pure permutation of the slab at a pointer offset) and combines the results in torch in the documented order, in fp32.
J = C * T (27, 144) and C * n_basis * T are no multiples of the 32-column tile, and 40 outputs leave 24 padding columns of Opad = 64.
Guard words either side of both gradients show that nothing else is written."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import convkan_amd as K
import route_cells as R

pytestmark = pytest.mark.gpu

LAYERS = {
    "tap": (dict(grid_size=3, spline_order=2, base_activation=nn.SiLU), 3, 40, "TAP"),
    "halo_cmajor": (dict(base_activation=nn.SiLU), 16, 128, "HALO"),
    "band": (dict(base_activation=nn.SiLU), 3, 40, "BAND"),
}
# (layer, batch, slabs the plan must give)
CASES = [("tap", 1, 1), ("tap", 8, 2), ("tap", 12, 3), ("tap", 36, 9),
         ("halo_cmajor", 1, 1), ("halo_cmajor", 2, 2), ("halo_cmajor", 3, 3), ("halo_cmajor", 9, 9),
         ("band", 1, 1), ("band", 2, 2), ("band", 3, 3), ("band", 9, 9), ("band", 19, 19)]
SENTINEL, PAD = 12345.0, 1 << 10


def combine(parts):
    """The documented summation order over a list of per-slab tensors."""
    zero = torch.zeros_like(parts[0])
    s = [zero.clone() for _ in range(8)]
    n, sl = len(parts), 0
    while sl + 8 <= n:
        for i in range(8):
            s[i] = s[i] + parts[sl + i]
        sl += 8
    for i in range(sl, n):
        s[0] = s[0] + parts[i]
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))


def _guarded(shape, device):
    n = 1
    for d in shape:
        n *= d
    big = torch.full((n + 2 * PAD,), SENTINEL, device=device)
    return big, big[PAD:PAD + n].view(shape)


def _check_guards(big):
    assert bool((big[:PAD] == SENTINEL).all()) and bool((big[-PAD:] == SENTINEL).all())
    assert bool((big[PAD:-PAD] != SENTINEL).all())


@pytest.mark.parametrize("name,B,slabs", CASES, ids=[f"{n}-b{b}-s{s}" for n, b, s in CASES])
def test_unpack_sums_slabs_in_the_documented_order(name, B, slabs, gpu_lib):
    from convkan_amd import _lib as L
    from convkan_amd import ops
    lib = L.load()
    kw, Cn, On, route = LAYERS[name]
    torch.manual_seed(B + On)
    layer = K.KANConv2DLayer(Cn, On, 3, padding=1, **kw).cuda()
    spec = layer.conv_spec()
    geom, basis, plan = ops._plan_cached(spec, B, Cn, 8, 8, On, Cn, On)
    geom1, basis1, plan1 = ops._plan_cached(spec, 1, Cn, 8, 8, On, Cn, On)          # one slab: unpacks a slab alone
    assert R.route_key(geom, basis, plan)[3] == route and R.route_key(geom1, basis1, plan1)[3] == route
    assert plan.bwd_weight_splits == slabs and plan1.bwd_weight_splits == 1
    assert (plan1.K, plan1.Kpad, plan1.Opad, plan1.bwd_weight_slab_elems) == (plan.K, plan.Kpad, plan.Opad, plan.bwd_weight_slab_elems)
    assert not plan.x_pm_wanted and not plan.dz_pm_wanted
    x = (torch.randn(B, Cn, 8, 8) * 1.5).cuda()
    dz = torch.randn(B, On, 8, 8, device="cuda")
    st = ops._stream(x)
    basis, basis1 = ops._with_table(basis, spec, x.device), ops._with_table(basis1, spec, x.device)
    n = plan.bwd_weight_slab_elems
    dwp = torch.zeros(slabs * n, device="cuda")
    L.check(lib.kan_conv_bwd_weight(ops._ptr(dz), ops._ptr(x), ops._ptr(x), ops._ptr(dwp), C.byref(geom), C.byref(basis), None, None, st),
            "kan_conv_bwd_weight")
    shapes = ((1, On, Cn, 3, 3), (1, On, Cn * spec.n_basis, 3, 3))
    (big_b, dwb), (big_s, dws) = (_guarded(s, x.device) for s in shapes)
    L.check(lib.kan_unpack_wgrad(ops._ptr(dwp), ops._ptr(dwb), ops._ptr(dws), C.byref(geom), C.byref(basis), st), "kan_unpack_wgrad")
    torch.cuda.synchronize()
    _check_guards(big_b)
    _check_guards(big_s)
    alone_b, alone_s = [], []
    for i in range(slabs):
        ub, us = (torch.empty(s, device=x.device) for s in shapes)
        L.check(lib.kan_unpack_wgrad(ops._ptr(dwp, i * n), ops._ptr(ub), ops._ptr(us), C.byref(geom1), C.byref(basis1), st), "kan_unpack_wgrad")
        alone_b.append(ub)
        alone_s.append(us)
    torch.cuda.synchronize()
    assert all(bool(u.abs().max() > 0) for u in alone_s)                   # every slab carries part of the sum
    assert torch.equal(dwb, combine(alone_b))
    assert torch.equal(dws, combine(alone_s))
