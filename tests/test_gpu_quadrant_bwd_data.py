"""4x4 planes with the batch a multiple of 32 and a weight gradient on the expanded-operand route (C a multiple of 128: the position-major copy of dz
exists): bwd-data orders a tile as 32 images x one 2x2 quadrant of the input plane and copies dz from dz_pm, so a 32-pixel MFMA block is one plane
position and is skipped under exactly the taps it has no source for (25 of 36 blocks issued; the row-block order issues 30).  `KanPlan.row_blocks`
keeps its bit 1 and `ops._quadrant_order(.., "bwd_data")` stays False; `ops._quadrant_bwd_data` states the route.  y, dx and dW against the fp64
oracle through the helpers and tolerances of the 4x4 row-block and quadrant tests; inputs are scaled by 1.5 so that border values are not small."""
import pytest
import torch
import torch.nn as nn

import convkan_amd as K
from helpers import check_vs_oracle

pytestmark = pytest.mark.gpu


def _cfg(kind, C, O, groups=1, **kw):
    c = dict(kind=kind, C=C, O=O, k=3, s=1, p=1, d=1, groups=groups)
    c.update(kw)
    return c


def _route(layer, B, C, O, G=1):
    """(dz_pm wanted, row_blocks bit of bwd-data, bwd-data on quadrant tiles when dz_pm is passed / when it is not)"""
    from convkan_amd import ops
    geom, _, plan = ops._plan_cached(layer.conv_spec(), B, C // G, 4, 4, O // G, C, O)
    assert not ops._quadrant_order(geom, plan, "bwd_data")
    return bool(plan.dz_pm_wanted), bool(plan.row_blocks & 2), ops._quadrant_bwd_data(geom, plan, True), ops._quadrant_bwd_data(geom, plan, False)


@pytest.mark.parametrize("C,O,B,G,act,quad", [(128, 128, 32, 1, "silu", True), (128, 256, 64, 1, "gelu", True), (256, 256, 32, 2, "silu", True),
                                                (128, 128, 40, 1, "silu", False)],
                         ids=["c128_o128_b32", "c128_o256_b64_gelu", "c256_o256_b32_groups2", "c128_o128_b40_row_blocks"])
def test_quadrant_bwd_data_on_4x4_planes_vs_oracle(C, O, B, G, act, quad, gpu_lib):
    """One image group, 10 channel tiles of which the last has an idle half; two image groups and GELU; two convolution groups; and B = 40, which has
    no whole 32-image groups and stays on the row-block kernel."""
    torch.manual_seed(C + O + B)
    layer = K.KANConv2DLayer(C, O, 3, padding=1, groups=G, base_activation=nn.SiLU if act == "silu" else nn.GELU)
    assert _route(layer, B, C, O, G) == (quad, True, quad, False)          # (B = 40: no expanded weight gradient either, so no dz_pm)
    check_vs_oracle(layer, _cfg("bspline", C, O, groups=G, act=act), torch.randn(B, C, 4, 4) * 1.5, groups=G)


def test_quadrant_bwd_data_is_image_for_image_independent_of_the_batch_order(gpu_lib):
    """A tile mixes 32 images: dx of the reversed batch (x and the upstream gradient both reversed) must be the reversed dx, bit for bit."""
    torch.manual_seed(128)
    layer = K.KANConv2DLayer(128, 128, 3, padding=1, base_activation=nn.SiLU).cuda()
    assert _route(layer, 32, 128, 128)[2]
    x = (torch.randn(32, 128, 4, 4) * 1.5).cuda()
    go = torch.randn(32, 128, 4, 4).cuda()

    def dx_of(xi, gi):
        xi = xi.clone().requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        layer(xi).backward(gi)
        return xi.grad

    dx, dxr = dx_of(x, go), dx_of(x.flip(0).contiguous(), go.flip(0).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(dxr, dx.flip(0))
