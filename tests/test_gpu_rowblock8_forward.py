"""8x8 planes with 256-output tiles and the batch a multiple of 4: the halo forward orders a tile as 4 images x half a plane in row blocks, so the
32-pixel MFMA block of the plane's first (last) row is skipped under tap row 0 (2): 11 of 12 blocks issued.  `KanPlan.row_blocks` stays 0 for these
geometries; `ops._row_blocks8_forward` states the route.  y, dx and dW against the fp64 oracle through the helpers and tolerances of the 4x4
row-block and quadrant tests; inputs are scaled by 1.5 so that border values are not small."""
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
    """(row_blocks bits, forward on half-plane row blocks)"""
    from convkan_amd import ops
    geom, _, plan = ops._plan_cached(layer.conv_spec(), B, C // G, 8, 8, O // G, C, O)
    assert plan.fwd_halo
    return plan.row_blocks, ops._row_blocks8_forward(geom, plan)


@pytest.mark.parametrize("C,O,B,G,want", [(4, 256, 4, 1, (0, True)), (6, 256, 8, 1, (0, True)), (4, 512, 8, 2, (0, True)), (4, 256, 6, 1, (0, False))],
                         ids=["o256_b4", "o256_b8_three_pairs", "o512_b8_groups2", "o256_b6_whole_planes"])
def test_row_block_forward_on_8x8_planes_vs_oracle(C, O, B, G, want, gpu_lib):
    """One image group (a top-half and a bottom-half tile); two groups and three channel pairs; two convolution groups; and B = 6, which has no whole
    4-image groups and stays on the whole-plane tile of 2 images."""
    torch.manual_seed(O + B)
    layer = K.KANConv2DLayer(C, O, 3, padding=1, groups=G, base_activation=nn.SiLU)
    assert _route(layer, B, C, O, G) == want
    check_vs_oracle(layer, _cfg("bspline", C, O, groups=G, act="silu"), torch.randn(B, C, 8, 8) * 1.5, groups=G)


def test_row_block_forward_is_image_for_image_independent_of_the_batch_order(gpu_lib):
    """A tile mixes 4 images and half planes: the forward of the reversed batch must be the reversed forward, bit for bit."""
    torch.manual_seed(88)
    layer = K.KANConv2DLayer(6, 256, 3, padding=1, base_activation=nn.SiLU).cuda()
    assert _route(layer, 8, 6, 256)[1]
    x = (torch.randn(8, 6, 8, 8) * 1.5).cuda()
    with torch.no_grad():
        y, yr = layer(x), layer(x.flip(0).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(yr, y.flip(0))


def test_row_block_forward_equals_the_whole_plane_tile_bit_for_bit(gpu_lib):
    """Only exact zeros are skipped and the order of the sum per output is unchanged, so the z slabs equal those of the whole-plane tile of 2 images.
    That tile is reached with the same inputs by a batch of 6 (no whole 4-image groups): its first four images against a batch-of-4 call.  The planner
    gives both the same fwd_splits (asserted), so the slabs themselves are compared, before any reduction."""
    from convkan_amd import ops
    torch.manual_seed(46)
    layer = K.KANConv2DLayer(4, 256, 3, padding=1, base_activation=nn.SiLU).cuda()
    assert _route(layer, 4, 4, 256) == (0, True) and _route(layer, 6, 4, 256) == (0, False)
    x6 = (torch.randn(6, 4, 8, 8) * 1.5).cuda()
    wb, ws = [layer.base_conv[0].weight.detach()], [layer.spline_conv[0].weight.detach()]
    with torch.no_grad():
        z6, _, _, _, plan6 = ops._conv_forward(layer.conv_spec(), x6, None, wb, ws, need_dgrad=False)
        z4, _, _, _, plan4 = ops._conv_forward(layer.conv_spec(), x6[:4].contiguous(), None, wb, ws, need_dgrad=False)
    torch.cuda.synchronize()
    assert plan4.fwd_splits == plan6.fwd_splits and z4.shape[0] == z6.shape[0]
    assert torch.equal(z4, z6[:, :4])
