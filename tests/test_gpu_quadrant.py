"""4x4 planes with the batch a multiple of 32: the halo forward orders a tile as 32 images x one 2x2 quadrant of the plane, so a 32-pixel
MFMA block is one plane position and is skipped under exactly the taps that leave the plane (25 of 36 blocks issued; the row-block order
issues 30).  bwd-data keeps its row blocks (the quadrant variant was measured and not shipped: DESIGN.md section 3).  y, dx and dW against the
fp64 oracle through the helpers and tolerances of test_gpu_oracle's row-block test; inputs are scaled by 1.5 so that border values are not small."""
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


def _plan(layer, B, C, O, G=1):
    from convkan_amd import ops
    return ops._plan_cached(layer.conv_spec(), B, C // G, 4, 4, O // G, C, O)


def _orders(layer, B, C, O, G=1):
    """(row_blocks bits, forward on the quadrant order)"""
    from convkan_amd import ops
    geom, _, plan = _plan(layer, B, C, O, G)
    assert not ops._quadrant_order(geom, plan, "bwd_data")
    return plan.row_blocks, ops._quadrant_order(geom, plan, "fwd")


@pytest.mark.parametrize("C,O,B,G,act,want", [(6, 256, 32, 1, "silu", (3, True)), (4, 512, 64, 1, "gelu", (3, True)),
                                                (6, 256, 96, 1, "silu", (3, True)), (8, 512, 32, 2, "silu", (3, True)),
                                                (6, 256, 40, 1, "silu", (3, False))],
                         ids=["o256_b32", "o512_b64_gelu", "o256_b96_three_groups", "o512_b32_groups2", "o256_b40_row_blocks"])
def test_quadrant_forward_on_4x4_planes_vs_oracle(C, O, B, G, act, want, gpu_lib):
    """One tile per quadrant and three channel pairs; two image groups and two output tiles; three image groups; two convolution groups;
    and B = 40, which has no whole 32-image groups and stays on the row-block kernel."""
    torch.manual_seed(O + B)
    layer = K.KANConv2DLayer(C, O, 3, padding=1, groups=G, base_activation=nn.SiLU if act == "silu" else nn.GELU)
    assert _orders(layer, B, C, O, G) == want          # row_blocks bit 0: forward, bit 1: bwd-data
    check_vs_oracle(layer, _cfg("bspline", C, O, groups=G, act=act), torch.randn(B, C, 4, 4) * 1.5, groups=G)


def test_quadrant_forward_for_the_recurrence_spec_vs_oracle(gpu_lib):
    """The degree-3 recurrence spec (P = 5 planes) on the quadrant forward; its bwd-data stays plain."""
    torch.manual_seed(11)
    layer = K.LucasKANConv2DLayer(6, 256, 3, degree=3, padding=1, base_activation=nn.SiLU)
    assert _orders(layer, 32, 6, 256) == (1, True)
    check_vs_oracle(layer, _cfg("lucas", 6, 256, act="silu", degree=3), torch.randn(32, 6, 4, 4) * 1.5)


def test_quadrant_forward_is_image_for_image_independent_of_the_batch_order(gpu_lib):
    """A tile mixes 32 images: the forward of the reversed batch must be the reversed forward, bit for bit (an image / position mix-up
    between neighbouring images could hide under the oracle tolerance)."""
    torch.manual_seed(288)
    layer = K.KANConv2DLayer(6, 256, 3, padding=1, base_activation=nn.SiLU).cuda()
    assert _orders(layer, 32, 6, 256)[1]
    x = (torch.randn(32, 6, 4, 4) * 1.5).cuda()
    with torch.no_grad():
        y, yr = layer(x), layer(x.flip(0).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(yr, y.flip(0))
