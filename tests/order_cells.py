"""Tile-order cells of the conv-KAN launchers: the pixel orders inside a tile that the public KanPlan does not show.

route_cells.route_key is built from KanPlan alone, so the six orders that kan_tile_orders reports (KAN_ORDER_* of include/kanconv.h, ORDER_* of
_lib.py) fall into the route cell of the launch they replace: the route matrix cannot tell a launch on such an order from one off it.  This
table gives them cells of their own:

    order_key(g, b, p) = (spec class, sorted names of the kan_tile_orders bits, grouped?, fwd route, bwd-data route, bwd-weight route)

Only keys with at least one bit are cells here (a launch with no bit is exactly its route cell: tests/route_cells.py).  ORDER_CASES holds one row
per reachable key -- the smallest geometry that reaches it, by oracle work B * H * W * C * O / G, over C in {1, 2, 3, 4, 8, 16, .. 256} and O in
{1, 2, 16, 32, .. 512} per group (tests/test_order_matrix.py holds every first row of a cell to that minimum) -- plus rows that run the stage of every
(spec class, bit) with one slab and with several where the planner makes both: fwd_splits for the three forward orders, bwd_data_splits for the two
bwd-data orders, kan_bwd_weight_rowgroup_slabs for the 8x8 weight gradient.  tests/test_gpu_order_matrix.py runs every row against the fp64 oracle."""
import ctypes

from convkan_amd import _lib as L
from route_cells import key_id, route_key, row, second_input, spec_class

# kan_tile_orders bit -> (name, stage whose launch it reorders)
BITS = {L.ORDER_QUAD_FWD: ("QUAD_FWD", "fwd"), L.ORDER_ROWBLK8_FWD: ("ROWBLK8_FWD", "fwd"), L.ORDER_FWD_WEIGHT_SIDE: ("FWD_WEIGHT_SIDE", "fwd"),
        L.ORDER_QUAD_BWD_DATA: ("QUAD_BWD_DATA", "bd"), L.ORDER_POS8_BWD_DATA: ("POS8_BWD_DATA", "bd"), L.ORDER_POS8_BWD_WEIGHT: ("POS8_BWD_WEIGHT", "bw")}
STAGE_OF = dict(BITS.values())
# images of one tile of the order: a permutation of the batch that crosses these groups moves an image to another tile and another slot
GROUP_OF = {"QUAD_FWD": 32, "QUAD_BWD_DATA": 32, "POS8_BWD_DATA": 32, "ROWBLK8_FWD": 4, "FWD_WEIGHT_SIDE": 128}


def order_names(g, b):
    """Sorted tuple of the names of the kan_tile_orders bits of a launch (host arithmetic)."""
    mask = L.load().kan_tile_orders(ctypes.byref(g), ctypes.byref(b))
    assert not mask & ~sum(BITS), f"kan_tile_orders reports a bit this table does not know: {mask:#x}"
    return tuple(sorted(name for bit, (name, _) in BITS.items() if mask & bit))


def order_key(g, b, p):
    return (spec_class(b), order_names(g, b), g.groups > 1) + route_key(g, b, p)[1:]


def order_splits(g, b, p):
    """{bit name: slabs of the launch it reorders} of a launch."""
    slabs = {"fwd": p.fwd_splits, "bd": p.bwd_data_splits, "bw": L.load().kan_bwd_weight_rowgroup_slabs(ctypes.byref(g), ctypes.byref(b))}
    return {name: slabs[STAGE_OF[name]] for name in order_names(g, b)}


def ops_takes_pos8_bw(names, b, w_iod=False):
    """Whether ops._conv_backward runs kan_conv_bwd_weight_rowgroups: `xn is None and spec.w_layout != W_IOD and _pos8_bwd_weight(geom, plan)` (ops.py:839)."""
    return not second_input(b) and not w_iod and "POS8_BWD_WEIGHT" in names


def work(c):
    """What a row costs the CPU oracle, up to a constant: B * H * W * C * O / G."""
    return c["B"] * c["H"] * c["W"] * c["C"] * c["O"] // c["G"]


def order_id(key):
    return "-".join([key[0], "+".join(key[1]), "G2" if key[2] else "G1", key_id(key[3:])])


def case_ids(cases):
    seen, out = {}, []
    for c in cases:
        i = order_id(c["key"])
        n = seen[i] = seen.get(i, 0) + 1
        out.append(i if n == 1 else f"{i}-{n}")
    return out


def orow(spec, orders, routes, layer, B, C, O, H, G=1, **opts):
    """One ORDER_CASES row: route_cells.row() on the 3x3 / stride 1 / pad 1 shape every tile order is made for, keyed by the order key."""
    c = row(f"{spec} {routes}", layer, "3x3", B, C, O, H, G=G, **opts)
    c["key"] = (spec, tuple(sorted(orders.split("+"))), G > 1) + tuple(routes.split())
    return c


def perm_batch(case):
    """Batch of the image-permutation check of a row: the first of 64, the row's own batch and twice that which holds more than one tile of every
    forward / bwd-data order of the row and is still the row's cell (B = 64: two 32-image groups; two 4-image groups from B = 4, two 128-image tiles from
    B = 128); the row's own batch where none is (eight cells exist at B = 32 only: the permutation then moves the images inside the one group)."""
    from route_cells import case_layer, case_structs
    layer = case_layer(case)
    need = max(GROUP_OF[n] for n in case["key"][1] if n in GROUP_OF)
    for B in (64, case["B"], 2 * case["B"]):
        if B > need:
            g, b, p = case_structs(dict(case, B=B), layer)
            if order_key(g, b, p) == case["key"]:
                return B
    return case["B"]


# cells knowingly left without a row: {key: "measured time of the smallest geometry; the GPU test that covers it instead"}.  At most two.
EXEMPT = {}

# Rows of the B-spline and ReLU-KAN specs alternate inputs scaled 3x past their grid range, every third row has a perturbed affine InstanceNorm, the four
# recurrence families of FAST_POLY4 take turns (as in route_cells.ROUTE_CASES).
ORDER_CASES = [
    # FAST_BSPLINE_GELU
    orow('FAST_BSPLINE_GELU', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM EXPANDED', 'kan_gelu', 128, 128, 80, 2),
    orow('FAST_BSPLINE_GELU', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM TAP-PM', 'kan_gelu', 128, 2, 80, 2, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM EXPANDED', 'kan_gelu', 128, 256, 160, 2, G=2, affine=True),
    orow('FAST_BSPLINE_GELU', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM TAP-PM', 'kan_gelu', 128, 4, 160, 2, G=2, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA', 'BAND TAP BAND', 'kan_gelu', 32, 1, 16, 8),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA', 'BAND TAP HALO', 'kan_gelu', 32, 64, 96, 8, scale=3.0, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA', 'BAND TAP TAP', 'kan_gelu', 32, 32, 192, 8),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA', 'HALO TAP HALO', 'kan_gelu', 32, 2, 128, 8, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA', 'BAND TAP BAND', 'kan_gelu', 32, 2, 32, 8, G=2, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA', 'BAND TAP HALO', 'kan_gelu', 32, 64, 192, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA', 'BAND TAP TAP', 'kan_gelu', 32, 32, 384, 8, G=2),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA', 'HALO TAP HALO', 'kan_gelu', 32, 4, 256, 8, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP BAND', 'kan_gelu', 32, 112, 16, 8),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP HALO', 'kan_gelu', 256, 4, 208, 8, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP TAP', 'kan_gelu', 32, 128, 48, 8, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'HALO TAP HALO', 'kan_gelu', 128, 8, 384, 8, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP BAND', 'kan_gelu', 256, 8, 32, 8, G=2),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP HALO', 'kan_gelu', 256, 2, 768, 8, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP TAP', 'kan_gelu', 32, 128, 96, 8, G=2),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'HALO TAP HALO', 'kan_gelu', 256, 8, 256, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_gelu', 128, 4, 512, 8, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_gelu', 64, 8, 1024, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_gelu', 32, 2, 256, 8),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_DATA+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_gelu', 32, 4, 512, 8, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT', 'BAND TAP BAND', 'kan_gelu', 2, 2, 1, 8),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT', 'BAND TAP HALO', 'kan_gelu', 2, 208, 464, 8, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT', 'BAND TAP TAP', 'kan_gelu', 2, 232, 416, 8, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT', 'HALO TAP HALO', 'kan_gelu', 2, 2, 128, 8, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT', 'BAND TAP BAND', 'kan_gelu', 2, 4, 2, 8, G=2),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT', 'BAND TAP HALO', 'kan_gelu', 2, 208, 928, 8, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT', 'BAND TAP TAP', 'kan_gelu', 2, 224, 864, 8, G=2),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT', 'HALO TAP HALO', 'kan_gelu', 2, 4, 256, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_gelu', 4, 2, 256, 8, affine=True),
    orow('FAST_BSPLINE_GELU', 'POS8_BWD_WEIGHT+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_gelu', 4, 4, 512, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'BAND TAP-RB EXPANDED', 'kan_gelu', 32, 128, 80, 4),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'BAND TAP-RB HALO', 'kan_gelu', 32, 1, 80, 4, scale=3.0, affine=True),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'BAND TAP-RB TAP-PM', 'kan_gelu', 32, 1, 16, 4),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'HALO TAP-RB EXPANDED', 'kan_gelu', 32, 128, 128, 4, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'HALO TAP-RB HALO', 'kan_gelu', 32, 2, 128, 4, affine=True),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'BAND TAP-RB EXPANDED', 'kan_gelu', 32, 256, 160, 4, G=2, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'BAND TAP-RB HALO', 'kan_gelu', 32, 2, 160, 4, G=2),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'BAND TAP-RB TAP-PM', 'kan_gelu', 32, 2, 32, 4, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'HALO TAP-RB EXPANDED', 'kan_gelu', 32, 256, 256, 4, G=2),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA', 'HALO TAP-RB HALO', 'kan_gelu', 32, 4, 256, 4, G=2, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA+QUAD_FWD', 'HALO+RB TAP-RB EXPANDED', 'kan_gelu', 32, 128, 256, 4, affine=True),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA+QUAD_FWD', 'HALO+RB TAP-RB HALO', 'kan_gelu', 32, 2, 256, 4, scale=3.0),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA+QUAD_FWD', 'HALO+RB TAP-RB EXPANDED', 'kan_gelu', 32, 256, 512, 4, G=2),
    orow('FAST_BSPLINE_GELU', 'QUAD_BWD_DATA+QUAD_FWD', 'HALO+RB TAP-RB HALO', 'kan_gelu', 32, 4, 512, 4, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_GELU', 'ROWBLK8_FWD', 'HALO TAP HALO', 'kan_gelu', 40, 2, 256, 8),
    orow('FAST_BSPLINE_GELU', 'ROWBLK8_FWD', 'HALO TAP HALO', 'kan_gelu', 40, 4, 512, 8, G=2, scale=3.0),
    # FAST_BSPLINE_SILU
    orow('FAST_BSPLINE_SILU', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM EXPANDED', 'kan_silu', 128, 128, 80, 2, affine=True),
    orow('FAST_BSPLINE_SILU', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM TAP-PM', 'kan_silu', 128, 2, 80, 2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM EXPANDED', 'kan_silu', 128, 256, 160, 2, G=2),
    orow('FAST_BSPLINE_SILU', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM TAP-PM', 'kan_silu', 128, 4, 160, 2, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA', 'BAND TAP BAND', 'kan_silu', 32, 1, 16, 8),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA', 'BAND TAP HALO', 'kan_silu', 32, 64, 96, 8, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA', 'BAND TAP TAP', 'kan_silu', 32, 32, 192, 8, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA', 'HALO TAP HALO', 'kan_silu', 32, 2, 128, 8, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA', 'BAND TAP BAND', 'kan_silu', 32, 2, 32, 8, G=2),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA', 'BAND TAP HALO', 'kan_silu', 32, 64, 192, 8, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA', 'BAND TAP TAP', 'kan_silu', 32, 32, 384, 8, G=2),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA', 'HALO TAP HALO', 'kan_silu', 32, 4, 256, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP BAND', 'kan_silu', 32, 112, 16, 8, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP HALO', 'kan_silu', 256, 4, 208, 8, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP TAP', 'kan_silu', 32, 128, 48, 8),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'HALO TAP HALO', 'kan_silu', 128, 8, 384, 8, scale=3.0, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP BAND', 'kan_silu', 256, 8, 32, 8, G=2),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP HALO', 'kan_silu', 256, 2, 768, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'BAND TAP TAP', 'kan_silu', 32, 128, 96, 8, G=2, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT', 'HALO TAP HALO', 'kan_silu', 256, 8, 256, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_silu', 128, 4, 512, 8),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+POS8_BWD_WEIGHT+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_silu', 64, 8, 1024, 8, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_silu', 32, 2, 256, 8),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_DATA+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_silu', 32, 4, 512, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT', 'BAND TAP BAND', 'kan_silu', 2, 2, 1, 8, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT', 'BAND TAP HALO', 'kan_silu', 2, 208, 464, 8, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT', 'BAND TAP TAP', 'kan_silu', 2, 232, 416, 8),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT', 'HALO TAP HALO', 'kan_silu', 2, 2, 128, 8, scale=3.0, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT', 'BAND TAP BAND', 'kan_silu', 2, 4, 2, 8, G=2),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT', 'BAND TAP HALO', 'kan_silu', 2, 208, 928, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT', 'BAND TAP TAP', 'kan_silu', 2, 224, 864, 8, G=2, affine=True),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT', 'HALO TAP HALO', 'kan_silu', 2, 4, 256, 8, G=2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_silu', 4, 2, 256, 8),
    orow('FAST_BSPLINE_SILU', 'POS8_BWD_WEIGHT+ROWBLK8_FWD', 'HALO TAP HALO', 'kan_silu', 4, 4, 512, 8, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'BAND TAP-RB EXPANDED', 'kan_silu', 32, 128, 80, 4),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'BAND TAP-RB HALO', 'kan_silu', 32, 1, 80, 4, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'BAND TAP-RB TAP-PM', 'kan_silu', 32, 1, 16, 4, affine=True),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'HALO TAP-RB EXPANDED', 'kan_silu', 32, 128, 128, 4, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'HALO TAP-RB HALO', 'kan_silu', 32, 2, 128, 4),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'BAND TAP-RB EXPANDED', 'kan_silu', 32, 256, 160, 4, G=2, scale=3.0, affine=True),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'BAND TAP-RB HALO', 'kan_silu', 32, 2, 160, 4, G=2),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'BAND TAP-RB TAP-PM', 'kan_silu', 32, 2, 32, 4, G=2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'HALO TAP-RB EXPANDED', 'kan_silu', 32, 256, 256, 4, G=2, affine=True),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA', 'HALO TAP-RB HALO', 'kan_silu', 32, 4, 256, 4, G=2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA+QUAD_FWD', 'HALO+RB TAP-RB EXPANDED', 'kan_silu', 32, 128, 256, 4),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA+QUAD_FWD', 'HALO+RB TAP-RB HALO', 'kan_silu', 32, 2, 256, 4, scale=3.0, affine=True),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA+QUAD_FWD', 'HALO+RB TAP-RB EXPANDED', 'kan_silu', 32, 256, 512, 4, G=2),
    orow('FAST_BSPLINE_SILU', 'QUAD_BWD_DATA+QUAD_FWD', 'HALO+RB TAP-RB HALO', 'kan_silu', 32, 4, 512, 4, G=2, scale=3.0),
    orow('FAST_BSPLINE_SILU', 'ROWBLK8_FWD', 'HALO TAP HALO', 'kan_silu', 40, 2, 256, 8, affine=True),
    orow('FAST_BSPLINE_SILU', 'ROWBLK8_FWD', 'HALO TAP HALO', 'kan_silu', 40, 4, 512, 8, G=2, scale=3.0),
    # FAST_POLY4
    orow('FAST_POLY4', 'QUAD_FWD', 'HALO+RB TAP TAP-PM', 'lucas_d3', 32, 2, 256, 4),
    orow('FAST_POLY4', 'QUAD_FWD', 'HALO+RB TAP TAP-PM', 'bessel_d3', 32, 4, 512, 4, G=2, affine=True),
    orow('FAST_POLY4', 'ROWBLK8_FWD', 'HALO TAP TAP', 'jacobi_d3', 4, 2, 256, 8),
    orow('FAST_POLY4', 'ROWBLK8_FWD', 'HALO TAP TAP', 'bersnstein_d3', 4, 4, 512, 8, G=2),
    # FAST_RELU8
    orow('FAST_RELU8', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM EXPANDED', 'relu_g5k3', 128, 128, 80, 2, affine=True),
    orow('FAST_RELU8', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM TAP-PM', 'relu_g5k3', 128, 2, 80, 2, scale=3.0),
    orow('FAST_RELU8', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM EXPANDED', 'relu_g5k3', 128, 256, 160, 2, G=2),
    orow('FAST_RELU8', 'FWD_WEIGHT_SIDE', 'EXPANDED TAP-PM TAP-PM', 'relu_g5k3', 128, 4, 160, 2, G=2, scale=3.0, affine=True),
    # the other split kind of a (spec class, bit) whose cell rows run only one: two forward slabs
    orow('FAST_POLY4', 'QUAD_FWD', 'HALO+RB TAP TAP-PM', 'lucas_d3', 32, 4, 256, 4),
    orow('FAST_POLY4', 'ROWBLK8_FWD', 'HALO TAP TAP', 'bessel_d3', 4, 4, 256, 8),
]
