"""CPU: the tile-order matrix (tests/order_cells.py) stays in step with the planner -- the five properties of tests/test_route_matrix.py on
order_key, whose second field is what kan_tile_orders reports:

(a) every ORDER_CASES row plans to exactly its declared key, so a planner change that widens, narrows or moves the predicate of a tile order fails
    here instead of silently leaving the order without its oracle check;
(b) every key with a tile order that the planner reaches -- over tests/golden/plan_snapshot.json and a grid over every basis spec, planes 2 / 4 / 8 /
    16, fourteen batches, one and two groups, C up to 256 and O up to 512 per group -- has a row, and conversely every row's key is reached, so
    deleting the only row of a cell fails (b);
(c) every first row of a cell is the smallest geometry of the grid that reaches it;
(d) wherever the planner runs the stage of a (spec class, tile order) both with one slab and with several, the table runs both;
(e) exemptions are live, and at most two.
And the scope tests/test_gpu_order_matrix.py relies on: no grid geometry of a basis with a second input, and none with the 1x1 kernel W_IOD needs,
has the 8x8 weight-gradient bit, so `ops._conv_backward` (ops.py:839) takes that entry wherever the bit is set."""
import functools
import json
import os

import pytest

from conftest import GOLDEN
from golden.make_plan_snapshot import basis_specs, geom, make_structs
from order_cells import EXEMPT, ORDER_CASES, STAGE_OF, case_ids, ops_takes_pos8_bw, order_id, order_key, order_names, order_splits, work
from route_cells import case_structs, plan_of, second_input

S3 = dict(k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1))          # every tile order is made for 3x3 / stride 1 / pad 1 / dilation 1
BATCHES = (1, 2, 4, 6, 8, 16, 17, 32, 40, 48, 64, 96, 128, 256)
PLANES = (2, 4, 8, 16)
COARSE_C, COARSE_O = (1, 2, 3, 8, 16, 64, 128, 256), (1, 2, 16, 40, 64, 96, 128, 192, 256, 384, 512)
FINE_C, FINE_O = (1, 2, 3, 4) + tuple(range(8, 257, 8)), (1, 2) + tuple(range(16, 513, 16))
FINE_SPECS = ("kan_silu", "kan_gelu", "lucas_d3", "relu_g5k3")      # one basis per spec class that has a tile order: searched in steps of 8 / 16


def grid_cases():
    """(tag, geometry list, basis list): every spec of make_plan_snapshot.basis_specs() on the coarse channel grid, the specs with tile orders on
    the fine one as well (channels in steps of 8, outputs in steps of 16: the search the rows are the minima of), and 1x1 kernels on 8x8 planes
    (the kernel shape of every W_IOD launch)."""
    out = []
    for name, bl in sorted(basis_specs().items()):
        for Cs, Os in ((COARSE_C, COARSE_O),) + (((FINE_C, FINE_O),) if name in FINE_SPECS else ()):
            for hw in PLANES:
                for B in BATCHES:
                    for G in (1, 2):
                        out += [(f"grid:{name}:{hw}:B{B}:G{G}", geom(B, C_, hw, hw, O, G=G, **S3), bl) for C_ in Cs for O in Os]
        for B in (2, 32, 64):
            out += [(f"1x1:{name}:B{B}", geom(B, C_, 8, 8, O, k=(1, 1), p=(0, 0)), bl) for C_ in (2, 16, 128) for O in (16, 128, 256)]
    return out


@functools.lru_cache(maxsize=1)
def planned():
    """([(tag, geometry, key, {bit: slabs}, work)] of the planned geometries that have a tile order, [(tag, geometry, basis, order names)] of all
    that plan, [rejected])."""
    with open(os.path.join(GOLDEN, "plan_snapshot.json")) as fh:
        snap = json.load(fh)
    cases = [(c["tag"], c["g"], snap["bases"][c["b"]]) for c in snap["cases"] if "plan" in c] + grid_cases()
    cells, every, rejected = [], [], []
    for tag, gl, bl in cases:
        g, b = make_structs(gl, bl)
        names = order_names(g, b)
        every.append((tag, gl, b, names))
        if not names:
            continue
        p = plan_of(g, b)
        if p is None:
            rejected.append((tag, gl))
            continue
        cells.append((tag, gl, order_key(g, b, p), order_splits(g, b, p), g.B * g.H * g.W * g.C * g.O * max(1, g.groups)))
    return cells, every, rejected


def reachable():
    """{key: (tag, geometry, work) of the cheapest geometry that reaches it}."""
    seen = {}
    for tag, gl, key, _, w in planned()[0]:
        if key not in seen or w < seen[key][2]:
            seen[key] = (tag, gl, w)
    return seen


def split_kinds(rows):
    """{(spec class, bit): {False, True}}: whether one-slab (False) and several-slab (True) launches of the bit's stage occur among (key, {bit: slabs})."""
    out = {}
    for key, splits in rows:
        for bit, n in splits.items():
            out.setdefault((key[0], bit), set()).add(n > 1)
    return out


@pytest.mark.parametrize("case", ORDER_CASES, ids=case_ids(ORDER_CASES))
def test_order_case_plans_to_its_key(case):
    g, b, p = case_structs(case)
    assert order_key(g, b, p) == case["key"], f"row {case} now plans to {order_key(g, b, p)}"
    assert case["key"][1] and set(case["key"][1]) <= set(STAGE_OF)


def test_grid_geometries_with_a_tile_order_all_plan():
    cells, _, rejected = planned()
    assert not rejected and len(cells) > 1000, f"{len(rejected)} geometries with a tile order do not plan, e.g. {rejected[:5]}"


def test_every_reachable_cell_has_a_row():
    have = {c["key"] for c in ORDER_CASES}
    missing = {k: v for k, v in reachable().items() if k not in have and k not in EXEMPT}
    assert not missing, f"{len(missing)} reachable tile-order cells have no ORDER_CASES row:\n" + \
        "\n".join(f"  {order_id(k)}  (cheapest: {tag}, geom {gl})" for k, (tag, gl, _) in sorted(missing.items()))


def test_every_row_is_a_reachable_cell():
    """The converse: the grid reaches every cell the table holds, so deleting the only row of any cell fails the check above."""
    reach = reachable()
    unreached = sorted({order_id(c["key"]) for c in ORDER_CASES if c["key"] not in reach})
    assert not unreached, f"{len(unreached)} ORDER_CASES cells are reached by no snapshot or grid geometry: {unreached}"


def test_first_row_of_every_cell_is_its_smallest_geometry():
    reach, seen, big = reachable(), set(), []
    for c in ORDER_CASES:
        if c["key"] in seen or c["key"] not in reach:
            continue
        seen.add(c["key"])
        if work(c) > reach[c["key"]][2]:
            big.append((order_id(c["key"]), work(c), reach[c["key"]]))
    assert not big, f"rows larger than the smallest geometry that reaches their cell (row work, (tag, geometry, work)): {big}"


def test_single_and_split_launches_of_every_order():
    """Wherever the planner runs the stage of a (spec class, tile order) both with one slab and with several, the table runs both."""
    want = split_kinds((key, splits) for _, _, key, splits, _ in planned()[0])
    have = split_kinds((c["key"], order_splits(*case_structs(c))) for c in ORDER_CASES)
    assert all(kinds == {False, True} for kinds in want.values()), f"a tile order the grid reaches with one split kind only: {want}"
    short = {sb: sorted(kinds - have.get(sb, set())) for sb, kinds in want.items() if kinds - have.get(sb, set())}
    assert not short, "(spec class, order): split kinds (False = one slab, True = several) the planner makes and no row runs: " + str(short)


def test_exemptions_are_live():
    """An exempted cell has no row and is still reached; at most two cells may be exempt."""
    assert len(EXEMPT) <= 2
    assert not set(EXEMPT) & {c["key"] for c in ORDER_CASES}, "an exempted cell also has a row: drop the exemption"
    assert set(EXEMPT) <= set(reachable()), "an exempted cell is no longer reached: drop the exemption"


def test_ops_takes_the_weight_gradient_entry_wherever_its_bit_is_set():
    """ops.py:839 withholds kan_conv_bwd_weight_rowgroups from a launch with a second input tensor or W_IOD weights.  The GPU matrix expects a
    k_conv_bwd_weight_pos8 sample for every row with the bit: that holds because no such launch has it."""
    every = planned()[1]
    xn = [(tag, gl) for tag, gl, b, names in every if second_input(b)]
    iod = [(tag, gl) for tag, gl, b, names in every if (gl[7], gl[8], gl[15]) == (1, 1, 1)]       # 1x1 kernel, one group: what w_layout = W_IOD requires
    assert len(xn) > 1000 and len(iod) > 500
    for tag, gl, b, names in every:
        w_iod = (gl[7], gl[8], gl[15]) == (1, 1, 1)
        if second_input(b) or w_iod:
            assert "POS8_BWD_WEIGHT" not in names, f"{tag} {gl}: the 8x8 weight-gradient bit on a launch ops.py:839 withholds it from"
        assert ops_takes_pos8_bw(names, b, w_iod) == ("POS8_BWD_WEIGHT" in names)
    for c in ORDER_CASES:
        g, b, p = case_structs(c)
        assert ops_takes_pos8_bw(c["key"][1], b) == ("POS8_BWD_WEIGHT" in c["key"][1])
