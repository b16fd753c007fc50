"""CPU: the route matrix (tests/route_cells.py) stays in step with the planner.

(a) every ROUTE_CASES row plans to exactly its declared (spec class, fwd, bwd-data, bwd-weight) key, so a planner change that
    moves a row to another route fails here instead of silently leaving a route without its oracle check;
(b) every cell the planner reaches -- over the geometries of tests/golden/plan_snapshot.json and a seeded grid over every
    compile-time spec, kernel shape, plane size and batch -- has a row, so a planner change that opens a new route for a spec
    fails here until an oracle row (tests/test_gpu_route_matrix.py) is added for it; and conversely every row's cell is reached,
    so deleting the only row of a cell fails (b);
(c) wherever the planner gives a (stage, route) both single-slab and split-K launches, the table runs both."""
import functools
import json
import os
import random

import pytest

from conftest import GOLDEN
from golden.make_plan_snapshot import basis_specs, geom, make_structs
from route_cells import ROUTE_CASES, case_ids, case_structs, key_id, plan_of, route_key, stage_splits

# cells knowingly left without a row: {key: "the GPU test that covers it instead"}.  Empty on purpose.
EXEMPT = {}

SHAPES = {"3x3": dict(k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1)), "1x1": dict(k=(1, 1), s=(1, 1), p=(0, 0), d=(1, 1)),
          "strided": dict(k=(3, 3), s=(2, 2), p=(1, 1), d=(1, 1)), "dilated": dict(k=(3, 3), s=(1, 1), p=(2, 2), d=(2, 2))}
WIDE_SHAPES = dict(SHAPES, **{"5x5": dict(k=(5, 5), s=(1, 1), p=(2, 2), d=(1, 1)), "p0": dict(k=(3, 3), s=(1, 1), p=(0, 0), d=(1, 1)),
                              "5x5s2": dict(k=(5, 5), s=(2, 2), p=(2, 2), d=(1, 1)), "1x1p1": dict(k=(1, 1), s=(1, 1), p=(1, 1), d=(1, 1)),
                              "1x1p2": dict(k=(1, 1), s=(1, 1), p=(2, 2), d=(1, 1))})
STAGES = ("fwd", "bd", "bw")


def grid_cases():
    """(tag, geometry list, basis list) of the seeded grid, every spec of make_plan_snapshot.basis_specs() in three parts:
    every shape x plane x batch of the small grid with channels / outputs / groups drawn; the same over wider shapes, planes, batches
    and channel counts; and every (batch, channels, outputs, groups) on the small planes where the halo, row-block, expanded and
    position-major routes meet."""
    rng = random.Random(20261016)
    out = []
    for name, bl in sorted(basis_specs().items()):
        for shape, sk in SHAPES.items():
            for hw in (2, 4, 8, 16, 32):
                for B in (16, 17, 128):
                    r = rng.random()
                    if r < 0.1:
                        C_, O, G = 1, rng.choice([1, 2]), rng.choice([4, 16])          # depthwise
                    else:
                        C_ = rng.choice([1, 2, 3, 4, 16, 64, 128])
                        O = rng.choice([16, 64, 96, 128, 192, 256])
                        G = 2 if r < 0.2 else 1
                    out.append((f"grid:{name}:{shape}:{hw}:B{B}", geom(B, C_, hw, hw, O, G=G, **sk), bl))
        for shape, sk in WIDE_SHAPES.items():
            for hw in (2, 3, 4, 5, 8, 13, 16, 32):
                for B in (1, 8, 16, 17, 128, 256):
                    for _ in range(4):
                        G = rng.choice([1, 1, 2])
                        C_ = rng.choice([1, 2, 3, 5, 16, 64, 128, 256, 512, 1024])
                        O = rng.choice([1, 2, 16, 40, 96, 128, 192, 256, 384, 512, 1024])
                        g = geom(B, C_, hw, hw, O, G=G, **sk)
                        # non-empty output, activations under 2 GiB (kan_plan's 32-bit buffer offsets: check() in kan_plan.hip)
                        if g[5] > 0 and g[6] > 0 and B * max(g[16], g[17]) * 4 < 2 ** 31:
                            out.append((f"wide:{name}:{shape}:{hw}:B{B}", g, bl))
        for shape, planes in (("3x3", (2, 4, 8)), ("1x1p1", (2,)), ("1x1p2", (2,))):
            for hw in planes:
                for B in (1, 2, 8, 16, 17, 128, 256):
                    for C_ in (1, 2, 3, 64, 128, 256, 512, 1024):
                        for O in (1, 2, 40, 96, 128, 256, 384, 512, 1024):
                            for G in (1, 2):
                                out.append((f"dense:{name}:{shape}:{hw}:B{B}", geom(B, C_, hw, hw, O, G=G, **WIDE_SHAPES[shape]), bl))
    return out


@functools.lru_cache(maxsize=1)
def planned():
    """[(tag, geometry, key, (fwd, bwd-data, bwd-weight splits))] over the snapshot's planned geometries and the grid, and the grid
    geometries kan_plan rejected."""
    with open(os.path.join(GOLDEN, "plan_snapshot.json")) as fh:
        snap = json.load(fh)
    cases = [(c["tag"], c["g"], snap["bases"][c["b"]]) for c in snap["cases"] if "plan" in c] + grid_cases()
    out, rejected = [], []
    for tag, gl, bl in cases:
        g, b = make_structs(gl, bl)
        p = plan_of(g, b)
        if p is None:
            rejected.append((tag, gl))
            continue
        out.append((tag, gl, route_key(g, b, p), tuple(stage_splits(p, st) for st in STAGES)))
    return out, rejected


def reachable():
    """{key: first (tag, geometry) that reaches it}."""
    seen = {}
    for tag, gl, key, _ in planned()[0]:
        seen.setdefault(key, (tag, gl))
    return seen


def split_kinds(rows):
    """{(stage, route): {False, True}}: whether single-slab (False) and split (True) launches occur among (key, splits) pairs."""
    out = {}
    for key, splits in rows:
        for i, st in enumerate(STAGES):
            out.setdefault((st, key[1 + i]), set()).add(splits[i] > 1)
    return out


@pytest.mark.parametrize("case", ROUTE_CASES, ids=case_ids(ROUTE_CASES))
def test_route_case_plans_to_its_key(case):
    g, b, p = case_structs(case)
    assert route_key(g, b, p) == case["key"], f"row {case} now plans to {route_key(g, b, p)}"


def test_grid_geometries_all_plan():
    """A grid geometry the planner starts rejecting would shrink what the completeness checks see without failing them."""
    rejected = planned()[1]
    assert not rejected, f"{len(rejected)} grid geometries no longer plan, e.g. {rejected[:5]}"


def test_every_reachable_cell_has_a_row():
    have = {c["key"] for c in ROUTE_CASES}
    missing = {k: v for k, v in reachable().items() if k not in have and k not in EXEMPT}
    assert not missing, f"{len(missing)} reachable route cells have no ROUTE_CASES row:\n" + \
        "\n".join(f"  {key_id(k)}  (first reached by {tag}, geom {gl})" for k, (tag, gl) in sorted(missing.items()))


def test_every_row_is_a_reachable_cell():
    """The converse: the grid reaches every cell the table holds, so deleting the only row of any cell fails the check above."""
    reach = reachable()
    unreached = sorted({key_id(c["key"]) for c in ROUTE_CASES if c["key"] not in reach})
    assert not unreached, f"{len(unreached)} ROUTE_CASES cells are reached by no snapshot or grid geometry: {unreached}"


def test_single_and_split_launches_of_every_stage_route():
    """Wherever the planner gives a (stage, route) both a single-slab and a split-K launch, the table runs both."""
    want = split_kinds((key, splits) for _, _, key, splits in planned()[0])
    have = split_kinds((c["key"], tuple(stage_splits(case_structs(c)[2], st) for st in STAGES)) for c in ROUTE_CASES)
    short = {sr: sorted(kinds - have.get(sr, set())) for sr, kinds in want.items() if kinds - have.get(sr, set())}
    assert not short, "(stage, route): split kinds (False = one slab, True = split-K) the planner makes and no row runs: " + str(short)


def test_exemptions_are_live():
    """An exempted cell has no row and is still reached (a stale exemption would hide a cell the planner no longer opens)."""
    assert not set(EXEMPT) & {c["key"] for c in ROUTE_CASES}, "an exempted cell also has a row: drop the exemption"
    assert set(EXEMPT) <= set(reachable()), "an exempted cell is no longer reached: drop the exemption"
