"""CPU: the norm cell matrix (tests/norm_cells.py) stays in step with `kan_norm_route`, the function the InstanceNorm (+ PReLU,
+ max-pool) entry points dispatch from.

(a) every NORM_CASES row routes, forward and backward, to exactly its declared key, so a moved threshold fails here instead of
    silently leaving a kernel variant without its fp64 check;
(b) every cell the dispatch reaches over a grid of planes, pool modes, slab counts, plane counts and pointer alignments has a row,
    and every row's cell is reached by the grid, so deleting the only row of a cell fails; every capped launcher has a row in which
    a workgroup runs its grid-stride loop more than once, and one in which none does;
(c) every switch point of the un-pooled and of the pooled-2x2 dispatch (the sizes n | n + 1 between which the cell changes) has a
    row on each side, at exactly those sizes; the rows the table is specified to hold beyond that (the 1x1 plane, the general-pool
    geometries, the slab counts, parameter combinations, ties, ...) are there; and every row is needed: the table without it
    breaks one of (b), (c) -- so deleting any row fails here;
(d) every row keeps the share of outputs its conditioning masks under norm_cells.MASK_CAP, and the tie rows really hold partial
    ties whose first maximum is not the window's first element, from the fp64 reference alone."""
import functools

import pytest

import convkan_amd as K
from norm_cells import MASK_CAP, NORM_CASES, case_id, case_ids, case_route, cell_of, launcher_of, mask_share, norm_key, route, tie_stats

# cells knowingly left without a row: {cell: "the GPU test that covers it instead"}.  Empty on purpose.
EXEMPT = {}

POOLS = (None, (2, 2), (3, 2), (3, 1), (5, 3), (7, 1), (15, 4), (15, 15), (2, 1))      # (2, 2): the 2x2 mode on even planes, general on odd ones
PLANES = ((3, 7), (5, 13), (4, 10000))                                                # 21, 65 and 40000 planes


@pytest.fixture(scope="module", autouse=True)
def _library():
    K.build_library()


@functools.lru_cache(maxsize=1)
def reached():
    """{key: first (B, C, H, W, S, pool, aligned) of the grid that reaches it}, plus the cap rows' own launches."""
    seen = {}
    for H in range(1, 73):
        for W in range(1, 73):
            for pool in POOLS:
                if pool and (H < pool[0] or W < pool[0]):
                    continue
                fallback = pool == (2, 2) and H % 2 == 0 and W % 2 == 0          # only the pooled 2x2 forward looks at the alignment
                for B, C in PLANES:
                    for S in (1, 2):
                        for bwd, aligned in ((False, True), (True, True)) + (((False, False),) if fallback else ()):
                            seen.setdefault(norm_key(route(bwd, B, C, H, W, S, pool, aligned), bwd), (B, C, H, W, S, pool, aligned))
    for case in NORM_CASES:
        if max(case["B"], case["C"]) > 500:                                       # the cap rows
            for bwd in (False, True):
                seen.setdefault(norm_key(case_route(case, bwd), bwd), tuple(case[k] for k in ("B", "C", "H", "W", "S", "pool")) + (True,))
    return seen


def declared(cases=NORM_CASES):
    return [c[d] for c in cases for d in ("fwd", "bwd")]


@functools.lru_cache(maxsize=1)
def switch_points():
    """[(bwd, pooled, n, cell at n, n + step, cell there)]: the neighbouring plane sizes (pixels; un-pooled 1 x n planes, pooled 2 x n / 2
    ones in steps of one window) between which the dispatch changes cell."""
    out = []
    for bwd in (False, True):
        for pooled in (False, True):
            step = 4 if pooled else 1
            sizes = range(step, 1101, step)
            cells = [cell_of(norm_key(route(bwd, 3, 7, 2 if pooled else 1, n // 2 if pooled else n, 1, (2, 2) if pooled else None), bwd)) for n in sizes]
            out += [(bwd, pooled, n, a, n + step, b) for n, a, b in zip(sizes, cells, cells[1:]) if a != b]
    return out


FAMILIES = ("fwd-REGS", "fwd-GEN", "bwd-REGS", "bwd-GEN")
GENERAL_POOLS = [(3, 2, 13, 13), (3, 2, 27, 27), (3, 2, 55, 55), (3, 2, 57, 56), (2, 2, 57, 57), (2, 2, 13, 11), (3, 1, 12, 14), (5, 3, 17, 17),
                 (7, 1, 9, 20), (15, 4, 31, 17), (15, 15, 15, 31), (3, 2, 3, 3), (3, 2, 9, 4), (2, 1, 2, 9), (3, 2, 5, 5), (3, 2, 7, 9), (3, 2, 19, 19)]


def _families(c):
    return {k[:8].rstrip("-") for k in (c["fwd"], c["bwd"])}


def shortfalls(cases):
    """What the table `cases` lacks, as a list of sentences (empty: complete)."""
    out = []
    have, reach = {cell_of(k) for k in declared(cases)}, {cell_of(k) for k in reached()}
    out += [f"reachable cell without a row: {k}" for k in sorted(reach - have - set(EXEMPT))]
    out += [f"row cell no grid launch reaches: {k}" for k in sorted(have - reach)]
    kinds = lambda keys: {(launcher_of(k), k.endswith("-strided")) for k in keys if launcher_of(k)}
    out += [f"no row runs launcher {l} {'strided' if s else 'unstrided'}" for l, s in sorted(kinds(reached()) - kinds(declared(cases)))]
    plain = [c for c in cases if max(c["B"], c["C"]) <= 500]
    for bwd, pooled, n0, cell0, n1, cell1 in switch_points():
        for n, cell in ((n0, cell0), (n1, cell1)):
            ok = any(c["H"] * c["W"] == n and cell_of(c["bwd" if bwd else "fwd"]) == cell and
                     (c["pool"] == (2, 2) and c["H"] % 2 == 0 and c["W"] % 2 == 0 if pooled else not c["pool"]) for c in plain)
            if not ok:
                out.append(f"switch point {n0} | {n1} pixels of the {'backward' if bwd else 'forward'}{', pooled 2x2' if pooled else ''}: no row of {n} pixels in {cell}")
    named = {
        "a 1x1 plane": lambda c: c["H"] * c["W"] == 1 and not c["pool"],
        "a 56x56 plane without a pool": lambda c: (c["H"], c["W"], c["pool"]) == (56, 56, None),
        "the generic 2x2 mode on 34x34": lambda c: (c["H"], c["W"], c["pool"]) == (34, 34, (2, 2)),
        "the generic 2x2 mode on 2x514": lambda c: (c["H"], c["W"], c["pool"]) == (2, 514, (2, 2)),
        "32 slabs on a pooled 2x2 plane": lambda c: (c["H"], c["W"], c["pool"], c["S"]) == (2, 2, (2, 2), 32),
        "3 slabs on a pooled register row": lambda c: c["S"] == 3 and c["fwd"].startswith("fwd-REGS") and c["fwd"].endswith("pool2"),
        "the alignment fallback on a pooled 8x8 plane": lambda c: (c["H"], c["W"], c["pool"], c["kind"]) == (8, 8, (2, 2), "unaligned"),
    }
    for k, s_, H, W in GENERAL_POOLS:
        named[f"pool ({k}, {s_}) on {H}x{W}"] = lambda c, q=(H, W, (k, s_), None): (c["H"], c["W"], c["pool"], c["kind"]) == q
    for kind in ("const", "ties"):
        for fam in ("fwd-REGS", "fwd-GEN"):
            named[f"a '{kind}' row on {fam}"] = lambda c, kind=kind, fam=fam: c["kind"] == kind and c["fwd"].startswith(fam)
    for fam in FAMILIES:
        for S in (2, 5, 9, 32):
            named[f"{S} slabs on {fam}"] = lambda c, fam=fam, S=S: c["S"] == S and fam in _families(c)
        for what, pred in (("2 groups", lambda c: c["groups"] == 2 and c["slope"]), ("3 groups", lambda c: c["groups"] == 3 and c["slope"]),
                           ("no affine", lambda c: c["affine"] == ""), ("negative gammas", lambda c: c["affine"] == "GB"),
                           ("gamma alone", lambda c: c["affine"] == "g"), ("beta alone", lambda c: c["affine"] == "b"),
                           ("no slope", lambda c: c["slope"] == ""), ("a negative slope", lambda c: c["slope"] == "-")):
            named[f"{what} on {fam}"] = lambda c, fam=fam, pred=pred: bool(pred(c)) and fam in _families(c)
    out += [f"no row with {what}" for what, pred in named.items() if not any(pred(c) for c in cases)]
    return out


@pytest.mark.parametrize("case", NORM_CASES, ids=case_ids(NORM_CASES))
def test_norm_case_routes_to_its_keys(case):
    got = tuple(norm_key(case_route(case, bwd), bwd) for bwd in (False, True))
    assert got == (case["fwd"], case["bwd"]), f"row {case} now routes to {got}"


def test_table_is_complete():
    """Cells both ways, strided and unstrided launchers, both sides of every switch point, the specified rows."""
    assert {l for l, s in {(launcher_of(k), k.endswith("-strided")) for k in reached()} if s} == \
        {"fwd_regs", "bwd_regs_NT1024", "bwd_regs_NT256", "bwd_generic"}
    assert len(switch_points()) == 2 * 9 + 7 + 9, switch_points()          # un-pooled: 8 variant changes + registers | generic, both directions; pooled likewise
    lacks = shortfalls(NORM_CASES)
    assert not lacks, "\n".join(lacks)


@pytest.mark.parametrize("idx", range(len(NORM_CASES)), ids=case_ids(NORM_CASES))
def test_every_row_is_needed(idx):
    """The table without this row lacks something: no row can be deleted unnoticed."""
    assert shortfalls(NORM_CASES[:idx] + NORM_CASES[idx + 1:]), f"nothing asks for row {case_id(NORM_CASES[idx])}"


def test_exemptions_are_live():
    assert not set(EXEMPT) & {cell_of(k) for k in declared()}, "an exempted cell also has a row: drop the exemption"
    assert set(EXEMPT) <= {cell_of(k) for k in reached()}, "an exempted cell is no longer reached: drop the exemption"


@pytest.mark.parametrize("case", NORM_CASES, ids=case_ids(NORM_CASES))
def test_mask_share_under_cap(case):
    share = mask_share(case)
    print(f"[norm mask] {case['fwd']} / {case['bwd']}: {share:.2e} of the outputs masked")
    assert share <= MASK_CAP, f"{case}: {share:.3%} of the outputs are masked (cap {MASK_CAP:.0%}): give the row another seed"


@pytest.mark.parametrize("case", [c for c in NORM_CASES if c["kind"] == "ties"], ids=case_id)
def test_tie_rows_hold_partial_ties(case):
    partial, late = tie_stats(case)
    assert partial >= 20 and late >= 10, f"{case}: {partial} unmasked windows with a partial tie, {late} of them with the first maximum past element 0"
