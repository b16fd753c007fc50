"""Print the BAND_CASES rows of tests/band_cells.py from its committed grid: for every cell `kan_band_route` reaches there, the smallest geometry
under band_cells.order().  The grid defines "reached"; this search only restates it as rows, and tests/test_band_matrix.py checks the result.

    python tools/make_band_cases.py > rows.txt          # CPU only; paste between the brackets of BAND_CASES

Instantiation cells take their own spec.  A feature cell ties over the specs on its smallest geometry: it takes a spec that already has a row there,
else SPEC_LAYERS[(B + C + O + H + W + G) % 6] first.  Rows that end up the smallest of no cell are dropped.  Input scale, affine norm and the
recurrence family alternate by row; a row's `seed=` and the comment that gives its reason are kept by hand."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import band_cells as BC      # noqa: E402


def frozen(c):
    return tuple(sorted(c.items()))


def cells(layer, c):
    g, b = BC.geom_of(c), BC.basis_of(layer)
    r = BC.band_route(g, b)
    return r, (BC.cells_of(g, b, r) if r is not None and r.fwd_band else [])


def main():
    n = len(BC.SPEC_LAYERS)
    best, cand = {}, collections.defaultdict(dict)
    launches = []
    for c in BC.grid():
        o = BC.order(c)
        rot = (c["B"] + c["C"] + c["O"] + c["H"] + c["W"] + c["G"]) % n
        for layer in BC.grid_layers(c):
            _, cs = cells(layer, c)
            if cs:
                launches.append((o, layer, c, cs))
            for cell in cs:
                k = (o, (BC.SPEC_LAYERS.index(layer) - rot) % n if cell[0] in ("Ff", "Wf") else 0)
                if cell not in best or k < best[cell][0]:
                    best[cell] = (k, layer, c)
    for o, layer, c, cs in launches:
        for cell in cs:
            if cell[0] in ("Ff", "Wf") and best[cell][0][0] == o:
                cand[cell][layer] = c
    rows = collections.OrderedDict()
    for cell in sorted(best, key=lambda x: tuple(map(str, x))):
        if cell[0] in ("F", "W"):
            rows.setdefault((best[cell][1], frozen(best[cell][2])), None)
    for cell in sorted(cand, key=lambda x: (x[0] != "Wf",) + tuple(map(str, x))):       # the weight gradient's cells first: fewer specs have them
        have = [l for l in BC.SPEC_LAYERS if l in cand[cell] and (l, frozen(cand[cell][l])) in rows]
        layer = have[0] if have else best[cell][1]
        rows.setdefault((layer, frozen(cand[cell][layer])), None)
    changed = True
    while changed:                                      # drop rows whose every smallest cell another row of the same order serves
        changed = False
        for k in list(rows):
            o = BC.order(dict(k[1]))
            mine = [cell for cell in cells(k[0], dict(k[1]))[1] if best[cell][0][0] == o]
            others = set()
            for k2 in rows:
                if k2 != k and BC.order(dict(k2[1])) == o:
                    others |= set(cells(k2[0], dict(k2[1]))[1])
            if all(cell in others for cell in mine):
                del rows[k]
                changed = True
                break
    poly = 0
    for i, (layer, ct) in enumerate(sorted(rows, key=lambda k: (BC.SPEC_LAYERS.index(k[0]), BC.order(dict(k[1]))))):
        c = dict(ct)
        r, _ = cells(layer, c)
        opts = ", scale=3.0" if layer in ("kan_silu", "kan_gelu", "fast_g8") and i % 2 == 1 else ""
        opts += ", affine=True" if i % 3 == 2 else ""
        if layer == "lucas_d3":
            poly += 1
            layer = "bessel_d3" if poly % 2 == 0 else layer
        bw = f"'{r.bw_WR}/{r.bw_NI}/{r.bw_slots}'" if r.bw_band else "None"
        grp = f", G={c['G']}" if c["G"] != 1 else ""
        print(f"    brow('{layer}', '{c['shape']}', {c['B']}, {c['C']}, {c['O']}, {c['H']}, {c['W']}, '{r.NG}/{r.MO}/{r.WP}', {bw}{grp}{opts}),")
    print(f"{len(best)} cells, {len(rows)} rows", file=sys.stderr)


if __name__ == "__main__":
    main()
