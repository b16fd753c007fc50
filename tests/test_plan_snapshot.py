"""CPU: the planner reproduces tests/golden/plan_snapshot.json -- every KanPlan field and kan_pack_cacheable of ~1.3k geometries (the conv
layers of KAN-VGG11, FastKAN-VGG11 and ChebyKAN-AlexNet, the golden cfgs, a seeded grid over every basis kind and compile-time spec), and
the return code and message of the geometries kan_plan rejects.  Regenerate with tests/golden/make_plan_snapshot.py only on purpose."""
import ctypes
import json
import os

from convkan_amd import _lib as L
from conftest import GOLDEN
from golden.make_plan_snapshot import GEOM_FIELDS, make_structs


def test_planner_reproduces_the_snapshot():
    with open(os.path.join(GOLDEN, "plan_snapshot.json")) as fh:
        snap = json.load(fh)
    assert snap["geom_fields"] == list(GEOM_FIELDS)
    assert snap["plan_fields"] == [n for n, _ in L.KanPlan._fields_]
    lib = L.load()
    diffs = []
    for i, c in enumerate(snap["cases"]):
        g, b = make_structs(c["g"], snap["bases"][c["b"]])
        p = L.KanPlan()
        rc = lib.kan_plan(ctypes.byref(g), ctypes.byref(b), ctypes.byref(p))
        if "plan" not in c:
            got = {"rc": rc, "msg": lib.kan_last_error().decode() if rc else None}
            want = {"rc": c["rc"], "msg": c["msg"]}
        else:
            got = {"rc": rc, "plan": dict(zip(snap["plan_fields"], (getattr(p, n) for n in snap["plan_fields"]))),
                   "cacheable": lib.kan_pack_cacheable(ctypes.byref(g), ctypes.byref(b))}
            want = {"rc": 0, "plan": dict(zip(snap["plan_fields"], c["plan"])), "cacheable": c["cacheable"]}
        if got != want:
            diffs.append(f"case {i} ({c['tag']}, geom {c['g']}): got {got}, want {want}")
    assert not diffs, f"{len(diffs)} of {len(snap['cases'])} cases differ:\n" + "\n".join(diffs[:10])
