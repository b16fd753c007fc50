"""CPU: what the AdamW cell matrix (tests/adamw_cells.py) rests on before any GPU runs.

(a) the fp64 reference equals torch.optim.AdamW(foreach=False) -- the optimizer the reference project builds, generic_train.py:24 -- on fp64
    parameters over 6 steps to 1e-12 relative, for every hyper-parameter set, grad_scale folded into the gradient;
(b) every row's declared cell key is what a restatement of the launch arithmetic derives from the row's arguments, every reachable cell has
    a row, and the free attributes take each of their values on rows of both classes;
(c) the `flatten` row's tables are the ones FusedAdamW._flatten builds;
(d) the judge can fail: the kernel's arithmetic restated in fp32 passes every row, each of seven deliberately wrong restatements is
    rejected on at least one row;
(e) no row masks more than MASK_CAP of its elements, and both references are finite on every element they are judged on;
(f) the special-value row's fp32 reference has the properties the GPU test relies on."""
import math

import pytest
import torch

import convkan_amd as K
from adamw_cells import (ADAMW_CASES, GSCALES, HYPER, MASK_CAP, REACHABLE_FLAT, REACHABLE_SEG, STEPS, WRONG, case_id, fake_grad_addresses, flat_key,
                         judge, judged_elems, kernel_restatement, layout, n_elems, reference_pair, seg_key, special_inputs, special_reference,
                         torch_order_step)

SMALL = [i for i, c in enumerate(ADAMW_CASES) if n_elems(c) <= 100_000]


@pytest.mark.parametrize("name", HYPER)
@pytest.mark.parametrize("gscale", GSCALES)
def test_fp64_reference_is_torch_adamw(name, gscale):
    lr, betas, eps, wd = HYPER[name]
    gen = torch.Generator().manual_seed(7)
    n = 301
    p0 = torch.randn(n, generator=gen, dtype=torch.float64) * (torch.arange(n) % 3 != 0)
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([param], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 7):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** torch.randint(-6, 3, (n,), generator=gen).double()
        param.grad = g * gscale
        opt.step()
        p, m, v = torch_order_step(p, g, m, v, HYPER[name], step, gscale)
        st = opt.state[param]
        for mine, theirs in ((p, param.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert float((mine - theirs).abs().max()) <= 1e-12 * float(theirs.abs().max()), (name, gscale, step)


def _key(case):
    if case["kind"] == "flat":
        return flat_key(case["n"])
    lay = layout(case)
    return seg_key(case["chunk"], lay["seg_n"], lay["chunk_seg"], lay["chunk_start"], fake_grad_addresses(case, lay), case["bias"] is not None)


@pytest.mark.parametrize("case", ADAMW_CASES, ids=case_id)
def test_row_runs_its_declared_cell(case):
    assert _key(case) == case["key"]
    if case["kind"] == "seg":
        lay = layout(case)
        assert case["chunk"] >= 4 and case["chunk"] % 4 == 0 and all(o % 4 == 0 for o in lay["seg_off"] + lay["chunk_start"])      # kanconv.h
        ends = [o + n for o, n in zip(lay["seg_off"], lay["seg_n"])]
        assert all(e <= o for e, o in zip(ends, lay["seg_off"][1:])) and ends[-1] <= lay["n_blk"]          # segments do not overlap
        assert all(0 <= s < lay["seg_n"][sg] for sg, s in zip(lay["chunk_seg"], lay["chunk_start"]))        # every chunk starts inside its segment


def test_every_reachable_cell_has_a_row():
    keys = [c["key"] for c in ADAMW_CASES]
    have_flat = {k for k in keys if k[0] == "flat"}
    have_seg = {(k[1], k[2] == "bias", cell) for k in keys if k[0] == "seg" for cell in k[4]}
    assert not set(REACHABLE_FLAT) - have_flat, f"flat cells without a row: {sorted(set(REACHABLE_FLAT) - have_flat)}"
    assert not set(REACHABLE_SEG) - have_seg, f"segment cells without a row: {sorted(set(REACHABLE_SEG) - have_seg)}"
    assert not have_flat - set(REACHABLE_FLAT), "a row reaches a flat cell the list of reachable cells does not know"
    assert {k[3] for k in keys if k[0] == "seg"} == {"none", "some", "all"}
    assert {(c["chunk"], c["bucket"]) for c in ADAMW_CASES if c["kind"] == "seg"} >= {(1024, False), (1024, True), (8192, False), (8192, True)}
    sizes = [c["n"] for c in ADAMW_CASES if c["kind"] == "flat"]
    assert sizes == [1, 2, 3, 4, 1023, 1024, 1025, 99998, 4096 * 1024, 4096 * 1024 + 4, 4096 * 1024 + 7]
    assert [c["n"] for c in ADAMW_CASES if c["kind"] == "flat" and c["n"] > 100_000] == sizes[-3:]              # the only large rows
    assert max(n_elems(c) for c in ADAMW_CASES if c["kind"] == "seg") < 100_000
    tiny = [c for c in ADAMW_CASES if c["kind"] == "seg" and len(c["segs"]) >= 2000]
    assert tiny and max(n for n, _ in tiny[0]["segs"]) <= 8


def test_free_attributes_vary_in_both_classes():
    for kind in ("flat", "seg"):
        rows = [c for c in ADAMW_CASES if c["kind"] == kind]
        assert {c["hyper"] for c in rows} == set(HYPER), kind
        assert {c["step"] for c in rows if not c.get("bias")} == set(STEPS), kind
        assert {c["gscale"] for c in rows} == set(GSCALES), kind
        assert {c["state"] for c in rows} == {"zero", "rand"}, kind
    bias = [c for c in ADAMW_CASES if c["kind"] == "seg" and c["bias"]]
    assert all(len(set(c["bias"])) > 1 and len(c["bias"]) == len(c["segs"]) for c in bias) and len(bias) >= 2


def test_flatten_row_yields_the_declared_tables():
    case = next(c for c in ADAMW_CASES if c["kind"] == "seg" and c["flatten"])
    assert [n for n, _ in case["segs"]] == [20003, 5, 64, 8192]
    from convkan_amd import optim
    assert case["chunk"] == optim._CHUNK
    lay = layout(case)
    params = [torch.nn.Parameter(torch.zeros(n)) for n, _ in case["segs"]]
    flat = K.FusedAdamW(params)._flat[0]
    for name in ("seg_off", "seg_n", "chunk_seg", "chunk_start"):
        assert flat["tab"][name].tolist() == lay[name], name
    assert flat["n"] == lay["n_blk"] and flat["tab"]["seg_off"].dtype == torch.int64 and flat["tab"]["seg_n"].dtype == torch.int32
    assert flat["tab"]["chunk_seg"].dtype == flat["tab"]["chunk_start"].dtype == torch.int32


@pytest.mark.parametrize("idx", range(len(ADAMW_CASES)), ids=[case_id(c) for c in ADAMW_CASES])
def test_kernel_arithmetic_passes_and_mask_stays_under_cap(idx):
    case = ADAMW_CASES[idx]
    inp, r64, r32 = reference_pair(idx)
    keep = judged_elems(case, inp, r64)
    assert float((~keep).float().mean()) <= MASK_CAP and (bool(keep.all()) or case["mask"]), "a row masks only for a reason it names, under the cap"
    for r in (r64, r32):                                                 # the references alone: nothing else would need masking
        assert all(bool(torch.isfinite(r[k][keep]).all()) for k in "pmv")
    assert bool((r64["v"] >= 0).all())
    lines, bad = judge(case, inp, kernel_restatement(case, inp), r64, r32)
    print(f"[adamw cpu] {case_id(case)}: " + "; ".join(lines))
    assert not bad, f"{case_id(case)}:\n  " + "\n  ".join(bad)


def test_judge_rejects_every_wrong_restatement():
    rejected = {w: [] for w in WRONG}
    for idx in SMALL:
        case = ADAMW_CASES[idx]
        inp, r64, r32 = reference_pair(idx)
        for w in WRONG:
            if judge(case, inp, kernel_restatement(case, inp, w), r64, r32)[1]:
                rejected[w].append(idx)
    for w, rows in rejected.items():
        print(f"[adamw cpu] {w}: rejected on rows {rows}")
    assert all(rejected.values()), f"never rejected: {[w for w, r in rejected.items() if not r]}"
    b00 = [i for i in SMALL if ADAMW_CASES[i]["hyper"] == "b00" and ADAMW_CASES[i]["state"] == "rand"]
    assert set(b00) & set(rejected["one_branch_lerp"]), "the one-branch lerp must fall on a betas = (0, 0) row"


def test_special_values_reference():
    inp, poisoned = special_inputs()
    r = special_reference(inp)
    lr, _, _, wd = HYPER["all"]
    assert poisoned.tolist() == [i in (1, 6, 8, 17) for i in range(19)]
    for k in "pmv":
        assert not bool(torch.isfinite(r[k][poisoned]).any()) and bool(torch.isfinite(r[k][~poisoned] if k != "v" else r["p"][~poisoned]).all())
    for i in (0, 14):                                                    # g = 0 on zero moments: decay only
        assert float(r["m"][i]) == 0.0 and float(r["v"][i]) == 0.0 and float(r["p"][i]) == float(inp["p"][i] * (1 - lr * wd))
    for i in (11, 12):                                                   # |g| = 1e20
        assert math.isinf(float(r["v"][i])) and math.isfinite(float(r["p"][i])) and math.isfinite(float(r["m"][i]))
