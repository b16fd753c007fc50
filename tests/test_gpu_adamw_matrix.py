"""Every row of the AdamW cell matrix (tests/adamw_cells.py) once through ctypes on torch's current stream: flat rows through
kan_adamw_step, segment rows through kan_adamw_step_segments with tables built here (the `flatten` row: by FusedAdamW._flatten).

Per row:
  - p, m and v live inside larger buffers filled with a NaN-pattern sentinel: 64 sentinel elements on each side, and the sentinel in every
    gap between segments;
  - after the launch the results are judged against the fp64 reference (adamw_cells.judge: tolerance max(2e-6, 4 x the fp32 CPU execution's
    own error, measured live)); every sentinel, border and gap, is intact; a segment with a null gradient is bit-unchanged in all three
    blocks; every gradient buffer and every table is bit-unchanged;
  - a second run on fresh copies is bit-identical (nothing here is atomic).
Then: n = 0 and n_chunks = 0 write nothing; the special-value row (g = 0 on zero moments, NaN, +-inf, 1e20) by class against the fp32 CPU run,
through both kernels and both paths of the segment kernel; the host-side refusals of both entry points.
Not covered: a chunk table that points outside its buffers is never handed to the device.  Measured figures: DESIGN.md section 4d."""
import ctypes as C

import pytest
import torch

from adamw_cells import (ADAMW_CASES, HYPER, SPECIAL_HYPER, SPECIAL_STEP, bias_table, case_id, judge, judge_special, layout, reference_pair, seg_key,
                         special_inputs, special_reference)

pytestmark = pytest.mark.gpu

PAD = 64                      # sentinel elements on each side of a guarded block
SENT_F = 0x7FA5A5A5           # (test_gpu_bnorm_matrix.py's NaN pattern: no kernel writes it)


def _guarded(n):
    """(buffer, view): n floats placed PAD elements into a larger buffer filled with the sentinel; the view is 256-byte aligned."""
    buf = torch.full((n + 2 * PAD,), SENT_F, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[PAD:PAD + n]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hyper_args(case):
    lr, (b1, b2), eps, wd = HYPER[case["hyper"]]
    return lr, b1, b2, eps, wd, case["step"], case["gscale"]


def _run_flat(lib, case, inp):
    """Returns (dense results {p, m, v}, findings)."""
    from convkan_amd import _lib as L
    n = case["n"]
    bufs = {k: _guarded(n) for k in "pmv"}
    for k in "pmv":
        bufs[k][1].copy_(inp[k])
    g = inp["g"].cuda()
    g0 = g.clone()
    L.check(lib.kan_adamw_step(_p(bufs["p"][1]), _p(g), _p(bufs["m"][1]), _p(bufs["v"][1]), n, *_hyper_args(case), _stream()), "kan_adamw_step")
    torch.cuda.synchronize()
    bad = []
    for k in "pmv":
        raw = bufs[k][0].view(torch.int32)
        if not (bool((raw[:PAD] == SENT_F).all()) and bool((raw[-PAD:] == SENT_F).all())):
            bad.append(f"{k}: memory next to the block was written")
    if not torch.equal(g.view(torch.int32), g0.view(torch.int32)):
        bad.append("the gradient was written")
    return {k: bufs[k][1].clone() for k in "pmv"}, bad


def _run_seg(lib, case, inp, flatten_tab=None):
    from convkan_amd import _lib as L
    lay = layout(case)
    segs, nb = case["segs"], lay["n_blk"]
    pos = torch.cat([torch.arange(o, o + n) for o, n in zip(lay["seg_off"], lay["seg_n"])])       # block position of every dense element
    gap = torch.ones(nb, dtype=torch.bool)
    gap[pos] = False
    gap, pos_d = gap.cuda(), pos.cuda()
    bufs = {k: _guarded(nb) for k in "pmv"}
    for k in "pmv":
        bufs[k][1][pos_d] = inp[k].cuda()
    # gradients: views of one flat bucket, or one allocation each; a view starts `offset` floats past a 16-byte boundary
    grads, stores = [], []
    if case["bucket"]:
        host = torch.full((lay["n_bucket"],), 7.0)
        for i, (n, goff) in enumerate(segs):
            if goff is not None:
                host[lay["grad_pos"][i]:lay["grad_pos"][i] + n] = inp["g"][lay["elem_off"][i]:lay["elem_off"][i] + n]
        stores.append(host.cuda())
    for i, (n, goff) in enumerate(segs):
        if goff is None:
            grads.append(None)
            continue
        if case["bucket"]:
            view = stores[0][lay["grad_pos"][i]:lay["grad_pos"][i] + n]
        else:
            stores.append(torch.full((n + goff + 1,), 7.0, device="cuda"))
            view = stores[-1][goff:goff + n]
            view.copy_(inp["g"][lay["elem_off"][i]:lay["elem_off"][i] + n])
        assert view.data_ptr() & 15 == 4 * goff
        grads.append(view)
    addr = [0 if g is None else g.data_ptr() for g in grads]
    assert seg_key(case["chunk"], lay["seg_n"], lay["chunk_seg"], lay["chunk_start"], addr, case["bias"] is not None) == case["key"]
    dev = lambda xs, dt: torch.tensor(xs, dtype=dt, device="cuda")
    if flatten_tab is not None:                                          # the optimizer's own device tables
        tab = {k: flatten_tab[k] for k in ("seg_off", "seg_n", "chunk_seg", "chunk_start")}
        assert all(tab[k].tolist() == lay[k] for k in tab)
    else:
        tab = dict(seg_off=dev(lay["seg_off"], torch.int64), seg_n=dev(lay["seg_n"], torch.int32), chunk_seg=dev(lay["chunk_seg"], torch.int32),
                   chunk_start=dev(lay["chunk_start"], torch.int32))
    tab["seg_grad"] = dev(addr, torch.int64)
    if case["bias"] is not None:
        tab["seg_bias"] = dev(bias_table(case["hyper"], case["bias"]), torch.float32)
    before = {k: t.clone() for k, t in tab.items()}
    stores0 = [s.clone() for s in stores]
    L.check(lib.kan_adamw_step_segments(_p(bufs["p"][1]), _p(bufs["m"][1]), _p(bufs["v"][1]), _p(tab["seg_grad"]), _p(tab["seg_off"]), _p(tab["seg_n"]),
                                        _p(tab["chunk_seg"]), _p(tab["chunk_start"]), _p(tab.get("seg_bias")), len(lay["chunk_seg"]), case["chunk"],
                                        *_hyper_args(case), _stream()), "kan_adamw_step_segments")
    torch.cuda.synchronize()
    bad, out = [], {}
    for k in "pmv":
        raw, blk = bufs[k][0].view(torch.int32), bufs[k][1]
        if not (bool((raw[:PAD] == SENT_F).all()) and bool((raw[-PAD:] == SENT_F).all())):
            bad.append(f"{k}: memory next to the block was written")
        if not bool((blk.view(torch.int32)[gap] == SENT_F).all()):
            bad.append(f"{k}: {int((blk.view(torch.int32)[gap] != SENT_F).sum())} elements in the gaps between segments were written")
        out[k] = blk[pos_d]
        same = out[k].cpu().view(torch.int32) == inp[k].view(torch.int32)
        for i, (n, goff) in enumerate(segs):
            if goff is None and not bool(same[lay["elem_off"][i]:lay["elem_off"][i] + n].all()):
                bad.append(f"{k}: segment {i} has a null gradient and changed")
    for k, t in tab.items():
        if not torch.equal(t, before[k]):
            bad.append(f"table {k} was written")
    if not all(torch.equal(s.view(torch.int32), s0.view(torch.int32)) for s, s0 in zip(stores, stores0)):
        bad.append("a gradient buffer was written")
    return out, bad


def _run(lib, case, inp):
    if case["kind"] == "flat":
        return _run_flat(lib, case, inp)
    tab = None
    if case["flatten"]:
        from convkan_amd import FusedAdamW
        group = dict(params=[torch.nn.Parameter(torch.zeros(n, device="cuda")) for n, _ in case["segs"]])
        tab = FusedAdamW._flatten(group)["tab"]
    return _run_seg(lib, case, inp, tab)


@pytest.mark.parametrize("idx", range(len(ADAMW_CASES)), ids=[case_id(c) for c in ADAMW_CASES])
def test_adamw_cell_vs_fp64(idx, gpu_lib):
    case = ADAMW_CASES[idx]
    inp, r64, r32 = reference_pair(idx)
    got, bad = _run(gpu_lib, case, inp)
    again, bad2 = _run(gpu_lib, case, inp)
    lines, wrong = judge(case, inp, got, r64, r32)
    print(f"[adamw] {case_id(case)}: " + "; ".join(lines))
    bad += wrong + [b + " (second run)" for b in bad2 if b not in bad]
    for k in "pmv":
        if not torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)):
            bad.append(f"{k}: two runs on the same inputs differ in {int((got[k].view(torch.int32) != again[k].view(torch.int32)).sum())} elements")
    if case["key"][0] == "seg" and case["key"][3] == "all":
        assert all(torch.equal(got[k].cpu().view(torch.int32), inp[k].view(torch.int32)) for k in "pmv"), "all gradients null: nothing may change"
    assert not bad, f"{case_id(case)} ({case['why']}):\n  " + "\n  ".join(bad)


def test_empty_launches_write_nothing(gpu_lib):
    bufs = [_guarded(8) for _ in range(4)]
    p, g, m, v = (b[1] for b in bufs)
    assert gpu_lib.kan_adamw_step(_p(p), _p(g), _p(m), _p(v), 0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0, _stream()) == 0
    tabs = [torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(5)]
    assert gpu_lib.kan_adamw_step_segments(_p(p), _p(m), _p(v), *(_p(t) for t in tabs), _p(None), 0, 8192, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0,
                                           _stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((b[0].view(torch.int32) == SENT_F).all()) for b in bufs)


def test_special_values_by_class(gpu_lib):
    """g = 0 on zero moments leaves p * decay and zero moments; NaN / +-inf poison their own element's p, m and v and no other lane of their
    float4, no neighbour; |g| = 1e20 overflows v with a finite p.  Flat kernel (float4 body and tail), segment kernel on both paths."""
    from convkan_amd import _lib as L
    inp, poisoned = special_inputs()
    r32 = special_reference(inp)
    n = inp["p"].numel()
    lr, (b1, b2), eps, wd = HYPER[SPECIAL_HYPER]
    hyper = (lr, b1, b2, eps, wd, SPECIAL_STEP, 1.0)
    runs = {}
    dev = {k: t.cuda() for k, t in inp.items()}
    L.check(gpu_lib.kan_adamw_step(_p(dev["p"]), _p(dev["g"]), _p(dev["m"]), _p(dev["v"]), n, *hyper, _stream()), "kan_adamw_step")
    runs["flat"] = dev
    for name, goff in (("segments, float4 path", 0), ("segments, scalar path", 1)):
        dev = {k: inp[k].cuda() for k in "pmv"}
        store = torch.zeros(n + 8, device="cuda")
        g = store[goff:goff + n]
        g.copy_(inp["g"])
        t = lambda xs, dt: torch.tensor(xs, dtype=dt, device="cuda")
        tab = [t([g.data_ptr()], torch.int64), t([0], torch.int64), t([n], torch.int32), t([0], torch.int32), t([0], torch.int32)]
        L.check(gpu_lib.kan_adamw_step_segments(_p(dev["p"]), _p(dev["m"]), _p(dev["v"]), *(_p(x) for x in tab), _p(None), 1, 8192, *hyper, _stream()), name)
        runs[name] = dev
    torch.cuda.synchronize()
    bad = [f"{name}: {b}" for name, got in runs.items() for b in judge_special(inp, poisoned, got, r32)]
    assert not bad, "\n  ".join(bad)


def test_argument_refusals(gpu_lib):
    """Host-side returns: no device work runs (the pointers are never dereferenced)."""
    ok, odd, null = C.c_void_p(4096), C.c_void_p(4096 + 4), C.c_void_p(0)
    st = null

    def flat(**kw):
        a = dict(p=ok, g=ok, m=ok, v=ok, n=8, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=1, gs=1.0, st=st) | kw
        return gpu_lib.kan_adamw_step(*a.values())

    def segm(**kw):
        a = dict(p=ok, m=ok, v=ok, seg_grad=ok, seg_off=ok, seg_n=ok, chunk_seg=ok, chunk_start=ok, seg_bias=null, n_chunks=1, chunk=8192, lr=1e-3,
                 b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=1, gs=1.0, st=st) | kw
        return gpu_lib.kan_adamw_step_segments(*a.values())

    def refused(rc, what):
        assert rc != 0 and gpu_lib.kan_last_error(), what

    for k in "pgmv":
        refused(flat(**{k: odd}), f"flat: misaligned {k}")
        refused(flat(**{k: null}), f"flat: null {k}")
    for bad in (dict(step=0), dict(step=-1), dict(n=-1)):
        refused(flat(**bad), f"flat: {bad}")
    for k in "pmv":
        refused(segm(**{k: odd}), f"segments: misaligned {k}")
    for k in ("p", "m", "v", "seg_grad", "seg_off", "seg_n", "chunk_seg", "chunk_start"):
        refused(segm(**{k: null}), f"segments: null {k}")
    for bad in (dict(step=0), dict(chunk=0), dict(chunk=-4), dict(chunk=2), dict(chunk=6), dict(chunk=8191), dict(n_chunks=-1)):
        refused(segm(**bad), f"segments: {bad}")
